"""The device eigensolver (gprx_eigh_*) at production sizes against numpy.linalg.eigh on the same
machine, and PreProcessor.fit host to host by both eigensolver routes.  One JSON line per measurement; everything is also
written to --out.

    python tools/eigh_probe.py [--sizes 256,512,1024,2048,4096,8192] [--fits 1000x200000,2000x100000,4096x50000] [--out profiles/eigh_probe.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/eigh_probe.py --solve-only 2048     (the per-phase split)

Device times: a host clock around gprx_eigh_dev, which returns after a device synchronise; the matrix is uploaded outside the
window (the solver overwrites it).  Matrices: the Gram matrix of centred field-like rows (12 strong modes plus noise, cells = 4 n).
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpras_amd import _lib  # noqa: E402
from gpras_amd.eigh import SymmetricEigensolver  # noqa: E402
from gpras_amd.preprocess import PreProcessor  # noqa: E402

EPS = np.finfo(np.float64).eps


def gram(n, seed=0):
    rng = np.random.default_rng(seed)
    r, cells = 12, 4 * n
    amp = rng.standard_normal((n, r)) * (3.0 * 0.7 ** np.arange(r))
    x = 0.5 * amp @ rng.standard_normal((r, cells)) + 0.01 * rng.standard_normal((n, cells))
    x -= x.mean(axis=0)
    return x @ x.T


def field(n_s, cells, seed=0):
    rng = np.random.default_rng(seed)
    r = 12
    elev = 10.0 + 2.0 * rng.random(cells)
    elev[rng.random(cells) < 0.1] += 50.0
    amp = rng.standard_normal((n_s, r)) * (3.0 * 0.7 ** np.arange(r))
    x = 11.0 + 0.5 * amp @ rng.standard_normal((r, cells)) + 0.01 * rng.standard_normal((n_s, cells))
    return np.ascontiguousarray(x), elev, 0.5 + rng.random(cells)


def device_solve(solver, g, reps):
    n = g.shape[0]
    a_dev, lam_dev, v_dev = _lib.DeviceBuffer(g.nbytes), _lib.DeviceBuffer(8 * n), _lib.DeviceBuffer(g.nbytes)
    try:
        times = []
        for _ in range(reps):
            _lib.check(_lib.load().gprx_memcpy_h2d(0, a_dev.ptr, _lib.ptr(g), g.nbytes))
            t0 = time.perf_counter()
            solver.eigh_dev(n, a_dev.ptr, n, lam_dev.ptr, v_dev.ptr, n)
            times.append((time.perf_counter() - t0) * 1e3)
        return times, lam_dev.to_array((n,)), v_dev.to_array((n, n))
    finally:
        for buf in (a_dev, lam_dev, v_dev):
            buf.free()


def solve_record(n, reps, with_host=True):
    g = gram(n)
    with SymmetricEigensolver(n) as solver:
        times, lam, v = device_solve(solver, g, reps)
        sweeps, off_rel = solver.info
    rec = dict(kind="solve", n=n, block=32, device_ms=[round(t, 2) for t in times], sweeps=sweeps, off_rel=off_rel)
    norm = np.linalg.norm(g)
    rec["residual_over_n_eps_norm"] = round(float(np.linalg.norm(g @ v - v * lam) / (n * EPS * norm)), 3)
    rec["ortho_over_sqrt_n_eps"] = round(float(np.max(np.abs(v.T @ v - np.eye(n))) / (np.sqrt(n) * EPS)), 2)
    if with_host:
        t0 = time.perf_counter()
        want = np.linalg.eigh(g)[0]
        rec["numpy_eigh_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        rec["numpy_threads"] = os.environ.get("OMP_NUM_THREADS")
        rec["eigenvalue_err_over_max"] = float(np.max(np.abs(lam - want)) / np.max(np.abs(want)))
    return rec


def fit_record(n_s, cells, reps):
    x, elev, w = field(n_s, cells)
    rec = dict(kind="fit", shape=[n_s, cells])
    for route in ("host", "device"):
        pre = PreProcessor(hydraulic_parameter="wse")
        pre.eigensolver = route
        runs = []
        for _ in range(reps):
            t0 = time.perf_counter()
            pre.fit(x, elev, w, None)
            runs.append(((time.perf_counter() - t0) * 1e3, dict(pre.last_timings_ms)))
        ms, ph = min(runs, key=lambda r: r[0])
        rec[route] = dict(fit_host_ms=round(ms, 1), all_ms=[round(r[0], 1) for r in runs], k=int(pre.spatial_mode_count),
                          phases_ms={k: round(v, 2) for k, v in ph.items()})
        if route == "device":
            rec[route]["sweeps"] = pre.last_eig_sweeps
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024,2048,4096,8192")
    ap.add_argument("--fits", default="1000x200000,2000x100000,4096x50000")
    ap.add_argument("--solve-only", type=int, default=0, help="one device solve of this size and nothing else (for a kernel trace)")
    ap.add_argument("--reps", type=int, default=3, help="timed repetitions per size and per fit route; every one is recorded")
    ap.add_argument("--out", default=os.path.join("profiles", "eigh_probe.json"))
    args = ap.parse_args()
    solve_record(256, 1, with_host=False)  # warm-up: code objects, the LDS attribute
    if args.solve_only:
        print(json.dumps(solve_record(args.solve_only, 1, with_host=False)), flush=True)
        return
    records = []
    for n in (int(v) for v in args.sizes.split(",") if v):
        records.append(solve_record(n, args.reps))
        print(json.dumps(records[-1]), flush=True)
    for spec in (s for s in args.fits.split(",") if s):
        n_s, cells = (int(v) for v in spec.split("x"))
        records.append(fit_record(n_s, cells, args.reps))
        print(json.dumps(records[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(block_widths_built=[32], records=records), f, indent=1)


if __name__ == "__main__":
    main()
