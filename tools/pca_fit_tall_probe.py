"""The covariance route of PreProcessor.fit (``sample_route = "auto"``, n_samples > n_wet) at production size: per shape the
host-to-host fit time, the per-stage device times (gprx_pcafit_timings: upload, statistics, centring, covariance, components,
projection) with the row-split kernels and, as the yardstick, with ``"pcafit_rowsplit"`` = 0 (the one-thread-per-cell kernels of the
Gram route on the same operation list), the host eigh, the raw H2D time of x in the same process and, where scikit-learn is
importable and the shape allows it in reasonable time, the reference's IncrementalPCA fit on the host.

    python tools/pca_fit_tall_probe.py [--shapes 20000x2000,200000x4000,100000x16000] [--sklearn-max-cells 4000] [--out FILE]
"""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpras_amd import _lib  # noqa: E402
from gpras_amd.preprocess import PreProcessor  # noqa: E402

STAGES = ("upload", "stats", "centring", "covariance", "components", "projection")


def field(n_s, cells, seed=0):
    """Low-rank signal plus noise, a tenth of the cells always dry; built in row blocks to keep the temporaries small."""
    rng = np.random.default_rng(seed)
    r = 12
    elev = 9.5 + 1.5 * rng.random(cells)
    elev[rng.random(cells) < 0.1] += 50.0
    pat = rng.standard_normal((r, cells))
    scales = 3.0 * 0.7 ** np.arange(r)
    x = np.empty((n_s, cells))
    for t0 in range(0, n_s, 8192):
        t1 = min(n_s, t0 + 8192)
        blk = rng.standard_normal((t1 - t0, cells), out=x[t0:t1])
        blk *= 0.01
        blk += 11.0 + 0.5 * (rng.standard_normal((t1 - t0, r)) * scales) @ pat
    return x, elev, 0.5 + rng.random(cells)


def raw_h2d_ms(x):
    buf = _lib.DeviceBuffer(x.nbytes)
    try:
        best = 1e30
        for _ in range(2):
            t0 = time.perf_counter()
            _lib.check(_lib.load().gprx_memcpy_h2d(0, buf.ptr, _lib.ptr(x), x.nbytes))
            best = min(best, (time.perf_counter() - t0) * 1e3)
        return best
    finally:
        buf.free()


def create_stage_ms(x, elev, w, rowsplit, repeats):
    """Device milliseconds of the stages inside gprx_pcafit_create_auto (no eigendecomposition), best total of ``repeats``."""
    lib = _lib.load()
    best = None
    _lib.check(lib.gprx_set_tuning(b"pcafit_rowsplit", rowsplit))
    try:
        for _ in range(repeats):
            h, route = C.c_void_p(), C.c_int(-1)
            _lib.check(lib.gprx_pcafit_create_auto(0, _lib.ptr(x), x.shape[0], x.shape[1], _lib.ptr(elev), _lib.ptr(w), 0, 0.03, C.byref(route), C.byref(h)))
            try:
                assert _lib.PCAFIT_ROUTES[route.value] == "covariance"
                ms = np.zeros(6)
                _lib.check(lib.gprx_pcafit_timings(h, ms.ctypes.data_as(C.POINTER(C.c_double))))
            finally:
                lib.gprx_pcafit_destroy(h)
            if best is None or ms[1] + ms[2] < best[1] + best[2]:
                best = ms
    finally:
        _lib.check(lib.gprx_set_tuning(b"pcafit_rowsplit", 1))
    return {k: round(float(v), 3) for k, v in zip(STAGES[:4], best[:4])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20000x2000,200000x4000,100000x16000")
    ap.add_argument("--sklearn-max-cells", type=int, default=4000, help="IncrementalPCA runs only up to this many cells (0: never)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    for spec in args.shapes.split(","):
        n_s, cells = (int(v) for v in spec.split("x"))
        big = n_s * cells > 2**28
        t0 = time.perf_counter()
        x, elev, w = field(n_s, cells)
        print(f"# {spec}: field built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        pre = PreProcessor(hydraulic_parameter="wse")
        pre.sample_route = "auto"
        pre.fit(x[:2048, :256].copy(), elev[:256], w[:256], 4)  # warm-up (module load, kernels)
        runs = []
        for _ in range(1 if big else 3):
            t0 = time.perf_counter()
            pre.fit(x, elev, w, None)
            runs.append(((time.perf_counter() - t0) * 1e3, dict(pre.last_timings_ms)))
            print(f"# {spec}: fit {runs[-1][0]:.0f} ms", file=sys.stderr, flush=True)
        assert pre.last_route == "covariance"
        host_ms, ph = min(runs, key=lambda r: r[0])
        n_wet = int(pre.input_mean.size)
        t0 = time.perf_counter()
        np.linalg.eigh(np.eye(n_wet) + 1e-3 * np.ones((n_wet, n_wet)))
        eigh_ms = (time.perf_counter() - t0) * 1e3
        tiles = (n_wet + 63) // 64
        cov_flops = 2.0 * (tiles * (tiles + 1) // 2) * 64 * 64 * n_s
        out = dict(shape=[n_s, cells], n_wet=n_wet, k=int(pre.spatial_mode_count), fit_host_ms=round(host_ms, 2),
                   stages_ms={k: round(v, 3) for k, v in ph.items() if k != "gram"}, host_eigh_ms=round(eigh_ms, 2),
                   covariance_tflops=round(cov_flops / (ph["covariance"] * 1e-3) / 1e12, 2), raw_h2d_ms=round(raw_h2d_ms(x), 2),
                   x_gib=round(x.nbytes / 2**30, 3))
        out["fit_over_h2d"] = round(host_ms / out["raw_h2d_ms"], 2)
        reps = 1 if big else 3
        out["create_rowsplit1_ms"] = create_stage_ms(x, elev, w, 1, reps)
        out["create_rowsplit0_ms"] = create_stage_ms(x, elev, w, 0, reps)
        out["rowsplit_speedup"] = {k: round(out["create_rowsplit0_ms"][k] / max(out["create_rowsplit1_ms"][k], 1e-9), 2) for k in ("stats", "centring")}
        print(f"# {spec}: yardstick done", file=sys.stderr, flush=True)
        out["sklearn_fit_ms"] = None
        if args.sklearn_max_cells and cells <= args.sklearn_max_cells:
            try:
                from sklearn.decomposition import IncrementalPCA

                xw = (x[:, ~pre.dry_indices] - pre.input_mean) * pre.weights
                t0 = time.perf_counter()
                IncrementalPCA().fit(xw)
                out["sklearn_fit_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                out["sklearn_threads"] = os.environ.get("OMP_NUM_THREADS")
                out["sklearn_over_fit"] = round(out["sklearn_fit_ms"] / host_ms, 2)
            except ImportError:
                pass
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del x


if __name__ == "__main__":
    main()
