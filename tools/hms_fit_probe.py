"""HmsPreProcessor on the device at production size: one JSON line per shape with the host-to-host fit / transform times,
the per-phase device times (gprx_hms_timings: upload, column pass, covariance, components, projection, API, features) and the
host eigh, the raw H2D time of x in the same process and, where scikit-learn is importable, the reference's host path
(numpy + IncrementalPCA + np.convolve, restated in tests/hms_numpy.py) on this host's CPUs, labelled as such.

    python tools/hms_fit_probe.py [--shapes 20000x150x3,200000x400x4] [--no-host] [--out profiles/hms_fit_probe.json]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpras_amd import _lib  # noqa: E402
from gpras_amd.preprocess import HmsPreProcessor  # noqa: E402


def field(T, p, n_bc, seed=0):
    rng = np.random.default_rng(seed)
    r = 8
    amp = rng.standard_normal((T, r)) * (3.0 * 0.6 ** np.arange(r))
    x = np.empty((T, n_bc + p), order="F")
    x[:, n_bc:] = 2.0 + 0.3 * amp @ rng.standard_normal((r, p)) + 0.02 * rng.random((T, p))
    x[:, :n_bc] = 40.0 + 5.0 * rng.standard_normal((T, n_bc))
    pm = np.zeros(n_bc + p, dtype=bool)
    pm[n_bc:] = True
    return x, ~pm, pm


def raw_h2d_ms(x):
    buf = _lib.DeviceBuffer(x.nbytes)
    try:
        best = 1e30
        for _ in range(3):
            t0 = time.perf_counter()
            _lib.check(_lib.load().gprx_memcpy_h2d(0, buf.ptr, _lib.ptr(x), x.nbytes))
            best = min(best, (time.perf_counter() - t0) * 1e3)
        return best
    finally:
        buf.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20000x150x3,200000x400x4")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for spec in args.shapes.split(","):
        T, p, n_bc = (int(v) for v in spec.split("x"))
        x, bm, pm = field(T, p, n_bc)
        pre = HmsPreProcessor()
        pre.fit(x[:2000], bm, pm)  # warm-up (module load, kernels)
        fits, trans = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            pre.fit(x, bm, pm)
            fits.append(((time.perf_counter() - t0) * 1e3, dict(pre.last_timings_ms)))
        for _ in range(3):
            t0 = time.perf_counter()
            pre.transform(x)
            trans.append(((time.perf_counter() - t0) * 1e3, dict(pre.last_timings_ms)))
        fit_ms, ph = min(fits, key=lambda r: r[0])
        tr_ms, ph_t = min(trans, key=lambda r: r[0])
        out = dict(shape=[T, p, n_bc], x_order="F", k=int(pre.precip_spatial_mode_count), fit_host_ms=round(fit_ms, 2),
                   fit_phases_ms={k: round(v, 3) for k, v in ph.items()}, transform_host_ms=round(tr_ms, 2),
                   transform_phases_ms={k: round(v, 3) for k, v in ph_t.items() if k not in ("column_pass", "covariance", "components", "host_eigh")},
                   raw_h2d_ms=round(raw_h2d_ms(np.ascontiguousarray(x)), 2), x_mib=round(x.nbytes / 2**20, 1))
        out["fit_over_h2d_plus_eigh"] = round(fit_ms / (out["raw_h2d_ms"] + ph["host_eigh"]), 2)
        xc = np.ascontiguousarray(x)
        t0 = time.perf_counter()
        pre.fit(xc, bm, pm)
        out["fit_host_ms_c_order"] = round((time.perf_counter() - t0) * 1e3, 2)
        out["fit_phases_ms_c_order"] = {k: round(v, 3) for k, v in pre.last_timings_ms.items()}
        if not args.no_host:
            try:
                from sklearn.decomposition import IncrementalPCA

                from hms_numpy import api

                host = {}
                t0 = time.perf_counter()
                xm = x - x.mean(axis=0)
                xp = xm[:, pm]
                host["centre_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                t0 = time.perf_counter()
                IncrementalPCA().fit(xp)
                host["incremental_pca_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                avg = xp.mean(axis=1)
                t0 = time.perf_counter()
                api(avg)
                host["api_k085_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                t0 = time.perf_counter()
                api(avg, k=1)
                host["api_k1_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                host["cpus"] = os.environ.get("OMP_NUM_THREADS")
                out["host_numpy_sklearn"] = host
            except ImportError:
                out["host_numpy_sklearn"] = None
        print(json.dumps(out), flush=True)
        rows.append(out)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
