"""PreProcessor.fit on the device at production size: one JSON line per shape with the host-to-host fit time, the
per-phase device times (gprx_pcafit_timings: upload, statistics, centring, Gram, components, projection), the host eigh,
the Gram's rate against the fp64 MFMA peak, the raw H2D time of x in the same process and, where scikit-learn is
importable, the reference's IncrementalPCA fit on the host.

    python tools/pca_fit_probe.py [--shapes 300x1000000,500x200000] [--no-sklearn]
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

PEAK_TFLOPS = 78.6


def field(n_s, cells, seed=0):
    rng = np.random.default_rng(seed)
    r = 12
    elev = 10.0 + 2.0 * rng.random(cells)
    elev[rng.random(cells) < 0.1] += 50.0
    amp = rng.standard_normal((n_s, r)) * (3.0 * 0.7 ** np.arange(r))
    x = 11.0 + 0.5 * amp @ rng.standard_normal((r, cells)) + 0.01 * rng.standard_normal((n_s, cells))
    return np.ascontiguousarray(x), elev, 0.5 + rng.random(cells)


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
    ap.add_argument("--shapes", default="300x1000000,500x200000")
    ap.add_argument("--no-sklearn", action="store_true")
    args = ap.parse_args()
    for spec in args.shapes.split(","):
        n_s, cells = (int(v) for v in spec.split("x"))
        x, elev, w = field(n_s, cells)
        pre = PreProcessor(hydraulic_parameter="wse")
        pre.fit(x[:, : max(n_s, 1024)].copy(), elev[: max(n_s, 1024)], w[: max(n_s, 1024)], 4)  # warm-up (module load, kernels)
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            pre.fit(x, elev, w, None)
            runs.append(((time.perf_counter() - t0) * 1e3, dict(pre.last_timings_ms)))
        host_ms, ph = min(runs, key=lambda r: r[0])
        n_wet = int(pre.input_mean.size)
        tiles = (n_s + 63) // 64
        gram_flops = 2.0 * (tiles * (tiles + 1) // 2) * 64 * 64 * n_wet  # the 64 x 64 tiles computed (lower triangle), 2 flops per FMA
        t0 = time.perf_counter()
        np.linalg.eigh(np.eye(n_s) + 1e-3 * np.ones((n_s, n_s)))
        eigh_ms = (time.perf_counter() - t0) * 1e3
        out = dict(shape=[n_s, cells], n_wet=n_wet, k=int(pre.spatial_mode_count), fit_host_ms=round(host_ms, 2),
                   phases_ms={k: round(v, 3) for k, v in ph.items()}, host_eigh_ms=round(eigh_ms, 2),
                   gram_tflops=round(gram_flops / (ph["gram"] * 1e-3) / 1e12, 2) if ph["gram"] > 0 else None,
                   raw_h2d_ms=round(raw_h2d_ms(x), 2), x_gib=round(x.nbytes / 2**30, 3))
        out["gram_frac_of_peak"] = round(out["gram_tflops"] / PEAK_TFLOPS, 3) if out["gram_tflops"] else None
        out["fit_over_h2d"] = round(host_ms / out["raw_h2d_ms"], 2)
        if not args.no_sklearn:
            try:
                from sklearn.decomposition import IncrementalPCA

                dry = pre.dry_indices
                xw = (x[:, ~dry] - pre.input_mean) * pre.weights
                t0 = time.perf_counter()
                IncrementalPCA().fit(xw)
                out["sklearn_fit_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                out["sklearn_threads"] = os.environ.get("OMP_NUM_THREADS")
            except ImportError:
                out["sklearn_fit_ms"] = None
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
