"""The temporal clipping on the device at production size: per-stage device times of `gprx_al_cutoff_dev` (`gprx_al_timings`: NaN
scan, column normalisers, row sums, finish) over two device blocks of (T, n) each, the bytes each sweep must read and its rate
against the measured copy rate of the chip, the wall time of the numpy restatement of the rule (tests/align_numpy.py) on the same host, and the bytes
`EventAligner.aligned_features` moves over the host link against the download - clip - upload route.  One JSON document.

    python tools/align_probe.py [--rows 300] [--cells 100000] [--repeats 7] [--out profiles/align_probe.json]
"""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import align_numpy  # noqa: E402
from gpras_amd import _lib  # noqa: E402
from gpras_amd.align import EventAligner  # noqa: E402

COPY_TBS = 6.29  # measured copy rate of one MI355X
ROW_TILE = 32  # csrc/align.h AL_RT


def hydrograph(rng, T, n):
    t = np.arange(T, dtype=np.float64)[:, None]
    peak, width = T * (0.25 + 0.3 * rng.random(n)), T * (0.08 + 0.1 * rng.random(n))
    return np.ascontiguousarray(100.0 + 5.0 * rng.random(n) + (0.5 + 2.0 * rng.random(n)) * np.exp(-0.5 * ((t - peak) / width) ** 2))


def numpy_rule(combo, threshold):
    """The clipping rule on the host: the numpy restatement the tests hold the device to (tests/align_numpy.py)."""
    return align_numpy.get_cutoff(combo, threshold)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=300)
    ap.add_argument("--cells", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--modes", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    T, n = args.rows, args.cells
    rng = np.random.default_rng(1)
    hf, lf = hydrograph(rng, T, n), hydrograph(rng, T, n)
    lib = _lib.load()
    al = EventAligner()
    bufs = [_lib.DeviceBuffer.from_array(hf), _lib.DeviceBuffer.from_array(lf)]
    blocks = [(b.ptr, n, n) for b in bufs]
    field_bytes = 8.0 * T * 2 * n
    sweep_bytes = {"scan": field_bytes, "normalisers": field_bytes + 8.0 * 2 * n,
                   "row_sums": 8.0 * 2 * n * ((T - 1) + -(-(T - 1) // ROW_TILE)) + 8.0 * 2 * n}
    runs = []
    for i in range(2 + args.repeats):
        t0 = time.perf_counter()
        cut = al._cutoff_dev(blocks, T)[:2]
        wall = (time.perf_counter() - t0) * 1e3
        if i >= 2:  # two warm-up calls: code objects, the handle's scratch
            runs.append(dict(al.stage_timings_ms(), wall=wall))
    best = min(runs, key=lambda r: sum(v for k, v in r.items() if k != "wall"))
    doc = {"rows": T, "cells_per_block": n, "blocks": 2, "field_MB": field_bytes / 1e6, "cutoff": cut, "repeats": args.repeats,
           "stage_ms_best_call": {k: round(v, 4) for k, v in best.items()},
           "stage_ms_all": {k: [round(r[k], 4) for r in runs] for k in best},
           "sweep_GBps": {k: round(sweep_bytes[k] / (best[k] * 1e-3) / 1e9, 1) for k in sweep_bytes},
           "share_of_copy_rate": {k: round(sweep_bytes[k] / (best[k] * 1e-3) / (COPY_TBS * 1e12), 3) for k in sweep_bytes}}
    for b in bufs:
        b.free()

    combo = np.concatenate([hf, lf], axis=1)
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref_cut = numpy_rule(combo, 0.95)
        walls.append(time.perf_counter() - t0)
    doc["numpy_restatement_s"] = {"best_of_3": round(min(walls), 3), "threads": "numpy elementwise and reductions: 1 thread", "cutoff": ref_cut}
    assert tuple(ref_cut) == tuple(cut), (ref_cut, cut)
    del combo

    # plan blocks -> features: the bytes over the host link
    from gpras_amd.preprocess import EOFProjector
    from gpras_amd.resample import MeshResampler

    n_full, n_lf, k = n + n // 5, n // 5, args.modes
    gather = MeshResampler.nearest(rng.permutation(n_full)[:n], n_full)
    lf_rs = MeshResampler.nearest(rng.integers(0, n_lf, n), n_lf, 90.0 + rng.random(n))
    proj = [EOFProjector(np.zeros(n, dtype=bool), 90.0 + rng.random(n), 102.0 + rng.normal(size=n), rng.uniform(0.5, 1.5, size=n),
                         rng.normal(size=(k, n)) / np.sqrt(k), rng.normal(size=k), rng.uniform(0.5, 2, size=k), "wse") for _ in range(2)]
    plan = [("p", hydrograph(rng, T, n_full), hydrograph(rng, T, n_lf))]
    for i in range(2):
        al.cutoffs.clear()
        t0 = time.perf_counter()
        x, y, _, _ = al.aligned_features(plan, gather, lf_rs, proj[0], proj[1])
        wall = time.perf_counter() - t0
    dur = len(x)
    moved = al.last_timings_ms["host_link_bytes"]
    # the route without the device cutoff: raw rows up, both fields down, numpy clips, the kept rows up, the features down
    other = 8 * (T * (n_full + n_lf) + 2 * T * n + 2 * dur * n + 2 * dur * k)
    doc["aligned_features"] = {"rows_kept": dur, "modes": k, "hf_block_cells": n_full, "lf_block_cells": n_lf, "wall_s_second_call": round(wall, 3),
                               "split_ms": {a: round(v, 2) for a, v in al.last_timings_ms.items() if a != "host_link_bytes"},
                               "host_link_bytes": int(moved), "download_clip_upload_route_bytes": int(other), "ratio": round(other / moved, 2)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
