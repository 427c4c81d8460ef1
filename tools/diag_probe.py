"""Time the diagnostics sort (gprx_dg_sort_abs_residual_dev) and DevicePipeline.diagnostics against the route without them:
to_host() of the fields, then np.sort(np.abs(a - b).flatten()) on the host.  Writes one JSON record (profiles/diag_sort.json).

    python tools/diag_probe.py [--out PATH] [--sizes 1000000,10000000,100000000] [--rows 1400 --cells 100000]

Device times are HIP-event times of the library (gprx_dg_sort_info) and host clocks around calls that end in a synchronisation; every
shape is warmed up once and the median of the repeats is reported next to all of them.  Bytes per executed pass: the count sweep
reads 8 n, the scatter reads 8 n and writes 8 n (the first pass of the fused route reads the pair: 16 n each time).
"""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 6.29e12  # bytes/s, the measured device copy rate the sweeps are held against


def median(v):
    return float(np.median(v))


def sort_record(fd, lib, n, repeats):
    from gpras_amd._lib import DeviceBuffer, check

    rng = np.random.default_rng(n)
    a = 100.0 + rng.standard_normal(n)
    b = a + 0.1 * rng.standard_normal(n)
    da, db, out = DeviceBuffer.from_array(a), DeviceBuffer.from_array(b), DeviceBuffer(8 * n)
    try:
        wall, hist, passes = [], [], []
        for i in range(repeats + 1):
            t0 = time.perf_counter()
            check(lib.gprx_dg_sort_abs_residual_dev(fd.handle, da.ptr, db.ptr, n, out.ptr))
            t1 = time.perf_counter()
            info = fd.last_sort_info()
            if i:  # the first call warms up (code objects, the workspace)
                wall.append((t1 - t0) * 1e3)
                hist.append(info["histogram_ms"])
                passes.append(info["passes_ms"])
        got = out.to_array((n,))
        host = []
        for _ in range(1 if n > 20_000_000 else 3):
            t0 = time.perf_counter()
            ha, hb = da.to_array((n,)), db.to_array((n,))
            t1 = time.perf_counter()
            want = np.sort(np.abs(ha - hb).flatten())
            t2 = time.perf_counter()
            host.append({"to_host_s": t1 - t0, "numpy_sort_s": t2 - t1, "total_s": t2 - t0})
        executed = info["executed_passes"]
        first, later = 16.0 * n + 16.0 * n + 8.0 * n, 8.0 * n + 8.0 * n + 8.0 * n
        pass_bytes = first + later * (len(executed) - 1) if executed else 0.0
        rec = {
            "n": n, "equal_to_numpy_sort": bool(np.array_equal(got, want)), "executed_passes": executed, "skipped_passes": info["skipped_passes"],
            "wall_ms_median": median(wall), "histogram_ms_median": median(hist), "passes_ms_median": median(passes),
            "wall_ms_all": wall, "histogram_ms_all": hist, "passes_ms_all": passes,
            "histogram_GBps": 16.0 * n / (median(hist) * 1e-3) / 1e9,
            "bytes_per_executed_pass": pass_bytes / max(len(executed), 1),
            "pass_GBps": pass_bytes / (median(passes) * 1e-3) / 1e9 if executed else None,
            "pass_share_of_copy_rate": pass_bytes / (median(passes) * 1e-3) / COPY_RATE if executed else None,
            "host_route": host, "host_route_best_total_s": min(h["total_s"] for h in host),
        }
        rec["ratio_host_over_device"] = rec["host_route_best_total_s"] / (rec["wall_ms_median"] * 1e-3)
        return rec
    finally:
        for buf in (da, db, out):
            buf.free()


def pipeline_record(rows, cells, repeats):
    import pandas as pd

    from gpras_amd.gpr import GPRAS
    from gpras_amd.pipeline import DevicePipeline
    from gpras_amd.preprocess import EOFProjector

    rng = np.random.default_rng(7)
    n, d, m, k, events = 256, 4, 32, 8, 14
    x = rng.normal(size=(n, d))
    y = np.stack([np.sin(x @ rng.normal(size=d)) + 0.05 * rng.normal(size=n) for _ in range(k)], axis=1)
    gpr = GPRAS("Matern32")
    gpr.fit(x, y, m, "kmeans", "adam", max_iter=5)
    elev = rng.uniform(0.0, 2.0, size=cells)
    proj = EOFProjector(np.zeros(cells, dtype=bool), elev, rng.normal(size=cells) + 1.5, rng.uniform(0.5, 1.5, size=cells), rng.normal(size=(k, cells)) / np.sqrt(k),
                        rng.normal(size=k), rng.uniform(0.5, 2, size=k), hydraulic_parameter="wse")
    x_test = rng.normal(size=(rows, d))
    truth = rng.uniform(0.0, 3.0, size=(rows, cells)) + elev
    lf = truth + 0.3 * rng.standard_normal(truth.shape)
    per = rows // events
    index = pd.MultiIndex.from_tuples([(f"e{min(t // per, events - 1)}", t) for t in range(rows)])
    truth_df = pd.DataFrame(truth, index=index, copy=False)
    pipe = DevicePipeline(gpr, proj)
    wall = []
    for i in range(repeats + 1):
        t0 = time.perf_counter()
        out = pipe.diagnostics(x_test, truth_df, lf, n_points=2048, wet_threshold_depth=0.1)
        if i:
            wall.append(time.perf_counter() - t0)
    # the route without it: the predicted field to the host, then the reference's numpy
    t0 = time.perf_counter()
    buf, ns = pipe.predict_mean_field_dev(x_test)
    pred = buf.to_array((ns, cells))
    buf.free()
    t1 = time.perf_counter()
    s_up = np.sort(np.abs(pred - truth).flatten())
    s_lf = np.sort(np.abs(lf - truth).flatten())
    t2 = time.perf_counter()
    ranks = out["ranks"]
    return {
        "rows": rows, "cells": cells, "events": events, "n_points": 2048, "diagnostics_wall_s_median": median(wall), "diagnostics_wall_s_all": wall,
        "includes": "predict, upload of truth and LF (2 x 8 rows cells bytes over the host link), 2 sorts, 4 scatter summaries, depth conversion, detection",
        "host_route": {"predict_and_to_host_s": t1 - t0, "two_numpy_sorts_s": t2 - t1},
        "cdf_equal_to_host_route": bool(np.array_equal(out["cdf_upskill"], s_up[ranks]) and np.array_equal(out["cdf_lf"], s_lf[ranks])),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/diag_sort.json")
    ap.add_argument("--sizes", default="1000000,10000000,100000000")
    ap.add_argument("--rows", type=int, default=1400)
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from gpras_amd import _lib
    from gpras_amd.diagnostics import DG_TILE, FieldDiagnostics

    lib = _lib.load()
    fd = FieldDiagnostics()
    threads = os.environ.get("OMP_NUM_THREADS", "unset")
    rec = {"tile": DG_TILE, "copy_rate_Bps": COPY_RATE, "host": {"OMP_NUM_THREADS": threads, "note": "np.sort and the elementwise numpy operations run on one thread"},
           "sort": [], "pipeline": None}

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)

    for n in [int(v) for v in args.sizes.split(",") if v]:
        rec["sort"].append(sort_record(fd, lib, n, args.repeats))
        print(json.dumps({k: v for k, v in rec["sort"][-1].items() if not k.endswith("_all") and k != "host_route"}), flush=True)
        flush()
    fd.close()
    if args.rows > 0:
        rec["pipeline"] = pipeline_record(args.rows, args.cells, 3)
        print(json.dumps(rec["pipeline"]), flush=True)
        flush()


if __name__ == "__main__":
    main()
