"""LF-to-HF mesh resampling at production size, one JSON record per measurement:

* kernel: the nearest (gather + floor) and the linear kernel alone at (T, n_hf) from n_lf source cells -- HIP-event time (median of
  the runs after warm-up), bytes moved (8 B per output element, the source block once, the per-cell indices, weights and elevations
  once per row tile) and the rate as a share of 6.3 TB/s and of the 4.90 TB/s of ps_surface_kernel.  Index orders: "mesh" (HF cells
  and LF cells both numbered along strips, as a mesh generator numbers them) and "random" (no locality at all).  Source sizes beside
  the asked one show what the gathered reads cost: 1 000 cells (8 KB rows, served by the vector cache) against 16 384 (128 KB, what
  LDS could hold) and 50 000 (400 KB, L2 only);
* features: ``MeshResampler.lf_features`` host to host ((T, n_lf) -> (T, k)) with its split and the bytes that crossed the host
  link, against the host chain: the reference's loop (one ``LinearNDInterpolator`` per row, timed over ``--host-rows`` rows and scaled
  to T, the loop being linear in T) and ``EOFProjector.transform`` from the host.

    python tools/resample_probe.py [--shape 512x1000000] [--n-lf 50000] [--k 20] [--runs 20] [--out profiles/resample_probe.json]
"""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpras_amd import _lib  # noqa: E402
from gpras_amd._lib import DeviceBuffer, check  # noqa: E402
from gpras_amd.resample import MeshResampler  # noqa: E402

HBM_ACHIEVABLE, PS_SURFACE_RATE = 6.3e12, 4.90e12
ROW_TILE = {"nearest": 8, "linear": 32}  # RS_RT x rs_groups(NV) of csrc/resample.h: the rows for which a thread keeps its per-cell arrays


def strip_order(xy, strips):
    """Cells numbered along horizontal strips, left to right."""
    return np.lexsort((xy[:, 0], np.floor(xy[:, 1] * strips)))


def meshes(n_lf, n_hf, order, seed=0):
    rng = np.random.default_rng(seed)
    lf, hf = rng.random((n_lf, 2)), 0.02 + 0.96 * rng.random((n_hf, 2))
    if order == "mesh":
        lf, hf = lf[strip_order(lf, int(np.sqrt(n_lf)))], hf[strip_order(hf, int(np.sqrt(n_hf)))]
    return lf, hf, 100.0 + 5.0 * rng.random(n_hf)


def resampler(kind, lf, hf, elev):
    if kind == "linear":
        return MeshResampler.linear(lf, hf, elev)
    from scipy.spatial import cKDTree

    return MeshResampler.nearest(cKDTree(lf).query(hf)[1], len(lf), elev)  # the LF cell around each HF centroid


def probe_kernel(kind, order, T, n_hf, n_lf, runs):
    lib = _lib.load()
    lf, hf, elev = meshes(n_lf, n_hf, order)
    rs = resampler(kind, lf, hf, elev)
    rng = np.random.default_rng(1)
    src = DeviceBuffer.from_array(100.0 + 5.0 * rng.random((T, n_lf)))
    out = DeviceBuffer(8 * T * n_hf)
    ms = (C.c_double * 1)()
    try:
        times = []
        for i in range(runs + 3):
            check(lib.gprx_rs_apply_dev(rs.handle, T, src.ptr, n_lf, None, out.ptr, n_hf))
            check(lib.gprx_rs_timings(rs.handle, ms))
            if i >= 3:
                times.append(ms[0])
        med = float(np.median(times))
        per_cell = 12.0 if kind == "nearest" else 44.0  # idx + elev; 3 idx + 3 weights + elev
        nbytes = 8.0 * T * n_hf + 8.0 * T * n_lf + per_cell * n_hf * -(-T // ROW_TILE[kind])
        return dict(what="kernel", kind=kind, order=order, shape=[T, n_hf], n_lf=n_lf, runs=runs, kernel_ms_median=round(med, 4),
                    kernel_ms_min=round(min(times), 4), kernel_ms_max=round(max(times), 4), bytes=nbytes, tb_per_s=round(nbytes / med / 1e9, 3),
                    share_of_6p3_tb_per_s=round(nbytes / (med * 1e-3) / HBM_ACHIEVABLE, 3),
                    share_of_ps_surface_4p90_tb_per_s=round(nbytes / (med * 1e-3) / PS_SURFACE_RATE, 3))
    finally:
        src.free()
        out.free()
        rs.close()


def probe_features(T, n_hf, n_lf, k, host_rows):
    from scipy.interpolate import LinearNDInterpolator
    from scipy.spatial import Delaunay

    from gpras_amd.preprocess import EOFProjector

    lf, hf, elev = meshes(n_lf, n_hf, "mesh")
    rng = np.random.default_rng(2)
    t0 = time.perf_counter()
    rs = MeshResampler.linear(lf, hf, elev)
    prepare_ms = (time.perf_counter() - t0) * 1e3
    proj = EOFProjector(np.zeros(n_hf, dtype=bool), elev, 102.0 + rng.normal(size=n_hf), rng.uniform(0.5, 1.5, size=n_hf),
                        rng.normal(size=(k, n_hf)) / np.sqrt(k), rng.normal(size=k), rng.uniform(0.5, 2, size=k), "wse")
    z = 100.0 + 5.0 * rng.random((T, n_lf))
    rs.lf_features(z[:64], proj)  # warm-up
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        feat = rs.lf_features(z, proj)
        ms = (time.perf_counter() - t0) * 1e3
        if best is None or ms < best[0]:
            best = (ms, dict(rs.last_timings_ms))
    rec = dict(what="features", kind="linear", shape=[T, n_hf], n_lf=n_lf, k=k, locate_and_weights_once_ms=round(prepare_ms, 1),
               device_host_to_host_ms=round(best[0], 2), device_split_ms={a: round(b, 3) for a, b in best[1].items() if a != "host_link_bytes"},
               device_host_link_bytes=int(best[1]["host_link_bytes"]), field_bytes=8 * T * n_hf)
    if host_rows:
        n = min(host_rows, T)
        t0 = time.perf_counter()
        tri = Delaunay(lf)
        vals = np.empty((n, n_hf))
        t1 = time.perf_counter()
        for i in range(n):
            vals[i] = LinearNDInterpolator(tri, z[i])(hf)
        loop_ms = (time.perf_counter() - t1) * 1e3
        mask = (vals < elev) | np.isnan(vals)
        vals[mask] = np.broadcast_to(elev, vals.shape)[mask]
        field = rs.lf_plan_data(z)
        t2 = time.perf_counter()
        zh = proj.transform(field)
        transform_ms = (time.perf_counter() - t2) * 1e3
        h = dict(triangulation_ms=round((t1 - t0) * 1e3, 1), loop_rows_timed=n, loop_ms_per_row=round(loop_ms / n, 1),
                 loop_ms_scaled_to_T=round(loop_ms / n * T, 1), transform_from_host_ms=round(transform_ms, 2), cpus=os.environ.get("OMP_NUM_THREADS"),
                 rows_equal_to_the_device_field=bool(np.array_equal(vals, field[:n], equal_nan=True)),
                 features_equal=bool(np.array_equal(zh, feat, equal_nan=True)))
        h["total_ms"] = round(h["loop_ms_scaled_to_T"] + transform_ms, 1)
        rec["host_chain"] = h
        rec["speedup"] = round(h["total_ms"] / best[0], 1)
    rs.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="512x1000000")
    ap.add_argument("--n-lf", default="50000,16384,1000")
    ap.add_argument("--orders", default="mesh,random")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--host-rows", type=int, default=3)
    ap.add_argument("--only", default="kernel,features")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    T, n_hf = (int(v) for v in args.shape.split("x"))
    sizes = [int(v) for v in args.n_lf.split(",")]
    rows = []

    def keep(rec):
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        if args.out:  # after every record: a later one that fails keeps the earlier ones
            with open(args.out, "w") as f:
                json.dump(rows, f, indent=1)

    for what in args.only.split(","):
        if what == "kernel":
            for n_lf in sizes:
                for order in args.orders.split(",")[: None if n_lf == sizes[0] else 1]:  # the other orders at the asked size only
                    for kind in ("nearest", "linear"):
                        keep(probe_kernel(kind, order, T, n_hf, n_lf, args.runs))
        else:
            keep(probe_features(T, n_hf, sizes[0], args.k, args.host_rows))


if __name__ == "__main__":
    main()
