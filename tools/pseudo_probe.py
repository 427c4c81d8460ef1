"""The pseudo-surface low-fidelity model at production size, one JSON record per measurement:

* surface: the surface kernel alone at (T, n_cells) with a fluvial operand -- HIP-event time (median of the runs after warm-up),
  bytes moved (16 B per element plus the once-read idx and elev) and the rate as a share of 6.3 TB/s;
* features: ``PseudoSurface.lf_features`` host to host (flows -> (T, k)) with its split, against the same result from the pieces
  that existed before it: ``GPRAS.predict`` -> ``EOFProjector.reverse_transform`` to the host -> numpy / scipy for the rating
  curves, the centerline, the gather and the two floors -> ``EOFProjector.transform``;
* fit: ``fit_centerline`` at (R, C) host to host and its kernel alone, against ``np.median`` on this host's CPUs.

    python tools/pseudo_probe.py [--surface 512x1000000] [--fit 100000x1000] [--k 20] [--runs 20] [--out profiles/pseudo_probe.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpras_amd import _lib  # noqa: E402
from gpras_amd._lib import DeviceBuffer, check  # noqa: E402
from gpras_amd.pseudo_surface import PseudoSurface, RatingCurve  # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def curve(rng, base, gain):
    q = 10.0 ** rng.uniform(1.1, 4.5, 4000)
    return RatingCurve(q, base + gain * np.log1p(q / 40.0) + 0.05 * rng.standard_normal(q.size))


def estimator(rng, cells, n_cl):
    elev = 108.0 + 16.0 * rng.random(cells)
    idx = np.sort(rng.integers(0, n_cl, cells))
    return PseudoSurface(elev, idx, curve(rng, 118.0, 2.1), curve(rng, 111.0, 1.7), np.sort(rng.random(n_cl)))


def timings(ps):
    ms = (C.c_double * 2)()
    check(_lib.load().gprx_ps_timings(ps.handle, ms))
    return ms[0], ms[1]


def probe_surface(T, cells, runs):
    rng = np.random.default_rng(0)
    lib = _lib.load()
    ps = estimator(rng, cells, 1000)
    us_q = 10.0 ** rng.uniform(1.2, 4.4, T)
    ps._rating(us_q, us_q * 1.1)
    fl = DeviceBuffer(8 * T * cells)
    out = DeviceBuffer(8 * T * cells)
    row = 104.0 + 24.0 * rng.random(cells)
    try:
        for t in range(T):  # some fluvial field: the kernel's time does not depend on the values
            check(lib.gprx_memcpy_h2d(0, fl.at(t * cells), _lib.ptr(row), row.nbytes))
        ms = []
        for i in range(runs + 3):
            check(lib.gprx_ps_surface_dev(ps.handle, 0, T, fl.ptr, cells, out.ptr, cells))
            if i >= 3:
                ms.append(timings(ps)[1])
        med = float(np.median(ms))
        nbytes = 16.0 * T * cells + 12.0 * cells + 16.0 * T
        return dict(what="surface", shape=[T, cells], runs=runs, kernel_ms_median=round(med, 4), kernel_ms_min=round(min(ms), 4),
                    kernel_ms_max=round(max(ms), 4), bytes=nbytes, tb_per_s=round(nbytes / med / 1e9, 3),
                    share_of_6p3_tb_per_s=round(nbytes / (med * 1e-3) / HBM_ACHIEVABLE, 3))
    finally:
        fl.free()
        out.free()
        ps.close()


def probe_features(T, cells, k, host):
    from scipy.interpolate import BSpline

    from gpras_amd.gpr import GPRAS
    from gpras_amd.preprocess import EOFProjector

    rng = np.random.default_rng(1)
    ps = estimator(rng, cells, 1000)
    n, d, kf = 512, 6, 10
    x = rng.normal(size=(n, d))
    y = np.stack([np.sin(x @ rng.normal(size=d)) + 0.05 * rng.normal(size=n) for _ in range(kf)], axis=1)
    gpr = GPRAS("Matern32")
    gpr.fit(x, y, 64, "kmeans", "adam", max_iter=5)

    def projector(modes, level, spread):
        dry = np.zeros(cells, dtype=bool)
        return EOFProjector(dry, ps.cell_elevations, level + rng.normal(size=cells), rng.uniform(0.5, 1.5, size=cells),
                            spread * rng.normal(size=(modes, cells)) / np.sqrt(modes), rng.normal(size=modes), rng.uniform(0.5, 2, size=modes), "wse")

    fluvial_proj, hf_proj = projector(kf, 116.0, 6.0), projector(k, 115.0, 1.0)
    fx = rng.normal(size=(T, d))
    us_q = 10.0 ** rng.uniform(1.2, 4.4, T)
    ds_q = us_q * rng.uniform(0.8, 1.3, T)
    ps.lf_features(us_q[:64], ds_q[:64], hf_proj, fluvial_x=fx[:64], fluvial_gpr=gpr, fluvial_projector=fluvial_proj)  # warm-up
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        z = ps.lf_features(us_q, ds_q, hf_proj, fluvial_x=fx, fluvial_gpr=gpr, fluvial_projector=fluvial_proj)
        ms = (time.perf_counter() - t0) * 1e3
        if best is None or ms < best[0]:
            best = (ms, dict(ps.last_timings_ms))
    rec = dict(what="features", shape=[T, cells], k=k, fluvial_modes=kf, device_host_to_host_ms=round(best[0], 2),
               device_split_ms={a: round(b, 3) for a, b in best[1].items() if a != "host_link_bytes"},
               device_host_link_bytes=int(best[1]["host_link_bytes"]), field_bytes=8 * T * cells)
    if host:
        h = {}
        t0 = t_all = time.perf_counter()

        def lap(key):
            nonlocal t0
            now = time.perf_counter()
            h[key] = round((now - t0) * 1e3, 2)
            t0 = now

        mean, _ = gpr.predict(fx)
        lap("predict_ms")
        fluvial = fluvial_proj.reverse_transform(mean)
        lap("reverse_to_host_ms")
        us = BSpline(ps.us_rating_curve.knots, ps.us_rating_curve.coefficients, 3, extrapolate=True)(us_q[:, None])
        ds = BSpline(ps.ds_rating_curve.knots, ps.ds_rating_curve.coefficients, 3, extrapolate=True)(ds_q[:, None])
        cl = us - np.outer(us - ds, ps.cl_interpolater)
        full = cl[:, ps.cell_interpolater]
        full = np.maximum(full, ps.cell_elevations[None, :])
        full = np.maximum(full, fluvial)
        lap("numpy_steps_1_to_4_ms")
        zh = hf_proj.transform(full)
        lap("transform_from_host_ms")
        h["total_ms"] = round((time.perf_counter() - t_all) * 1e3, 2)
        h["cpus"] = os.environ.get("OMP_NUM_THREADS")
        h["max_abs_difference_of_features"] = float(np.max(np.abs(zh - z)))
        rec["host_chain"] = h
        rec["speedup"] = round(h["total_ms"] / best[0], 2)
    ps.close()
    return rec


def probe_fit(R, n_cl, host):
    rng = np.random.default_rng(2)
    ps = PseudoSurface(np.zeros(4), np.zeros(4, dtype=np.int64), None, None, n_centerline=n_cl)
    us = 120.0 + 6.0 * rng.random(R)
    ds = us - (1.0 + 4.0 * rng.random(R))
    wse = us[:, None] - (us - ds)[:, None] * (np.sort(rng.random(n_cl))[None, :] + 0.08 * rng.standard_normal((R, n_cl)))
    us_q = np.where(rng.random(R) < 0.1, 0.0, 100.0)
    ds_q = np.where(rng.random(R) < 0.5, 0.0, 100.0)
    ps.fit_centerline(us[:1000], ds[:1000], us_q[:1000], ds_q[:1000], wse[:1000])  # warm-up
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        w = ps.fit_centerline(us, ds, us_q, ds_q, wse)
        runs.append(((time.perf_counter() - t0) * 1e3, timings(ps)[0]))
    best = min(runs)
    rec = dict(what="fit_centerline", shape=[R, n_cl], kept_rows=int(((us_q > 0) | (ds_q > 0)).sum()), device_host_to_host_ms=round(best[0], 2),
               kernel_ms=round(best[1], 3), block_bytes=wse.nbytes, kernel_passes_tb_per_s=round(9 * wse.nbytes / best[1] / 1e9, 3))
    if host:
        t0 = time.perf_counter()
        keep = (us_q > 0) | (ds_q > 0)
        want = np.median((us[keep, None] - wse[keep]) / (us[keep] - ds[keep])[:, None], axis=0)
        rec["numpy_median_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        rec["cpus"] = os.environ.get("OMP_NUM_THREADS")
        rec["equal_to_numpy"] = bool(np.array_equal(w, want, equal_nan=True))
        rec["speedup"] = round(rec["numpy_median_ms"] / best[0], 2)
    ps.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--surface", default="512x1000000")
    ap.add_argument("--fit", default="100000x1000")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--only", default="surface,features,fit")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    T, cells = (int(v) for v in args.surface.split("x"))
    R, n_cl = (int(v) for v in args.fit.split("x"))
    rows = []
    for what in args.only.split(","):
        rec = {"surface": lambda: probe_surface(T, cells, args.runs), "features": lambda: probe_features(T, cells, args.k, not args.no_host),
               "fit": lambda: probe_fit(R, n_cl, not args.no_host)}[what]()
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        if args.out:  # after every record: a later one that fails keeps the earlier ones
            with open(args.out, "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
