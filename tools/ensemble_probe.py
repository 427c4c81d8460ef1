"""Peak ensemble at a production shape: the fused peak kernel against ``route="refield"`` (reverse -> depth -> per-member row maximum on
the existing kernels), alternating, by the stage timer of ``PeakEnsemble.evaluate`` (host milliseconds around work that ends in a
synchronisation) and the device time of the fused launches.

    python tools/ensemble_probe.py [--events 35] [--event-rows 86] [--cells 100000] [--modes 50] [--members 256] [--repeats 3]
                                   [--rng host|device|both] [--verify] [--timing] [--out profiles/ensemble_peaks.json]

A ``GPRAS`` of ``--modes`` sparse models (M = 50, a few Adam steps: the probe times the prediction side) feeds ``PeakEnsemble.evaluate``.
The first round warms both routes up and compares them (every output bit for bit), so that a faster number is a number for the same
answer.  The FMA rate counts the fused multiply-adds the result needs -- members x rows x cells x modes -- over the device time of the
fused kernel, against the 78.6 TFLOP/s (39.3 T fma/s) AMD quotes for fp64 vector work on this part; the draw + upload share is the host
time of generating the normals and sending them up over the whole call.

``--rng host`` (the default) and ``--rng device`` run that comparison of the routes with the one generator.  ``--rng both`` compares the
generators instead (profiles/ensemble_rng.json): ``rng="host"`` -- ``np.random.default_rng`` and the upload, the route every earlier release
took and the yardstick -- against ``rng="device"`` (``gprx_pca_normals_dev``), alternating in one run on the default route, by the same stage
timer; ``draw_upload`` is the stage the generator is timed in.

``--verify`` (profiles/ensemble_verify.json) measures the verification against the truth instead: the ``"verify"`` stage of
``evaluate(observed=...)`` with ``"stats"`` beside it, the device time of ``gprx_pca_member_verify_dev`` by HIP events, and the same scores formed
on the host from a downloaded ``peak`` block (download, ``np.sort``, vectorised weights: the yardstick), alternating in one run.

``--timing`` (profiles/ensemble_timing.json) measures the event timing instead -- arrival, duration and time of the peak at three thresholds:
``evaluate`` with the peaks kernel alone (``timing=False``, what the parent commit ran), with the timing kernel in its place (``timing=True``) and with
``route="refield"`` for the same maps, alternating in one run after a warm-up round that compares the two routes bit for bit; the device times of
the two fused kernels, the ``"peaks"``, ``"stats"`` and ``"timing"`` stages, and the same maps with numpy from downloaded fields of one event
at ``--host-members`` members (the yardstick: what a caller without the kernel would do)."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_VECTOR_PEAK_FMA = 39.3e12


def compare_generators(args, run, shape, draw_ms) -> None:
    """``rng="host"`` against ``rng="device"`` on the default route, alternating; the first round warms both up."""
    from gpras_amd.ensemble import DEFAULT_RNG, DEFAULT_ROUTE

    stages = {"host": [], "device": []}
    finite = True
    for rep in range(args.repeats + 1):
        for rng in ("host", "device") if rep % 2 == 0 else ("device", "host"):
            res = run(DEFAULT_ROUTE, rng)
            if rep == 0:
                finite = finite and bool(np.all(np.isfinite(res.peak_mean)) and np.all(np.isfinite(res.peak_std)))
            else:
                stages[rng].append(res.last_timings_ms)

    def med(rng, key):
        return statistics.median(t[key] for t in stages[rng])

    keys = ("joint", "draw_upload", "draws", "peaks", "stats", "total")
    out = {
        "shape": shape, "route": DEFAULT_ROUTE, "repeats": args.repeats, "outputs_finite": finite, "default_rng": DEFAULT_RNG,
        "stage_ms_median": {rng: {key: med(rng, key) for key in keys} for rng in stages},
        "total_ms": {rng: {"median": med(rng, "total"), "min": min(t["total"] for t in stages[rng]), "max": max(t["total"] for t in stages[rng])}
                     for rng in stages},
        "draw_upload_ms": {rng: {"median": med(rng, "draw_upload"), "min": min(t["draw_upload"] for t in stages[rng]),
                                 "max": max(t["draw_upload"] for t in stages[rng])} for rng in stages},
        "host_link_bytes": {rng: stages[rng][0]["host_link_bytes"] for rng in stages},
        "host_normals_ms": draw_ms,
        "normals_per_call": float(shape["modes"]) * shape["members"] * shape["rows"],
    }
    out["speedup_host_over_device_draw_upload"] = med("host", "draw_upload") / med("device", "draw_upload")
    out["speedup_host_over_device_total"] = med("host", "total") / med("device", "total")
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def host_scores(peak_dev, obs, members, cells):
    """The yardstick of ``--verify``: the scores of ``gprx_pca_member_verify_dev`` formed on the host from a downloaded ``peak`` -- the
    download, ``np.sort`` over the members and the weights vectorised over ``(S, cells)``.  Returns the scores and the three times in ms."""
    t0 = time.perf_counter()
    peak = peak_dev.to_array((members, cells))
    t1 = time.perf_counter()
    xs = np.sort(peak, axis=0)
    t2 = time.perf_counter()
    i = np.arange(members, dtype=np.float64)[:, None]
    gt = xs > obs[None, :]
    acc = (np.abs(xs - obs[None, :]) * np.where(gt, (members - i) - 0.5, i + 0.5)).sum(axis=0)
    crps = (2.0 * acc) / (float(members) * float(members))
    below, equal = (xs < obs[None, :]).sum(axis=0), (xs == obs[None, :]).sum(axis=0)
    t3 = time.perf_counter()
    return (crps, below, equal), {"download": (t1 - t0) * 1e3, "sort": (t2 - t1) * 1e3, "weights": (t3 - t2) * 1e3, "total": (t3 - t0) * 1e3}


def measure_verification(args, ens, xs, ranges, shape) -> None:
    """``--verify``: ``evaluate(observed=...)`` by its stage timer (the ``"verify"`` stage, ``"stats"`` for context), the device time of the
    verification kernel by HIP events, and per event the call ``verify_peaks`` against the host yardstick (``host_scores``) on the same
    resident peak block, alternating; the first round warms both up and compares their answers."""
    from gpras_amd._lib import DeviceBuffer
    from gpras_amd.ensemble import DEFAULT_ROUTE

    members, cells, rows = shape["members"], shape["cells"], shape["rows"]
    rng = np.random.default_rng(2)
    truth = DeviceBuffer.from_array(np.maximum(rng.normal(size=(rows, cells)) * 0.5 + 0.6, 0.0), ens.device)
    lo, hi = ranges[0]
    mean_dev, lc_dev, _ = ens.joint_dev(xs[lo:hi])
    scores = ens.scores_dev(mean_dev, lc_dev, np.random.default_rng(3).standard_normal((shape["modes"], members, hi - lo)), members, hi - lo)
    peak = ens.member_peaks_dev(scores, members, hi - lo)
    obs_dev = ens.observed_peak_dev(truth, lo, hi)
    obs = obs_dev.to_array((cells,))
    for buf in (mean_dev, lc_dev, scores):
        buf.free()
    calls, host, kernel, stages = [], [], [], []
    agree = None
    for rep in range(args.repeats + 1):
        for side in ("device", "host") if rep % 2 == 0 else ("host", "device"):
            if side == "device":
                t0 = time.perf_counter()
                got = ens.verify_peaks(peak, obs_dev, members)
                call_ms = (time.perf_counter() - t0) * 1e3
                res = ens.evaluate(xs, ranges, members, thresholds=(0.5, 1.0), quantiles=(0.05, 0.5, 0.95), seed=1, route=DEFAULT_ROUTE, rng=args.rng,
                                   observed=truth)
                if rep:
                    calls.append(call_ms)
                    kernel.append(ens.last_device_verify_ms)
                    stages.append(res.last_timings_ms)
            else:
                (crps, below, equal), ms = host_scores(peak, obs, members, cells)
                if rep:
                    host.append(ms)
                else:
                    want = (crps, below, equal)
        if rep == 0:
            agree = bool(np.array_equal(got["below"], want[1]) and np.array_equal(got["equal"], want[2])
                         and np.allclose(got["crps"], want[0], rtol=1e-12, atol=0))
    for buf in (peak, obs_dev, truth):
        buf.free()

    def med(rows_, key):
        return statistics.median(t[key] for t in rows_)

    events = shape["events"]
    out = {
        "shape": shape, "route": DEFAULT_ROUTE, "rng": args.rng, "repeats": args.repeats, "host_agrees": agree,
        "evaluate_stage_ms_median": {key: med(stages, key) for key in ("joint", "draw_upload", "draws", "peaks", "stats", "verify", "total")},
        "evaluate_device_verify_ms_median": med(stages, "device_verify"),
        "per_event": {
            "device_kernel_ms": {"median": statistics.median(kernel), "min": min(kernel), "max": max(kernel)},
            "verify_peaks_call_ms": {"median": statistics.median(calls), "min": min(calls), "max": max(calls)},
            "host_yardstick_ms": {key: {"median": med(host, key), "min": min(t[key] for t in host), "max": max(t[key] for t in host)}
                                  for key in ("download", "sort", "weights", "total")},
            "peak_bytes_downloaded_by_the_yardstick": 8 * members * cells,
        },
    }
    out["host_yardstick_ms_per_call"] = med(host, "total") * events
    out["speedup_host_yardstick_over_verify_peaks_call"] = med(host, "total") / statistics.median(calls)
    out["speedup_host_yardstick_over_verify_stage"] = out["host_yardstick_ms_per_call"] / med(stages, "verify")
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


TIMING_FIELDS = ("t_peak_sum", "t_peak_quantiles", "duration_sum", "duration_quantiles", "duration_below_counts", "arrival_counts", "arrival_sum",
                 "arrival_quantiles", "arrival_by_counts")
RESULT_FIELDS = ("exceed_counts", "peak_mean", "peak_std", "peak_quantiles", "wet_area")


def host_timing(ens, scores, members, rows, thr):
    """The yardstick of ``--timing``: the members' fields of one event formed on the device (reverse -> depth), downloaded, and reduced with
    numpy to the maps of ``member_timing_dev``.  Returns the maps and the times in ms."""
    from gpras_amd._lib import DeviceBuffer, check

    pr, lib = ens.projector, ens._lib
    cells, k = pr.n_cells, pr.spatial_mode_count
    field = DeviceBuffer(8 * members * rows * cells, ens.device)
    try:
        t0 = time.perf_counter()
        check(lib.gprx_pca_reverse_dev(pr.handle, scores.ptr, None, members * rows, field.ptr, None))
        if pr.hydraulic_parameter != "velocity":
            check(lib.gprx_pca_to_depth_dev(pr.handle, field.ptr, members * rows, int(pr.hydraulic_parameter == "depth")))
        check(lib.gprx_pca_synchronize(pr.handle))
        t1 = time.perf_counter()
        y = field.to_array((members, rows, cells))
        t2 = time.perf_counter()
    finally:
        field.free()
    maps = [np.argmax(y, axis=1)]
    above = [y > t for t in thr]
    maps += [a.sum(axis=1) for a in above]
    maps += [np.where(a.any(axis=1), np.argmax(a, axis=1), rows) for a in above]
    out = np.stack(maps, axis=1).astype(np.int32)
    t3 = time.perf_counter()
    return out, {"fields_on_device": (t1 - t0) * 1e3, "download": (t2 - t1) * 1e3, "numpy": (t3 - t2) * 1e3, "total": (t3 - t0) * 1e3}


def measure_timing(args, ens, xs, ranges, shape) -> None:
    """``--timing``: see the module's docstring."""
    members, k = shape["members"], shape["modes"]
    thr, durations, arrive_by = (0.25, 0.5, 1.0), (1, 6, 24), (6, 24, 48)
    kw = dict(thresholds=thr, quantiles=(0.05, 0.5, 0.95), seed=1, rng=args.rng)
    variants = {"peaks_only": dict(route="fused"), "timing_fused": dict(route="fused", timing=True, durations=durations, arrive_by=arrive_by),
                "timing_refield": dict(route="refield", timing=True, durations=durations, arrive_by=arrive_by)}
    order = list(variants)
    stages = {name: [] for name in variants}
    agree = {}
    for rep in range(args.repeats + 1):
        keep = {}
        for name in order if rep % 2 == 0 else order[::-1]:
            res = ens.evaluate(xs, ranges, members, **kw, **variants[name])
            if rep == 0:
                keep[name] = res
            else:
                stages[name].append(res.last_timings_ms)
        if rep == 0:
            a, b, c = keep["timing_fused"], keep["timing_refield"], keep["peaks_only"]
            agree["routes_agree_bit_for_bit"] = bool(all(np.array_equal(getattr(a.timing, n), getattr(b.timing, n)) for n in TIMING_FIELDS)
                                                     and all(np.array_equal(getattr(a, n), getattr(b, n)) for n in RESULT_FIELDS))
            agree["peaks_fields_keep_their_bits"] = bool(all(np.array_equal(getattr(a, n), getattr(c, n)) for n in RESULT_FIELDS))
            agree["arrival_counts_equal_exceed_counts"] = bool(np.array_equal(a.timing.arrival_counts, a.exceed_counts))
            agree["share_of_member_cells_never_arriving"] = [float(1.0 - a.timing.p_arrival[:, j].mean()) for j in range(len(thr))]
            del keep, a, b, c
    # the yardstick on one event at a member count whose fields fit the host
    hm = max(1, min(args.host_members, members))
    lo, hi = ranges[0]
    rows = hi - lo
    mean_dev, lc_dev, _ = ens.joint_dev(xs[lo:hi])
    scores = ens.scores_dev(mean_dev, lc_dev, np.random.default_rng(3).standard_normal((k, hm, rows)), hm, rows)
    host, host_same = [], None
    for rep in range(args.repeats + 1):
        maps, ms = host_timing(ens, scores, hm, rows, thr)
        if rep == 0:
            peak_dev, timing_dev = ens.member_timing_dev(scores, hm, rows, thr)
            host_same = bool(np.array_equal(ens.timing_to_array(timing_dev, hm, 1 + 2 * len(thr)), maps))
            peak_dev.free()
            timing_dev.free()
        else:
            host.append(ms)
    for buf in (mean_dev, lc_dev, scores):
        buf.free()

    def med(name, key):
        return statistics.median(t[key] for t in stages[name])

    def spread(name, key):
        return {"median": med(name, key), "min": min(t[key] for t in stages[name]), "max": max(t[key] for t in stages[name])}

    events = shape["events"]
    out = {
        "shape": shape, "rng": args.rng, "repeats": args.repeats, "thresholds": thr, "durations": durations, "arrive_by": arrive_by, **agree,
        "stage_ms_median": {name: {key: med(name, key) for key in stages[name][0] if key != "host_link_bytes"} for name in stages},
        "device_walk_ms": {name: spread(name, "device_peaks") for name in ("peaks_only", "timing_fused")},
        "peaks_stage_ms": {name: spread(name, "peaks") for name in stages},
        "timing_stage_ms": {name: spread(name, "timing") for name in ("timing_fused", "timing_refield")},
        "total_ms": {name: spread(name, "total") for name in stages},
        "host_yardstick": {
            "members": hm, "events": 1, "maps_agree_bit_for_bit": host_same, "field_bytes_downloaded": 8 * hm * rows * shape["cells"],
            "ms": {key: {"median": statistics.median(t[key] for t in host), "min": min(t[key] for t in host), "max": max(t[key] for t in host)}
                   for key in ("fields_on_device", "download", "numpy", "total")},
        },
    }
    out["timing_kernel_over_peaks_kernel"] = med("timing_fused", "device_peaks") / med("peaks_only", "device_peaks")
    out["refield_over_fused_peaks_stage_with_timing"] = med("timing_refield", "peaks") / med("timing_fused", "peaks")
    out["timing_call_over_peaks_call_total"] = med("timing_fused", "total") / med("peaks_only", "total")
    per_member_event = out["host_yardstick"]["ms"]["total"]["median"] / hm
    out["host_yardstick"]["ms_per_member_event"] = per_member_event
    out["host_yardstick"]["extrapolated_ms_per_call"] = per_member_event * members * events  # (linear in members x events: every field is touched once)
    out["device_walk_ms_per_member_event"] = med("timing_fused", "device_peaks") / (members * events)
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=35)
    ap.add_argument("--event-rows", type=int, default=86)
    ap.add_argument("--cells", type=int, default=100_000)
    ap.add_argument("--modes", type=int, default=50)
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--train-rows", type=int, default=1000)
    ap.add_argument("--features", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hydraulic-parameter", default="wse")
    ap.add_argument("--rng", choices=("host", "device", "both"), default="host")
    ap.add_argument("--verify", action="store_true", help="measure the verification against the truth (profiles/ensemble_verify.json)")
    ap.add_argument("--timing", action="store_true", help="measure the event timing (profiles/ensemble_timing.json)")
    ap.add_argument("--host-members", type=int, default=8, help="--timing: members whose fields the numpy yardstick downloads")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.timing and (args.verify or args.rng == "both"):
        ap.error("--timing is a mode of its own: not with --verify or --rng both")
    if args.verify and args.rng == "both":
        ap.error("--verify takes one generator: --rng host or --rng device")

    from gpras_amd.ensemble import PeakEnsemble
    from gpras_amd.gpr import GPRAS
    from gpras_amd.preprocess import EOFProjector
    from gpras_amd.synth import make_regression

    rng = np.random.default_rng(0)
    cells, k, rows, members = args.cells, args.modes, args.events * args.event_rows, args.members
    dry = np.zeros(cells, dtype=bool)
    dry[rng.choice(cells, size=cells // 50, replace=False)] = True
    n_wet = int(cells - dry.sum())
    elev = rng.uniform(0.0, 2.0, size=cells)
    proj = EOFProjector(dry, elev, rng.uniform(0.2, 1.0, size=n_wet) + elev[~dry], rng.uniform(0.5, 1.5, size=n_wet),
                        rng.standard_normal((k, n_wet)) / np.sqrt(n_wet), rng.standard_normal(k) * 0.1, rng.uniform(0.5, 2.0, size=k) * np.sqrt(n_wet) * 0.05,
                        hydraulic_parameter=args.hydraulic_parameter)
    x, y, xs = make_regression(args.train_rows, args.features, n_outputs=k, n_test=rows, config=7)
    gpr = GPRAS("Matern32")
    gpr.fit(x, y, 50, "kmeans", "adam", max_iter=3)
    ranges = [(i * args.event_rows, (i + 1) * args.event_rows) for i in range(args.events)]
    ens = PeakEnsemble(gpr, proj)
    # the generator's share alone: the normals of one call, drawn as evaluate draws them
    t0 = time.perf_counter()
    g = np.random.default_rng(1)
    for _ in ranges:
        g.standard_normal((k, members, args.event_rows))
    draw_ms = (time.perf_counter() - t0) * 1e3

    def run(route, rng=args.rng):
        return ens.evaluate(xs, ranges, members, thresholds=(0.5, 1.0), quantiles=(0.05, 0.5, 0.95), seed=1, route=route, rng=rng)

    shape = {"events": args.events, "event_rows": args.event_rows, "rows": rows, "cells": cells, "modes": k, "members": members,
             "train_rows": args.train_rows, "inducing": 50, "hydraulic_parameter": args.hydraulic_parameter}
    if args.rng == "both":
        compare_generators(args, run, shape, draw_ms)
        proj.close()
        return
    if args.verify:
        measure_verification(args, ens, xs, ranges, shape)
        proj.close()
        return
    if args.timing:
        measure_timing(args, ens, xs, ranges, shape)
        proj.close()
        return

    stages = {"fused": [], "refield": []}
    same = None
    for rep in range(args.repeats + 1):
        for route in ("fused", "refield") if rep % 2 == 0 else ("refield", "fused"):
            res = run(route)
            if rep == 0:
                if route == "fused":
                    keep = res
                else:
                    same = all(np.array_equal(getattr(keep, n), getattr(res, n)) for n in ("exceed_counts", "peak_mean", "peak_std", "peak_quantiles", "wet_area"))
            else:
                stages[route].append(res.last_timings_ms)

    def med(route, key):
        return statistics.median(t[key] for t in stages[route])

    fmas = float(members) * rows * cells * k
    keys = ("joint", "draw_upload", "draws", "peaks", "stats", "total")
    out = {
        "shape": shape, "rng": args.rng,
        "repeats": args.repeats, "routes_agree_bit_for_bit": bool(same),
        "stage_ms_median": {route: {key: med(route, key) for key in keys} for route in stages},
        "peaks_ms": {route: {"median": med(route, "peaks"), "min": min(t["peaks"] for t in stages[route]), "max": max(t["peaks"] for t in stages[route])}
                     for route in stages},
        "fused_device_peaks_ms_median": med("fused", "device_peaks"),
        "fma_count": fmas,
        "fp64_vector_peak_fma_per_s": FP64_VECTOR_PEAK_FMA,
        "host_normals_ms": draw_ms,
    }
    out["fused_fma_per_s"] = fmas / (out["fused_device_peaks_ms_median"] * 1e-3)
    out["fused_share_of_fp64_vector_peak"] = out["fused_fma_per_s"] / FP64_VECTOR_PEAK_FMA
    out["speedup_refield_over_fused_peaks_stage"] = out["peaks_ms"]["refield"]["median"] / out["peaks_ms"]["fused"]["median"]
    out["speedup_refield_over_fused_total"] = med("refield", "total") / med("fused", "total")
    out["draw_upload_share_of_total"] = {route: med(route, "draw_upload") / med(route, "total") for route in stages}
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    proj.close()


if __name__ == "__main__":
    main()
