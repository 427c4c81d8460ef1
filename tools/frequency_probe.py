"""Depth-frequency maps at the production shape of the ensemble probes: the accumulate of ``gpras_amd.frequency`` inside
``PeakEnsemble.evaluate`` and against what the parent commit offers for the same ``rate``.

    python tools/frequency_probe.py [--events 35] [--event-rows 86] [--cells 100000] [--modes 50] [--members 256] [--levels 64] [--repeats 3]
                                    [--out profiles/frequency_maps.json]

A ``GPRAS`` of ``--modes`` sparse models (M = 50, a few Adam steps: the probe times the prediction side) feeds ``PeakEnsemble.evaluate`` with
``rng="device"``.  Measured, alternating in one run after a warm-up round:

* ``evaluate`` without and with ``frequency=`` (a fresh ``FrequencyMaps`` per call): the ``"frequency"`` stage of the timer (host clock around
  calls that end in a synchronisation), the summed device time of the accumulate kernel by HIP events, and the call's total; the warm-up
  round checks that every other field of the result keeps its bits;
* on one event's resident ``peak (S, cells)`` block: ``add_peaks`` against the same ``rate`` formed the parent's way -- ceil(L / 8) calls of
  ``member_stats`` (8 thresholds each, the counts downloaded) combined on the host by the three rounded operations --, compared bit for bit;
* ``depth_at`` for 1 and 16 targets (host clock: the call with its download).

The byte count of one accumulate is the peak read, ``8 S cells``, plus the update of the rate entries whose count is not zero, at most
``16 L cells``; both bounds are given with the rates they imply beside the copy rate measured on this part, 6.29 TB/s."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_COPY_BYTES_PER_S = 6.29e12
RESULT_FIELDS = ("exceed_counts", "peak_mean", "peak_std", "peak_quantiles", "wet_area")


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def parent_rate(ens, peak, members, levels, weight, rate):
    """``rate + weight * (count / S)`` from ceil(L / 8) calls of ``member_stats``: what the parent commit offers."""
    out = np.empty_like(rate)
    for l0 in range(0, levels.size, 8):
        n = ens.member_stats(peak, members, thresholds=levels[l0:l0 + 8])["exceed"]
        t = n.astype(np.float64) / np.float64(members)
        u = np.float64(weight) * t
        out[l0:l0 + 8] = rate[l0:l0 + 8] + u
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=35)
    ap.add_argument("--event-rows", type=int, default=86)
    ap.add_argument("--cells", type=int, default=100_000)
    ap.add_argument("--modes", type=int, default=50)
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--levels", type=int, default=64)
    ap.add_argument("--train-rows", type=int, default=1000)
    ap.add_argument("--features", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from gpras_amd.ensemble import PeakEnsemble
    from gpras_amd.frequency import FrequencyMaps
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
                        hydraulic_parameter="wse")
    x, y, xs = make_regression(args.train_rows, args.features, n_outputs=k, n_test=rows, config=7)
    gpr = GPRAS("Matern32")
    gpr.fit(x, y, 50, "kmeans", "adam", max_iter=3)
    ranges = [(i * args.event_rows, (i + 1) * args.event_rows) for i in range(args.events)]
    ens = PeakEnsemble(gpr, proj)
    levels = np.linspace(0.0, 2.5, args.levels)
    weights = (0.5 / (1.0 + np.arange(args.events))).tolist()
    kw = dict(thresholds=(0.5, 1.0), quantiles=(0.05, 0.5, 0.95), seed=1, rng="device")

    # ---- evaluate without and with the frequency maps ------------------------------------------------------------------------------------
    stages = {"plain": [], "frequency": []}
    keeps_bits = rate_first = None
    for rep in range(args.repeats + 1):
        for name in ("plain", "frequency") if rep % 2 == 0 else ("frequency", "plain"):
            if name == "plain":
                res = ens.evaluate(xs, ranges, members, **kw)
            else:
                with FrequencyMaps(proj, levels) as fm:
                    res = ens.evaluate(xs, ranges, members, **kw, frequency=fm, weights=weights)
                    if rep == 0:
                        rate_first = fm.rate()
            if rep == 0:
                if name == "plain":
                    keep = res
                else:
                    keeps_bits = bool(all(np.array_equal(getattr(keep, n), getattr(res, n)) for n in RESULT_FIELDS))
            else:
                stages[name].append(res.last_timings_ms)
    monotone = bool(np.all(np.diff(rate_first, axis=0) <= 0.0))
    share_nonzero = float(np.count_nonzero(rate_first) / rate_first.size)
    del keep, res

    # ---- one event's resident peak block: add_peaks against the parent's way ----------------------------------------------------------------
    lo, hi = ranges[0]
    mean_dev, lc_dev, _ = ens.joint_dev(xs[lo:hi])
    zn = ens.normals_dev(0, members, hi - lo, 1, 0)
    scores = ens.scores_dev(mean_dev, lc_dev, zn, members, hi - lo)
    peak = ens.member_peaks_dev(scores, members, hi - lo)
    for buf in (mean_dev, lc_dev, zn, scores):
        buf.free()
    kernel, call, parent, invert = [], [], [], {1: [], 16: []}
    same = None
    with FrequencyMaps(proj, levels) as fm:
        host_rate = np.zeros((levels.size, cells))
        for rep in range(args.repeats + 1):
            for side in ("device", "parent") if rep % 2 == 0 else ("parent", "device"):
                t0 = time.perf_counter()
                if side == "device":
                    fm.add_peaks(peak, members, weights[0])
                    ms = (time.perf_counter() - t0) * 1e3
                    if rep:
                        call.append(ms)
                        kernel.append(fm.last_device_ms)
                else:
                    host_rate = parent_rate(ens, peak, members, levels, weights[0], host_rate)
                    if rep:
                        parent.append((time.perf_counter() - t0) * 1e3)
        same = bool(np.array_equal(fm.rate().view(np.uint64), host_rate.view(np.uint64)))
        positive = host_rate[host_rate > 0.0]
        targets = np.quantile(positive, np.linspace(0.05, 0.95, 16))
        for rep in range(args.repeats + 1):
            for n in (1, 16):
                t0 = time.perf_counter()
                fm.depth_at(targets[:n])
                if rep:
                    invert[n].append((time.perf_counter() - t0) * 1e3)
    peak.free()

    def med(name, key):
        return statistics.median(t[key] for t in stages[name])

    events = args.events
    peak_bytes, rate_bytes_most = 8.0 * members * cells, 16.0 * levels.size * cells
    kernel_s = statistics.median(kernel) * 1e-3
    out = {
        "shape": {"events": events, "event_rows": args.event_rows, "rows": rows, "cells": cells, "modes": k, "members": members, "levels": int(levels.size),
                  "train_rows": args.train_rows, "inducing": 50},
        "repeats": args.repeats, "result_fields_keep_their_bits": keeps_bits, "rate_non_increasing": monotone, "share_of_rate_entries_nonzero": share_nonzero,
        "evaluate_stage_ms_median": {name: {key: med(name, key) for key in stages[name][0] if key != "host_link_bytes"} for name in stages},
        "evaluate_total_ms": {name: spread([t["total"] for t in stages[name]]) for name in stages},
        "frequency_stage_ms": spread([t["frequency"] for t in stages["frequency"]]),
        "device_frequency_ms_per_call": spread([t["device_frequency"] for t in stages["frequency"]]),
        "device_accumulate_ms_per_event_in_evaluate": statistics.median(t["device_frequency"] for t in stages["frequency"]) / events,
        "one_event": {
            "device_accumulate_kernel_ms": spread(kernel), "add_peaks_call_ms": spread(call),
            "parent_member_stats_calls": -(-int(levels.size) // 8), "parent_way_ms": spread(parent), "parent_way_agrees_bit_for_bit": same,
            "speedup_parent_way_over_add_peaks_call": statistics.median(parent) / statistics.median(call),
            "bytes_peak_read": peak_bytes, "bytes_rate_update_at_most": rate_bytes_most,
            "achieved_bytes_per_s_peak_read_alone": peak_bytes / kernel_s, "achieved_bytes_per_s_at_most": (peak_bytes + rate_bytes_most) / kernel_s,
            "hbm_copy_bytes_per_s": HBM_COPY_BYTES_PER_S, "share_of_copy_rate_at_most": (peak_bytes + rate_bytes_most) / kernel_s / HBM_COPY_BYTES_PER_S,
        },
        "parent_way_ms_per_call_extrapolated": statistics.median(parent) * events,
        "depth_at_call_ms": {str(n): spread(v) for n, v in invert.items()},
    }
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    proj.close()


if __name__ == "__main__":
    main()
