"""Mode-count sweep at a production shape: the fused pass against the per-count chain (``route="refield"``), alternating, with the
handle's stage timer (host milliseconds around work that ends in a synchronisation) and the device time of the fused launches.

    python tools/sweep_probe.py [--events 14] [--event-rows 215] [--cells 100000] [--modes 50] [--repeats 5] [--out profiles/sweep_probe.json]

The inputs live on the device before the timed window (``DevicePipeline.mode_count_sweep`` hands device buffers over the same way); what
is timed is ``ModeCountSweep.evaluate`` per route, stage ``evaluate``.  The two routes' results are compared on the way (per-cell tables of
the first and last count bit for bit), so that a faster number is a number for the same answer."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COUNTS = [1, 3, 5, 7, 10, 15, 20, 30, 50]  # run_spatial_modes (production/analysis/cross_validation.py:100)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=14)
    ap.add_argument("--event-rows", type=int, default=215)
    ap.add_argument("--cells", type=int, default=100_000)
    ap.add_argument("--modes", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hydraulic-parameter", default="wse")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from gpras_amd import _lib
    from gpras_amd._lib import DeviceBuffer
    from gpras_amd.preprocess import EOFProjector
    from gpras_amd.sweep import ModeCountSweep

    rng = np.random.default_rng(0)
    cells, k, rows = args.cells, args.modes, args.events * args.event_rows
    counts = [c for c in COUNTS if c <= k]
    dry = np.zeros(cells, dtype=bool)
    dry[rng.choice(cells, size=cells // 50, replace=False)] = True
    n_wet = int(cells - dry.sum())
    elev = rng.uniform(0.0, 2.0, size=cells)
    proj = EOFProjector(dry, elev, rng.uniform(0.2, 1.0, size=n_wet) + elev[~dry], rng.uniform(0.5, 1.5, size=n_wet),
                        rng.standard_normal((k, n_wet)) / np.sqrt(n_wet), rng.standard_normal(k) * 0.1, rng.uniform(0.5, 2.0, size=k) * np.sqrt(n_wet) * 0.05,
                        hydraulic_parameter=args.hydraulic_parameter)
    mean = rng.standard_normal((rows, k))
    var = rng.uniform(0.01, 0.3, size=(rows, k))
    truth = proj.reverse_transform(mean) + 0.2 * rng.standard_normal((rows, cells), dtype=np.float32)
    if args.hydraulic_parameter != "velocity":
        truth = np.maximum(truth - elev, 0.0)
    ranges = [(i * args.event_rows, (i + 1) * args.event_rows) for i in range(args.events)]
    d_mean, d_var, d_truth = DeviceBuffer.from_array(mean), DeviceBuffer.from_array(var), DeviceBuffer.from_array(truth)
    del truth
    sweep = ModeCountSweep(proj, counts)

    def run(route):
        return sweep.evaluate(d_mean, d_var, d_truth, ranges, v_tol=0.1, route=route, rows=rows)

    times = {"fused": [], "refield": [], "fused_device": []}
    same = None
    for rep in range(args.repeats + 1):  # the first round warms both routes up and compares them
        for route in ("fused", "refield") if rep % 2 == 0 else ("refield", "fused"):
            res = run(route)
            t = res.stage_timings_ms()
            if rep == 0:
                if route == "fused":
                    keep = res
                    continue
                same = all(np.array_equal(keep.cell_block(j, i)[0][[0, 1, 2, 4, 5]], res.cell_block(j, i)[0][[0, 1, 2, 4, 5]], equal_nan=True)
                           and np.array_equal(keep.cell_block(j, i)[1], res.cell_block(j, i)[1]) for j in (0, len(counts) - 1) for i in (0, args.events - 1))
                same = bool(same and np.array_equal(keep.matches, res.matches))
                keep.close()
            else:
                times[route].append(t["evaluate"])
                if route == "fused":
                    times["fused_device"].append(t["device_sweep"])
            res.close()
    out = {
        "shape": {"events": args.events, "event_rows": args.event_rows, "rows": rows, "cells": cells, "modes": k, "counts": counts,
                  "hydraulic_parameter": args.hydraulic_parameter},
        "repeats": args.repeats, "routes_agree_per_cell": same,
        "evaluate_ms": {r: {"median": statistics.median(v), "min": min(v), "max": max(v)} for r, v in times.items()},
        # a model, not a measurement: bytes of field traffic each route asks of HBM per pass
        "model_bytes": {"refield": 96.0 * rows * cells * len(counts), "fused": 8.0 * rows * cells * -(-len(counts) // _lib.load().gprx_pca_sweep_group())},
    }
    out["speedup_refield_over_fused"] = out["evaluate_ms"]["refield"]["median"] / out["evaluate_ms"]["fused"]["median"]
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for b in (d_mean, d_var, d_truth):
        b.free()
    proj.close()


if __name__ == "__main__":
    main()
