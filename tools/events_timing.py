"""Time the storm-event selection: the reference's four stages on the CPU (``EventSelection`` of
production/pre_processing/event_selection.py, run as it is) and the stages of ``gpras_amd.events.EventSelector`` on the device, on
synthetic storms of (events, hours) = (3000, 72) and (20000, 96).

    python tools/events_timing.py --device   [--out profiles/events_timing.json]       # needs the GPU
    python tools/events_timing.py --reference PATH_TO_REFERENCE_CHECKOUT [--out ...]   # CPU only

Either part merges its numbers into the JSON file, so the two can run on different machines.  Device stage times are device events
(``gprx_ev_timings``); the wall times are host clocks around calls that end in a stream synchronise.  Every size is run once untimed
first (code objects load at first launch), then ``--repeats`` times; the median is kept, the spread is recorded.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = ((3000, 72), (20000, 96))
TARGET_RPS = [2, 5, 10, 25, 50, 100, 200, 500, 1000, 2000]
N_TRAIN, N_TEST = 35, 14


def synthetic_storms(n_events: int, n_hours: int, seed: int = 7):
    """Long-format columns of ragged gamma-pulse storms, rows shuffled: (event_id, datetime, precip_excess, precip_cum, inflow)."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(n_hours // 2, n_hours + 1, size=n_events)
    lengths[0] = n_hours
    ev = np.repeat(np.arange(n_events, dtype=np.int64), lengths)
    first = np.cumsum(lengths) - lengths
    t = (np.arange(ev.size) - first[ev]).astype(np.float64) + 1.0
    amp = np.exp(rng.normal(0.0, 0.9, size=n_events))

    def pulse(peak, shape):
        x = t / peak[ev]
        return x ** shape[ev] * np.exp(shape[ev] * (1.0 - x))

    pe = 0.4 * amp[ev] * pulse(2.0 + 0.35 * n_hours * rng.random(n_events), 1.5 + 2.0 * rng.random(n_events))
    pc = np.cumsum(pe)
    pc = pc - (pc[first] - pe[first])[ev]  # the cumulative sum restarts with every event
    q = (-3.0 + 40.0 * rng.random(n_events))[ev] + 900.0 * (amp * np.exp(rng.normal(0.0, 0.35, size=n_events)))[ev] * pulse(
        4.0 + 0.45 * n_hours * rng.random(n_events), 2.0 + 2.0 * rng.random(n_events))
    start = np.datetime64("2026-01-01T00:00:00", "ns") + (rng.integers(0, 24 * 365, size=n_events) * 3600 * 10**9).astype("timedelta64[ns]")
    dt = start[ev] + ((t - 1.0).astype(np.int64) * 3600 * 10**9).astype("timedelta64[ns]")
    perm = rng.permutation(ev.size)
    return ev[perm] * 3 + 11, dt[perm], pe[perm], pc[perm], q[perm]


def median_and_spread(samples):
    a = np.asarray(samples, dtype=np.float64)
    return {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max())}


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t0)


def time_device(repeats: int) -> dict:
    from gpras_amd.events import EventSelector

    out = {}
    for n_events, n_hours in SIZES:
        cols = synthetic_storms(n_events, n_hours)
        runs = []
        for rep in range(repeats + 1):
            row = {}
            sel, row["host_lexsort_and_checks_wall"] = clock(lambda: EventSelector(*cols, test_rp_range=[2, 2000]))
            _, row["upload_pivot_maxima_wall"] = clock(lambda: sel.handle)
            _, row["event_max_wall"] = clock(lambda: sel.event_max)
            aep, row["select_aep_host_wall"] = clock(lambda: sel.select_aep(TARGET_RPS))
            _, row["select_diverse_wall"] = clock(lambda: sel.select_diverse(aep["event_id"].tolist(), N_TRAIN - len(aep)))
            row["host_eigh_wall"] = sel.host_eigh_ms
            _, row["select_test_host_wall"] = clock(lambda: sel.select_test([2, 2000], N_TEST, aep["event_id"].tolist() + list(sel.diverse_order_)))
            for name, ms in sel.stage_timings_ms().items():
                row["device_" + name] = ms
            sel.close()
            if rep:  # the first pass warms up
                runs.append(row)
        out[f"{n_events}x{n_hours}"] = {"rows": int(cols[0].size), "repeats": repeats, "n_aep": int(len(aep)),
                                        "stages": {k: median_and_spread([r[k] for r in runs]) for k in runs[0]}}
    return out


def time_reference(path: str, repeats: int) -> dict:
    import pandas as pd

    sys.path.insert(0, os.path.join(path, "production", "pre_processing"))
    import event_selection as ref_mod

    out = {}
    for n_events, n_hours in SIZES:
        ev, dt, pe, pc, q = synthetic_storms(n_events, n_hours)
        df = pd.DataFrame({"event_id": ev, "datetime": dt, "precip-excess": pe, "precip-cum": pc, "inflow": q})
        runs = []
        with tempfile.TemporaryDirectory() as tmp:
            pq = os.path.join(tmp, "storms.pq")
            df.to_parquet(pq)
            for rep in range(repeats + 1):
                row = {}
                with np.errstate(all="ignore"):
                    ref, row["read_parquet_and_return_periods"] = clock(lambda: ref_mod.EventSelection(pq, test_rp_range=[2, 2000]))
                    _, row["return_periods"] = clock(ref._calculate_return_periods)
                    aep, row["select_aep"] = clock(lambda: ref._select_aep_storms(TARGET_RPS))
                    div, row["select_diverse"] = clock(lambda: ref._select_diverse_storms(aep.event_id.tolist(), N_TRAIN - len(aep)))
                    _, row["select_test"] = clock(lambda: ref._select_test_storms([2, 2000], N_TEST, aep.event_id.tolist() + div.event_id.tolist()))
                if rep:
                    runs.append(row)
        out[f"{n_events}x{n_hours}"] = {"rows": int(ev.size), "repeats": repeats, "stages": {k: median_and_spread([r[k] for r in runs]) for k in runs[0]}}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", action="store_true", help="time EventSelector on the GPU")
    ap.add_argument("--reference", metavar="PATH", help="time the reference's EventSelection from this checkout (CPU)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_timing.json"))
    args = ap.parse_args()
    if not args.device and not args.reference:
        ap.error("nothing to do: give --device and / or --reference PATH")
    result = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            result = json.load(f)
    if args.device:
        if not os.path.exists("/dev/kfd"):
            raise SystemExit("--device needs a GPU: no device time is ever estimated on a CPU")
        result["device"] = time_device(args.repeats)
    if args.reference:
        result["reference_cpu"] = time_reference(args.reference, args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
