"""The two measurements behind DESIGN section 3.22 (event-fold cross-validation), into one JSON file.

    python tools/crossval_probe.py --parent-lib PATH/libgprx.so [--out profiles/crossval_probe.json] [--skip-crossval]

1. "No cost to calls without holds": gprx_adam_batch at N = 4096, d = 10, M = 50 with 16 and 50 cells, 2 000 steps, through a build of the
   parent commit's library (``--parent-lib``) and through this tree's, alternating in one process, REPEATS timed runs each after one
   warm run.  Per-step time = wall time around the call / steps taken.  The variables the two libraries leave behind are compared bit
   for bit.
2. "What the feature buys": ``cross_validate`` at N = 4096, d = 10, K = 10, M = 50, 35 events (34 of 117 rows and one of 118), two-stage at
   max_iter = 100 and adam at max_iter = 2 000, ``route="held"`` against ``route="engines"``: wall time around the call (which ends with
   the results on the host), after a warm call of each route at max_iter = 2.
"""

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from gpras_amd import _lib  # noqa: E402
from gpras_amd.synth import make_regression  # noqa: E402

N, D, M = 4096, 10, 50
STEPS = 2000
REPEATS = 3
_vp, _i64 = C.c_void_p, C.c_int64


def _bind(path):
    """The few entry points the first measurement needs, from any build of the library (the parent's lacks the held forms that
    ``_lib.load`` insists on)."""
    lib = C.CDLL(str(path))
    for name in ("gprx_create", "gprx_destroy", "gprx_set_data", "gprx_adam_batch", "gprx_last_optimizer_route"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.PROTOTYPES[name]
    return lib


def _adam_inputs(cells):
    x, y, _ = make_regression(N, D, n_outputs=cells, n_test=0, config=33, unit=cells)
    rng = np.random.default_rng(cells)
    ini = float(np.mean(np.abs(x)))
    from gpras_amd.model import softplus_inv

    theta = np.tile(np.array([softplus_inv(1.0), softplus_inv(ini), softplus_inv(1.0 - 1e-6)], dtype=np.float64), (cells, 1))
    zs = np.stack([x[rng.choice(N, size=M, replace=False)] + 1e-3 * rng.standard_normal((M, D)) for _ in range(cells)])
    return x, y, np.ascontiguousarray(theta), np.ascontiguousarray(zs)


def _adam_run(lib, cells, x, y, theta, zs):
    h = _vp()
    assert lib.gprx_create(0, N, D, M, 0, 0, C.byref(h)) == 0
    try:
        assert lib.gprx_set_data(h, _lib.ptr(x), _lib.ptr(y), cells) == 0
        units = np.arange(cells, dtype=np.int32)
        times, out = [], None
        for rep in range(REPEATS + 1):  # (the first run warms: allocations, code objects)
            th, z = theta.copy(), zs.copy()
            ev, batches = np.zeros(cells, dtype=np.int32), C.c_int()
            t0 = time.perf_counter()
            rc = lib.gprx_adam_batch(h, cells, _lib.ptr(units), _lib.ptr(th), _lib.ptr(z), 15, STEPS, _lib.ptr(ev), C.byref(batches))
            dt = time.perf_counter() - t0
            assert rc == 0, rc
            if rep > 0:
                times.append(1e6 * dt / max(int(ev.max()), 1))
            out = (th, z, ev)
        route, waits = C.c_int(), C.c_int()
        lib.gprx_last_optimizer_route(h, C.byref(route), C.byref(waits))
        return times, out, route.value
    finally:
        lib.gprx_destroy(h)


def measure_no_cost(parent_path):
    libs = {"parent": _bind(parent_path), "head": _bind(_lib.LIB_PATH)}
    res = {}
    for cells in (16, 50):
        x, y, theta, zs = _adam_inputs(cells)
        per = {"parent": [], "head": []}
        last = {}
        for _ in range(2):  # parent, head, parent, head: each with its own warm run and REPEATS timed ones
            for name in ("parent", "head"):
                times, out, route = _adam_run(libs[name], cells, x, y, theta, zs)
                per[name] += times
                last[name] = out
                assert route == 1
        same = all(np.array_equal(a, b) for a, b in zip(last["parent"], last["head"]))
        res[f"{cells}_cells"] = {
            "steps": int(last["head"][2].max()),
            "us_per_step_parent": per["parent"],
            "us_per_step_head": per["head"],
            "parent_min_max": [min(per["parent"]), max(per["parent"])],
            "head_median": float(np.median(per["head"])),
            "head_median_within_parent_spread": bool(min(per["parent"]) <= float(np.median(per["head"])) <= max(per["parent"])),
            "variables_bit_equal": bool(same),
        }
        print(cells, res[f"{cells}_cells"], flush=True)
    return res


def measure_crossval():
    from gpras_amd.crossval import cross_validate

    k = 10
    x, y, _ = make_regression(N, D, n_outputs=k, n_test=0, config=33, unit=99)
    events = [(117 * e, 117 * (e + 1)) for e in range(34)] + [(117 * 34, N)]
    res = {"N": N, "d": D, "K": k, "M": M, "events": len(events), "cells": len(events) * k}
    for method, iters in (("two-stage", 100), ("adam", 2000)):
        entry = {}
        for route in ("held", "engines"):
            cross_validate("RBF", x, y, events, M, optimization_method=method, route=route, max_iter=2)  # warm
            t0 = time.perf_counter()
            out = cross_validate("RBF", x, y, events, M, optimization_method=method, route=route, max_iter=iters)
            dt = time.perf_counter() - t0
            rmse, nlpd = out.scores(y)
            entry[route] = {"wall_s": dt, "stages_ms": out.last_timings_ms, "evaluations_max": int(out.n_evals.max()),
                            "evaluations_total": int(out.n_evals.sum()), "mean_rmse": float(rmse.mean()), "mean_nlpd": float(nlpd.mean()),
                            "loss_first_mean": float(out.first_loss.mean()), "loss_last_mean": float(out.last_loss.mean())}
            print(method, route, entry[route], flush=True)
        entry["engines_over_held"] = entry["engines"]["wall_s"] / entry["held"]["wall_s"]
        entry["fit_engines_over_held"] = entry["engines"]["stages_ms"]["fit_ms"] / entry["held"]["stages_ms"]["fit_ms"]
        res[f"{method}_max_iter_{iters}"] = entry
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "crossval_probe.json"))
    ap.add_argument("--skip-crossval", action="store_true")
    args = ap.parse_args()
    result = {"command": "python tools/crossval_probe.py " + " ".join(sys.argv[1:]), "no_cost_without_holds": measure_no_cost(args.parent_lib)}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    if not args.skip_crossval:
        result["cross_validate_held_against_engines"] = measure_crossval()
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
