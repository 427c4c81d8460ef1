"""The two measurements behind DESIGN section 3.22b (held-out rows in the general sparse launch sequence), into one JSON file.

    python tools/crossval_general_probe.py --parent-lib PATH/libgprx.so [--out profiles/crossval_general_probe.json]
                                           [--skip-no-cost] [--skip-crossval] [--m 100 300]

1. "No cost to calls without holds": gprx_adam_batch at N = 4096, d = 10, 16 cells, M = 128 and M = 300, STEPS steps, through a build of
   the parent commit's library (``--parent-lib``) and through this tree's, alternating in one process: parent, head, parent, head, each
   visit one warm run and three timed ones -- six timed runs per library.  Per-step time = wall time around the call / steps taken.  The
   variables the two libraries leave behind are compared bit for bit.
2. "What the feature buys": ``cross_validate`` at N = 4096, d = 10, K = 10, 35 events (34 of 117 rows and one of 118), M = 100 and M = 300,
   two-stage at max_iter = 100 and adam at max_iter = 500, ``route="held_general"`` against ``route="engines"``: wall time around the call
   (which ends with the results on the host) after a warm call of each route at max_iter = 2; the held route's time split into its stages
   (init = the per-fold k-means, fit, predict).

The file is rewritten after every entry, so a run that is cut short keeps what it measured.
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

N, D, CELLS = 4096, 10, 16
STEPS = 200
REPEATS = 3
_vp = C.c_void_p


def _bind(path):
    """The few entry points the first measurement needs, from any build of the library."""
    lib = C.CDLL(str(path))
    for name in ("gprx_create", "gprx_destroy", "gprx_set_data", "gprx_adam_batch", "gprx_last_optimizer_route"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.PROTOTYPES[name]
    return lib


def _adam_inputs(m):
    from gpras_amd.model import softplus_inv

    x, y, _ = make_regression(N, D, n_outputs=CELLS, n_test=0, config=33, unit=m)
    rng = np.random.default_rng(m)
    ini = float(np.mean(np.abs(x)))
    theta = np.tile(np.array([softplus_inv(1.0), softplus_inv(ini), softplus_inv(1.0 - 1e-6)], dtype=np.float64), (CELLS, 1))
    zs = np.stack([x[rng.choice(N, size=m, replace=False)] + 1e-3 * rng.standard_normal((m, D)) for _ in range(CELLS)])
    return x, y, np.ascontiguousarray(theta), np.ascontiguousarray(zs)


def _adam_run(lib, m, x, y, theta, zs):
    h = _vp()
    assert lib.gprx_create(0, N, D, m, 0, 0, C.byref(h)) == 0
    try:
        assert lib.gprx_set_data(h, _lib.ptr(x), _lib.ptr(y), CELLS) == 0
        units = np.arange(CELLS, dtype=np.int32)
        times, out = [], None
        for rep in range(REPEATS + 1):  # (the first run warms: allocations, code objects, the captured step)
            th, z = theta.copy(), zs.copy()
            ev, batches = np.zeros(CELLS, dtype=np.int32), C.c_int()
            t0 = time.perf_counter()
            rc = lib.gprx_adam_batch(h, CELLS, _lib.ptr(units), _lib.ptr(th), _lib.ptr(z), 15, STEPS, _lib.ptr(ev), C.byref(batches))
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


def measure_no_cost(parent_path, save):
    libs = {"parent": _bind(parent_path), "head": _bind(_lib.LIB_PATH)}
    res = {"N": N, "d": D, "cells": CELLS, "max_steps": STEPS}
    for m in (128, 300):
        x, y, theta, zs = _adam_inputs(m)
        per = {"parent": [], "head": []}
        last = {}
        for _ in range(2):
            for name in ("parent", "head"):
                times, out, route = _adam_run(libs[name], m, x, y, theta, zs)
                per[name] += times
                last[name] = out
                assert route == 2
        same = all(np.array_equal(a, b) for a, b in zip(last["parent"], last["head"]))
        res[f"M_{m}"] = {
            "steps": int(last["head"][2].max()),
            "us_per_step_parent": per["parent"],
            "us_per_step_head": per["head"],
            "parent_min_max": [min(per["parent"]), max(per["parent"])],
            "head_min_max": [min(per["head"]), max(per["head"])],
            "parent_median": float(np.median(per["parent"])),
            "head_median": float(np.median(per["head"])),
            "head_median_above_parent_slowest": bool(float(np.median(per["head"])) > max(per["parent"])),
            "variables_bit_equal": bool(same),
        }
        print(m, res[f"M_{m}"], flush=True)
        save("no_cost_without_holds", res)
    return res


def measure_crossval(ms, save, earlier):
    from gpras_amd.crossval import cross_validate

    k = 10
    x, y, _ = make_regression(N, D, n_outputs=k, n_test=0, config=33, unit=99)
    events = [(117 * e, 117 * (e + 1)) for e in range(34)] + [(117 * 34, N)]
    res = dict(earlier)  # (a run per M: each adds its entries)
    res.update({"N": N, "d": D, "K": k, "events": len(events), "cells": len(events) * k})
    for m in ms:
        for method, iters in (("two-stage", 100), ("adam", 500)):
            entry = {}
            for route in ("held_general", "engines"):
                cross_validate("RBF", x, y, events, m, optimization_method=method, route=route, max_iter=2)  # warm
                t0 = time.perf_counter()
                out = cross_validate("RBF", x, y, events, m, optimization_method=method, route=route, max_iter=iters)
                dt = time.perf_counter() - t0
                rmse, nlpd = out.scores(y)
                entry[route] = {"wall_s": dt, "stages_ms": out.last_timings_ms, "evaluations_max": int(out.n_evals.max()),
                                "evaluations_total": int(out.n_evals.sum()), "mean_rmse": float(rmse.mean()), "mean_nlpd": float(nlpd.mean()),
                                "loss_first_mean": float(out.first_loss.mean()), "loss_last_mean": float(out.last_loss.mean())}
                print(m, method, route, entry[route], flush=True)
            entry["engines_over_held_general"] = entry["engines"]["wall_s"] / entry["held_general"]["wall_s"]
            entry["fit_engines_over_held_general"] = entry["engines"]["stages_ms"]["fit_ms"] / entry["held_general"]["stages_ms"]["fit_ms"]
            res[f"M_{m}_{method}_max_iter_{iters}"] = entry
            save("cross_validate_held_general_against_engines", res)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "crossval_general_probe.json"))
    ap.add_argument("--skip-no-cost", action="store_true")
    ap.add_argument("--skip-crossval", action="store_true")
    ap.add_argument("--m", type=int, nargs="*", default=[100, 300])
    args = ap.parse_args()
    out = Path(args.out)
    result = json.loads(out.read_text()) if out.exists() else {}
    result.setdefault("commands", []).append("python tools/crossval_general_probe.py " + " ".join(sys.argv[1:]))

    def save(key, value):
        result[key] = value
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(result, indent=1) + "\n")

    if not args.skip_no_cost:
        if not args.parent_lib:
            ap.error("--parent-lib is needed for the first measurement")
        measure_no_cost(args.parent_lib, save)
    if not args.skip_crossval:
        measure_crossval(args.m, save, result.get("cross_validate_held_general_against_engines", {}))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
