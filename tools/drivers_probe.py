"""Time the optimiser drivers on one MI355X: GPRAS.fit on sparse models (RBF, N = 4096, d = 10, M = 50 or ``--m``, 16 modes) with
``three-stage``, ``adadelta``, ``diffential_evolution``, ``stochastic`` and, for scale, ``adam``.  Per driver one warm-up fit, then
three timed fits (a host clock around the optimiser loop over the modes, GPRAS._run_optimizers, which ends in a synchronising
download; the handle, the upload of the data and the k-means initialisation are outside the window); reported: best, the spread (min
to max of the three) and the evaluation count.  Not a test and not bench.py.  Only the package's public interface is used, so the
same file also times a checkout of an earlier commit (where the engine has no ``last_optimizer_route`` the route is reported as null).

    python tools/drivers_probe.py [--out FILE.json] [--tiny] [--m M] [--drivers adam,adadelta]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpras_amd.gpr import GPRAS  # noqa: E402
from gpras_amd.synth import make_regression  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--tiny", action="store_true", help="a rehearsal of the script itself at toy sizes")
ap.add_argument("--m", type=int, default=50, help="inducing points per model (M > 64 takes the general launch sequence)")
ap.add_argument("--drivers", default=None, help="comma-separated subset of the drivers (default: all five)")
args = ap.parse_args()

n, d, m, modes = (4096, 10, args.m, 16) if not args.tiny else (256, 3, min(args.m, 8), 3)
scale = 1 if not args.tiny else 50
DRIVERS = [
    ("three-stage", lambda: {"max_iter": 100 // scale}),
    ("adadelta", lambda: {"max_iter": 1000 // scale}),
    ("diffential_evolution", lambda: {"adam_iter": 3000 // scale, "popsize": 3, "max_iter": 2, "seed": 3, "verbose": False}),
    ("stochastic", lambda: {"n_starts": max(2, 40 // scale), "iter_initial": max(2, 20 // scale), "iter_final": 10, "rng": np.random.default_rng(5)}),
    ("adam", lambda: {"max_iter": 1000 // scale}),
]

if args.drivers:
    DRIVERS = [dr for dr in DRIVERS if dr[0] in args.drivers.split(",")]

x, y, _ = make_regression(n, d, n_outputs=modes, n_test=0, config=2, unit=0)
result = {"kernel": "RBF", "n": n, "d": d, "m": m, "modes": modes, "drivers": {}}
for name, kwargs in DRIVERS:
    times, evals, stats = [], 0, None
    for rep in range(4):  # (the first fit is the warm-up)
        g = GPRAS("RBF")
        g.x, g.y = x, y
        g._init_models(x, y, m, "kmeans")
        kw = kwargs()
        t0 = time.perf_counter()
        g._run_optimizers(g.models, name, None, kw)
        dt = time.perf_counter() - t0
        evals, stats = sum(mod.n_evals for mod in g.models), getattr(g, "lockstep_stats", None)
        route = [list(eng.last_optimizer_route()) if hasattr(eng, "last_optimizer_route") else None for eng in g.engines]
        for eng in g.engines:
            eng.close()
        if rep > 0:
            times.append(dt)
    entry = {"kwargs": {k: v for k, v in kwargs().items() if k != "rng"}, "best_s": min(times), "min_s": min(times), "max_s": max(times),
             "times_s": times, "evaluations": evals, "lockstep_stats": stats,
             "route_and_host_waits": route}
    if name in ("adam", "adadelta"):
        entry["per_step_us"] = 1e6 * min(times) / max(1, evals // modes)
    result["drivers"][name] = entry
    print(name, json.dumps(entry), flush=True)
print(json.dumps(result), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
