"""Times the blocked leave-one-event-out route against the refactor route (gpras_amd/loeo.py) on one GPU at
N = 4096, d = 10, RBF, 16 modes and 35 equal events, with M = 100 and M = 300, in one process:

    python tools/loeo_blocked_timing.py [--out profiles/loeo_blocked_timing.json] [--quick]

Per M: wall seconds of leave_event_out per route (host arrays in and out; the first call and three later ones), the six stage times
and the group count of gprx_last_loeo_blocked, and the agreement of the two routes.  Then the measurements the fixed choices of
gp_loeo_blocked.h rest on, per mp = 64 ... 320 (M = 60, 100, 180, 250, 300; blocked route only): the Cholesky-plus-inverse stage under
each schedule of chol(H) ("loeo_blocked_potrf" 0 / 1 / 2 -- the inverse is the same launches under all three, so differences are the
factorisation's).  Every figure of a candidate: one warm-up call, then the median and the range of five.  --quick: M = 100 only, no refactor route."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gpras_amd import _lib, loeo
from gpras_amd.engine import Engine
from gpras_amd.synth import make_regression

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--quick", action="store_true")
args = ap.parse_args()

n, d, k, ne = 4096, 10, 16, 35
x, y, _ = make_regression(n, d, n_outputs=k, config=1, unit=0)
sp_inv = lambda u: u + np.log(-np.expm1(-u))
thetas = np.stack([[sp_inv(1.0 + 0.02 * c), sp_inv(2.0 + 0.05 * c), sp_inv(0.1)] for c in range(k)])
cuts = np.linspace(0, n, ne + 1).astype(int)
ranges = [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]
units = list(range(k))
lib = _lib.load()


def inducing(m):
    rows = np.linspace(0, n - 1, m).astype(int)
    return np.stack([x[rows] + 0.01 * (c + 1) for c in range(k)])


class Mode:
    def __init__(s, b, u, zs): s.backend, s.unit, s.Z = b, u, zs[u]
    def theta(s): return thetas[s.unit]
class G: pass


def stage_stats(eng, zs, key, reps=5):
    eng.loeo_batch_blocked(units, thetas, zs, ranges)  # warm-up under this setting
    vals = []
    for _ in range(reps):
        eng.loeo_batch_blocked(units, thetas, zs, ranges)
        vals.append(eng.last_loeo_blocked()[2][key])
    vals.sort()
    return {"median_ms": vals[len(vals) // 2], "min_ms": vals[0], "max_ms": vals[-1], "reps": reps}


out = {"shape": {"n": n, "d": d, "modes": k, "events": ne, "kernel": "RBF"}, "routes": {}, "potrf_route": {}}
for m in ((100,) if args.quick else (100, 300)):
    zs = inducing(m)
    eng = Engine("RBF", x, y, m)
    g = G(); g.kernel_str, g.ard, g.distance_form, g.device = "RBF", False, "difference", 0
    g.x, g.y = x, y
    g.models = [Mode(eng, u, zs) for u in range(k)]
    rec = {}
    for route in (("blocked",) if args.quick else ("blocked", "refactor")):
        times = []
        for rep in range(4):  # the first run of each route loads code objects and allocates
            t0 = time.perf_counter()
            mean, var = loeo.leave_event_out(g, ranges, route=route)
            times.append(time.perf_counter() - t0)
        rec[route] = {"first_s": times[0], "later_s": sorted(times[1:])}
        if route == "blocked":
            ran, groups, stages = eng.last_loeo_blocked()
            rec["groups"], rec["stages_ms"] = groups, stages
            blk = (mean, var)
        else:
            rec["max_rel_diff_mean"] = float(np.max(np.abs(mean - blk[0])) / np.max(np.abs(mean)))
            rec["max_rel_diff_var"] = float(np.max(np.abs(var - blk[1]) / var))
    ts = []
    for rep in range(5):  # the Engine call alone (no Python scatter)
        t0 = time.perf_counter(); eng.loeo_batch_blocked(units, thetas, zs, ranges); ts.append(time.perf_counter() - t0)
    rec["engine_call_s"] = sorted(ts)
    out["routes"][f"M{m}"] = rec
    eng.close()
    print(json.dumps({f"M{m}": rec}), flush=True)

for m in ((100,) if args.quick else (60, 100, 180, 250, 300)):
    mp = 64 * ((m + 63) // 64)
    zs = inducing(m)
    eng = Engine("RBF", x, y, m)
    try:
        rec = {}
        for route, name in ((0, "fused_panel"), (1, "split_panel"), (2, "cell_kernel")):
            if route == 2 and mp == 64:
                continue
            assert lib.gprx_set_tuning(b"loeo_blocked_potrf", route) == 0
            rec[name] = stage_stats(eng, zs, "chol_inverse_ms")
        lib.gprx_set_tuning(b"loeo_blocked_potrf", -1)
        out["potrf_route"][f"mp{mp}"] = rec
        print(json.dumps({f"mp{mp}": rec}), flush=True)
    finally:
        lib.gprx_set_tuning(b"loeo_blocked_potrf", -1)
        eng.close()

text = json.dumps(out, indent=1)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
print(text)
