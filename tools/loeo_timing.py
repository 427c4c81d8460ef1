"""Times both leave-one-event-out routes (gpras_amd/loeo.py) on one GPU at N = 4096, d = 10, M = 50, 16 modes and 35
equal events, in one process: python tools/loeo_timing.py.  Prints one JSON object: wall seconds of leave_event_out per route (the
first call and three later ones), the stage times of gprx_last_loeo, the agreement of the two routes, Engine.loeo_batch alone."""
import json, time, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gpras_amd.engine import Engine
from gpras_amd.synth import make_regression
from gpras_amd import loeo

n, d, m, k, ne = 4096, 10, 50, 16, 35
x, y, _ = make_regression(n, d, n_outputs=k, config=1, unit=0)
rows = np.linspace(0, n - 1, m).astype(int)
zs = np.stack([x[rows] + 0.01 * (c + 1) for c in range(k)])
sp_inv = lambda u: u + np.log(-np.expm1(-u))
thetas = np.stack([[sp_inv(1.0 + 0.02 * c), sp_inv(2.0 + 0.05 * c), sp_inv(0.1)] for c in range(k)])
cuts = np.linspace(0, n, ne + 1).astype(int)
ranges = [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]

class Mode:
    def __init__(s, b, u): s.backend, s.unit, s.Z = b, u, zs[u]
    def theta(s): return thetas[s.unit]
class G: pass
g = G(); g.kernel_str, g.ard, g.distance_form, g.device = "RBF", False, "difference", 0
g.x, g.y = x, y
eng = Engine("RBF", x, y, m)
g.models = [Mode(eng, u) for u in range(k)]
out = {}
for route in ("downdate", "refactor"):
    times = []
    for rep in range(4):  # the first run of each route loads code objects and allocates
        t0 = time.perf_counter()
        mean, var = loeo.leave_event_out(g, ranges, route=route)
        times.append(time.perf_counter() - t0)
    out[route] = {"first_s": times[0], "later_s": sorted(times[1:])}
    if route == "downdate":
        out["stages_ms"] = eng.last_loeo()[1]
        down = (mean, var)
    else:
        out["max_rel_diff_mean"] = float(np.max(np.abs(mean - down[0])) / np.max(np.abs(mean)))
        out["max_rel_diff_var"] = float(np.max(np.abs(var - down[1]) / var))
# the Engine call alone (no Python scatter)
units = list(range(k))
ts = []
for rep in range(5):
    t0 = time.perf_counter(); eng.loeo_batch(units, thetas, zs, ranges); ts.append(time.perf_counter() - t0)
out["engine_call_s"] = sorted(ts)
out["stages_ms_engine_call"] = eng.last_loeo()[1]
print(json.dumps(out, indent=1))
