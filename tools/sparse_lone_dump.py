"""Every output of lone sparse calls (gprx_factorize, gprx_objective with masks 15 / 7 / 8, gprx_predict with and without noise) over a
seeded table of cases, written to one .npz -- to compare two builds of the library bit for bit (profiles/sparse_one_route.txt).

    GPRX_LIBRARY=<old>/libgprx.so python tools/sparse_lone_dump.py --out old.npz
    python tools/sparse_lone_dump.py --out new.npz
    python tools/sparse_lone_dump.py --compare old.npz new.npz      (no GPU: equal arrays, and the largest difference of the others)
    python tools/sparse_lone_dump.py --time                         (lone-call medians at N = 4096, d = 10, one JSON line each)

The table: M = 40 with "sgpr_fused" 1 and 0, M = 64 .. 320 on both sides of every mp step, np below, at and above the split-K switch
(1024), ARD and one lengthscale, both distance forms, two kernels, 9 / 4097 / 8193 test points, d = 70 at M = 40 and M = 130; every case
once more under gprx_set_profiling(1)."""
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from gpras_amd import _lib
from gpras_amd._lib import check, ptr
from gpras_amd.synth import make_regression
from oracle import kernels as okn
from oracle import transforms as otr

# (kernel, ard, form, d, m, n, ns, sgpr_fused)
TABLE = [("RBF", 0, 0, 10, 40, 700, 9, 1), ("Matern32", 1, 0, 10, 40, 1100, 4097, 0), ("RBF", 1, 1, 10, 64, 1100, 9, 1),
         ("Matern32", 0, 0, 10, 65, 700, 4097, 1), ("RBF", 0, 0, 10, 128, 1100, 8193, 1), ("Matern32", 1, 1, 10, 130, 1000, 9, 1),
         ("RBF", 1, 0, 10, 300, 1100, 4097, 1), ("Matern32", 0, 0, 10, 320, 700, 8193, 1), ("Matern32", 1, 0, 70, 40, 700, 4097, 1),
         ("RBF", 1, 0, 70, 130, 1100, 9, 1)]


def inputs(seed, kernel, ard, form, d, m, n, ns, fused):
    x, y, xs = make_regression(n, d, n_outputs=2, n_test=ns, config=33, unit=seed)
    rng = np.random.default_rng(500 + seed)
    ls = np.sqrt(d) * rng.uniform(0.6, 1.6, d if ard else 1)
    theta = np.ascontiguousarray(np.concatenate([np.atleast_1d(w) for w in otr.unconstrain(rng.uniform(0.5, 2.0), ls, 10.0 ** rng.uniform(-2.0, -0.5))]))
    z = np.ascontiguousarray(x[rng.choice(n, size=m, replace=False)] + 1e-3 * rng.standard_normal((m, d)))
    return x, y, xs, theta, z


def handle(lib, kernel, ard, form, d, m, x, y, fused, profiling):
    h = C.c_void_p()
    check(lib.gprx_create(0, x.shape[0], d, m, okn.KERNEL_IDS[kernel], ard, C.byref(h)))
    check(lib.gprx_set_data(h, ptr(x), ptr(y), y.shape[1]), h)
    check(lib.gprx_set_distance_form(h, form), h)
    check(lib.gprx_set_handle_tuning(h, b"sgpr_fused", fused), h)
    check(lib.gprx_set_profiling(h, profiling), h)
    return h


def dump(path):
    lib, out = _lib.load(), {}
    for profiling in (0, 1):
        for seed, case in enumerate(TABLE):
            kernel, ard, form, d, m, n, ns, fused = case
            x, y, xs, theta, z = inputs(seed, *case)
            key = f"{kernel}-ard{ard}-form{form}-d{d}-m{m}-n{n}-ns{ns}-fused{fused}-prof{profiling}"
            h = handle(lib, kernel, ard, form, d, m, x, y, fused, profiling)
            try:
                loss = C.c_double()
                check(lib.gprx_factorize(h, 1, ptr(theta), ptr(z), 15, C.byref(loss)), h)
                out[key + "/factorize"] = np.array(loss.value)
                for noise in (1, 0):
                    mean, var = np.zeros(ns), np.zeros(ns)
                    check(lib.gprx_predict(h, ptr(xs), ns, ptr(mean), ptr(var), noise), h)
                    out[key + f"/mean{noise}"], out[key + f"/var{noise}"] = mean, var
                for mask in (15, 7, 8):  # (one shape: launched eagerly, captured, replayed)
                    grad = np.zeros(theta.size + z.size)
                    check(lib.gprx_objective(h, 1, ptr(theta), ptr(z), mask, C.byref(loss), ptr(grad)), h)
                    out[key + f"/loss{mask}"], out[key + f"/grad{mask}"] = np.array(loss.value), grad
                mean, var = np.zeros(ns), np.zeros(ns)
                check(lib.gprx_predict(h, ptr(xs), ns, ptr(mean), ptr(var), 1), h)  # from the factorisation the objective left
                out[key + "/mean_after_objective"], out[key + "/var_after_objective"] = mean, var
            finally:
                lib.gprx_destroy(h)
            print(key, "finite", all(bool(np.isfinite(v).all()) for k, v in out.items() if k.startswith(key)), flush=True)
    np.savez(path, **out)


def compare(a, b):
    a, b = np.load(a), np.load(b)
    assert sorted(a.files) == sorted(b.files)
    equal = [k for k in a.files if np.array_equal(a[k], b[k])]
    print(f"{len(a.files)} arrays, {len(equal)} equal bit for bit")
    for k in sorted(set(a.files) - set(equal)):
        print(f"  differs: {k}: max |a - b| / max |a| = {np.max(np.abs(a[k] - b[k])) / np.max(np.abs(a[k])):.2e}")
    return len(equal) == len(a.files)


def median_ms(call):
    for _ in range(3):
        call()
    t0 = time.perf_counter()
    call()
    reps = int(min(2000, max(5, 1.0 / (time.perf_counter() - t0))))
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()  # (every one of these calls returns after its stream has been waited for)
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), reps


def timings():
    lib = _lib.load()
    for m, fused in ((128, 1), (300, 1), (50, 0)):
        case = ("RBF", 0, 0, 10, m, 4096, 100000, fused)
        x, y, xs, theta, z = inputs(77, *case)
        h = handle(lib, "RBF", 0, 0, 10, m, x, y, fused, 0)
        loss, grad, mean, var = C.c_double(), np.zeros(theta.size + z.size), np.zeros(xs.shape[0]), np.zeros(xs.shape[0])
        row = {"m": m, "sgpr_fused": fused}
        row["factorize_ms"], row["factorize_reps"] = median_ms(lambda: check(lib.gprx_factorize(h, 0, ptr(theta), ptr(z), 15, C.byref(loss)), h))
        row["objective_ms"], row["objective_reps"] = median_ms(lambda: check(lib.gprx_objective(h, 0, ptr(theta), ptr(z), 15, C.byref(loss), ptr(grad)), h))
        check(lib.gprx_factorize(h, 0, ptr(theta), ptr(z), 15, C.byref(loss)), h)
        row["predict_ms"], row["predict_reps"] = median_ms(lambda: check(lib.gprx_predict(h, ptr(xs), xs.shape[0], ptr(mean), ptr(var), 1), h))
        lib.gprx_destroy(h)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--out"]:
        dump(sys.argv[2])
    elif sys.argv[1:2] == ["--compare"]:
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
    elif sys.argv[1:2] == ["--time"]:
        timings()
    else:
        sys.exit(__doc__)
