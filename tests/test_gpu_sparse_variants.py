"""Every compiled variant of the fused sparse evaluation (sgpr_fused.h, M <= 64) and of the resident Adam loop against the oracle.

Pass 1 and pass 2 are compiled per (kernel id, distance form, isotropy, NP) with NP = 6 for d <= 12, 8 for d <= 16 and 0 (the
restaging variants) above; pass 2 and the merged Adam + prep launch are templated on ISO = (not ARD and difference form).  The case
table below holds one case per (kernel, class, NP) -- 45 pass-2 instantiations, 15 Adam ones -- and rotates the edges of d, M and N
through them; ``test_case_table_covers_every_instantiation_and_edge`` (no GPU) checks that it does.

The inputs keep the comparisons non-vacuous: lengthscales sqrt(d) U(0.6, 1.6) keep Kuf away from underflow at d = 64 (the test
asserts the median of Kuf / variance), and Z sits on data rows plus 1e-3 noise, off r = 0.
"""

import ctypes as C
import time

import numpy as np
import pytest

from gpras_amd import _lib
from gpras_amd._lib import check, ptr
from gpras_amd.synth import make_regression
from oracle import kernels as okn
from oracle import sgpr as osg
from oracle import transforms as otr

KERNELS = ("RBF", "Matern12", "Matern32", "Matern52", "Exponential")
CLASSES = ("iso", "ard", "expanded")
EXPANDED_ISO = ("Matern12", "Exponential")  # their GPRAS default form is the expanded one (gpr.py DEFAULT_DISTANCE_FORM), isotropic
NP_DIMS = {6: (1, 5, 12), 8: (13, 16), 0: (17, 32, 33, 48, 49, 50, 64)}
M_EDGES = (1, 2, 15, 16, 17, 32, 33, 50, 63, 64)
N_EDGES = (40, 63, 64, 65, 255, 256, 257, 511, 513, 1100)
N_LARGE = 4097  # crosses 16 chunks of 256 columns (and 64 tiles of 64)
SF_DK = 16  # dimensions per staged chunk (sgpr_fused_dev.h)
# Matern12 / Exponential in the expanded form: r^2 = |a|^2 + |b|^2 - 2 a.b leaves a rounding residue of a few ulp of |a|^2 where r = 0
# (the diagonal of Kuu), and r = sqrt(residue) ~ 1e-8 moves k by as much.  The value is then fixed only to that level by ANY
# implementation: the oracle's own loss moves by up to 3.3e-8 and its gradient blocks by up to 5.5e-7 when only the order of the
# dimensions in its sums changes (all 15 cells of the class's cases, d = 12 .. 50).  That class is held to 3x that instead of 1e-9 / 1e-7;
# an indexing error moves these values by orders of magnitude more.
NONSMOOTH_EXPANDED_TOL = (1e-7, 2e-6)
HYPER = _lib.TRAIN_VARIANCE | _lib.TRAIN_LENGTHSCALE | _lib.TRAIN_NOISE
ALL = HYPER | _lib.TRAIN_Z
# d = 1 with 33 or more inducing points: on a line, their spacing cannot keep cond(Kuu + 1e-6 I) <= 1e6 (2.7e7 .. 7.0e7 here).  Their
# gradient bounds scale with cond / 1e6, as test_gpu_random_sweep.py's do; the case id says so
COND_SCALED = {"RBF-iso-np6-d1-m50-n40", "Matern32-iso-np6-d1-m33-n257", "Matern52-iso-np6-d1-m64-n1100"}


def np_of(d):
    """sf_pass1.hip / sf_pass2.hip launchers: np = d <= 12 ? 6 : (d <= 16 ? 8 : 0)."""
    return 6 if d <= 12 else (8 if d <= SF_DK else 0)


def class_flags(kernel, cls):
    """(ard, form) of a class: iso-difference, ARD-difference, expanded (isotropic for Matern12 / Exponential, ARD otherwise)."""
    if cls == "iso":
        return False, 0
    if cls == "ard":
        return True, 0
    return kernel not in EXPANDED_ISO, 1


def instantiation(kernel, d, ard, form):
    """(kid, form, iso, np) of pass 2, as the launcher picks it: iso = !ard && form == 0."""
    return okn.KERNEL_IDS[kernel], form, int(not ard and form == 0), np_of(d)


def _cases():
    out = []
    for g, (npv, dims) in enumerate(NP_DIMS.items()):
        for k, kernel in enumerate(KERNELS):
            for c, cls in enumerate(CLASSES):
                j = 3 * k + c
                i = 15 * g + j
                d = dims[j % len(dims)]
                m = M_EDGES[i % len(M_EDGES)]
                n = N_EDGES[(i + i // len(N_EDGES)) % len(N_EDGES)]
                if n == 40 and dims[j % len(dims)] == 1:  # (N < M on a line: near-coincident inducing points, no Z-gradient is defined to 1e-2)
                    n = N_EDGES[1]
                if n == 40 and m <= 40:  # N = 40 is the edge N < M
                    m = 50
                if (g, k, c) == (0, 2, 1):
                    n = N_LARGE
                ard, form = class_flags(kernel, cls)
                cid = f"{kernel}-{cls}-np{npv}-d{d}-m{m}-n{n}"
                out.append(dict(id=cid + ("-condscaled" if cid in COND_SCALED else ""), kernel=kernel, cls=cls, d=d, m=m, n=n, ard=ard,
                                form=form, cells=3 + i % 5, seed=i, cond_scaled=cid in COND_SCALED))
    return out


CASES = _cases()

# resident Adam: every (kernel, class) pair once, with d in {3, 14, 20, 50}, M in {1, 17, 64} and the masks 15, 8, 7 spread across them.
# Matern12 and Exponential train no Z beside M > 1: their loss is not differentiable where an inducing point meets a data point, the
# L-BFGS start of the early-stopping cell does not settle there, and that cell would not stop early.
ADAM_TABLE = [("RBF", "iso", 3, 1, 15), ("RBF", "ard", 14, 17, 8), ("RBF", "expanded", 20, 64, 7),
              ("Matern12", "iso", 50, 17, 7), ("Matern12", "ard", 3, 64, 7), ("Matern12", "expanded", 14, 1, 8),
              ("Matern32", "iso", 20, 64, 8), ("Matern32", "ard", 50, 1, 7), ("Matern32", "expanded", 3, 17, 15),
              ("Matern52", "iso", 14, 1, 15), ("Matern52", "ard", 20, 17, 8), ("Matern52", "expanded", 50, 64, 7),
              ("Exponential", "iso", 3, 17, 7), ("Exponential", "ard", 14, 64, 7), ("Exponential", "expanded", 20, 1, 8)]
ADAM_DIMS = (3, 14, 20, 50)
ADAM_MS = (1, 17, 64)
ADAM_MASKS = (15, 8, 7)


def _adam_cases():
    out = []
    for i, (kernel, cls, d, m, mask) in enumerate(ADAM_TABLE):
        ard, form = class_flags(kernel, cls)
        out.append(dict(id=f"{kernel}-{cls}-d{d}-m{m}-mask{mask}", kernel=kernel, cls=cls, d=d, m=m, mask=mask, ard=ard, form=form, seed=i))
    return out


ADAM_CASES = _adam_cases()


def test_case_table_covers_every_instantiation_and_edge():
    """The tables reach all 45 pass-2 instantiations (5 kernels x {iso-difference, ARD-difference, expanded} x NP {6, 8, 0}), all 15
    sf_adam_prep_kernel<KID, FORM, ISO> ones, and every edge of d, M and N listed above."""
    p2 = {instantiation(c["kernel"], c["d"], c["ard"], c["form"]) for c in CASES}
    want = {(kid, form, iso, npv) for kid in range(5) for (form, iso) in ((0, 1), (0, 0), (1, 0)) for npv in (6, 8, 0)}
    assert len(CASES) == 45 and p2 == want
    assert {c["d"] for c in CASES} == {d for dims in NP_DIMS.values() for d in dims}
    assert {c["m"] for c in CASES} == set(M_EDGES)
    assert {c["n"] for c in CASES} == set(N_EDGES) | {N_LARGE}
    assert sum(c["n"] == N_LARGE for c in CASES) == 1
    assert all(c["m"] > c["n"] for c in CASES if c["n"] == 40)
    assert all(3 <= c["cells"] <= 7 for c in CASES)
    assert len({c["id"] for c in CASES}) == 45
    assert all(c["m"] <= 64 for c in CASES)
    adam = {instantiation(c["kernel"], c["d"], c["ard"], c["form"])[:3] for c in ADAM_CASES}
    assert len(ADAM_CASES) == 15 and adam == {(kid, form, iso) for kid in range(5) for (form, iso) in ((0, 1), (0, 0), (1, 0))}
    assert {c["d"] for c in ADAM_CASES} == set(ADAM_DIMS)
    assert {c["m"] for c in ADAM_CASES} == set(ADAM_MS)
    assert {c["mask"] for c in ADAM_CASES} == set(ADAM_MASKS)
    # the expanded class is isotropic exactly for the two kernels whose GPRAS default it is: ISO = 0 with one lengthscale
    assert {(c["kernel"], c["ard"]) for c in CASES if c["form"] == 1} == {(k, k not in EXPANDED_ISO) for k in KERNELS}


# ---- helpers ------------------------------------------------------------------------------------------------------------------


def draw_inputs(case, units=3):
    d, m, n, cells = case["d"], case["m"], case["n"], case["cells"]
    x, y, _ = make_regression(n, d, n_outputs=units, n_test=0, config=31, unit=case["seed"])
    rng = np.random.default_rng(500 + case["seed"])
    nl = d if case["ard"] else 1
    variance = rng.uniform(0.5, 2.0, cells)
    ls = np.sqrt(d) * rng.uniform(0.6, 1.6, (cells, nl))
    noise = 10.0 ** rng.uniform(-2.0, -0.5, cells)
    thetas = np.ascontiguousarray([np.concatenate([np.atleast_1d(w) for w in otr.unconstrain(variance[c], ls[c], noise[c])]) for c in range(cells)])
    zs = np.ascontiguousarray(np.stack([inducing_on_rows(x, m, rng) for _ in range(cells)]))
    units_ = np.ascontiguousarray(rng.integers(0, units, size=cells), dtype=np.int32)
    units_[0], units_[-1] = 0, units - 1  # (mixed units in every batch)
    return x, y, thetas, zs, units_, variance, ls, noise


def inducing_on_rows(x, m, rng):
    """Z on data rows plus 1e-3 noise; where M > N the extra points are data rows moved by 0.3 (one row cannot hold two points)."""
    n, d = x.shape
    rows = rng.choice(n, size=min(m, n), replace=False)
    z = x[rows] + 1e-3 * rng.standard_normal((rows.size, d))
    if m > n:
        z = np.concatenate([z, x[rng.choice(n, size=m - n)] + 0.3 * rng.standard_normal((m - n, d))])
    return z


def ref_eval(case, x, y, z, theta, mask=(True, True, True, True)):
    wl = theta[1:-1] if case["ard"] else float(theta[1])
    loss, g = osg.loss_and_grad(case["kernel"], x, y, z, float(theta[0]), wl, float(theta[-1]), mask, form="expanded" if case["form"] else "direct")
    return loss, np.concatenate([[g["variance"]], np.atleast_1d(g["lengthscales"]), [g["noise"]], np.asarray(g["Z"]).ravel()])


def ls_arg(case, ls):
    return ls if case["ard"] else float(ls[0])


def preconditions(case, x, z, variance, ls):
    """The median of Kuf / variance and cond(Kuu + 1e-6 I) of one cell: the comparison is not vacuous, and well posed."""
    form = "expanded" if case["form"] else "direct"
    kuf = okn.kmat(case["kernel"], z, x, variance, ls_arg(case, ls), form)
    kuu = okn.kmat(case["kernel"], z, z, variance, ls_arg(case, ls), form)
    return float(np.median(kuf / variance)), float(np.linalg.cond(kuu + 1e-6 * np.eye(z.shape[0])))


def make_handle(lib, case, x, y):
    h = C.c_void_p()
    check(lib.gprx_create(0, x.shape[0], x.shape[1], case["m"], okn.KERNEL_IDS[case["kernel"]], int(case["ard"]), C.byref(h)))
    check(lib.gprx_set_data(h, ptr(x), ptr(y), y.shape[1]), h)
    check(lib.gprx_set_distance_form(h, case["form"]), h)
    return h


def batch(lib, h, units, thetas, zs, mask):
    cells, nt = thetas.shape
    losses, grads = np.zeros(cells), np.zeros((cells, nt + zs[0].size))
    check(lib.gprx_objective_batch(h, cells, ptr(units), ptr(thetas), ptr(zs), mask, ptr(losses), ptr(grads)), h)
    return losses, grads


def blockwise_error(got, ref, nt):
    """Largest |got - ref| of the hyperparameter block and of the Z block, each relative to its block's largest |ref|."""
    return (float(np.max(np.abs(got[:nt] - ref[:nt])) / np.max(np.abs(ref[:nt]))),
            float(np.max(np.abs(got[nt:] - ref[nt:])) / np.max(np.abs(ref[nt:]))))


# ---- 1. parity sweep ------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_fused_variant_against_the_oracle(lib, case):
    """One (kernel, class, NP) instantiation of the five fused launches: loss 1e-9 and gradient blocks 1e-7 of their largest entry for
    every cell, cells 0 and -1 equal to single gprx_objective calls bit for bit, the launch sequence ("sgpr_fused" = 0) within rounding
    but not bit-equal (the fused kernels ran), and predict after a single objective within 1e-8."""
    x, y, thetas, zs, units, variance, ls, noise = draw_inputs(case)
    cells, nt = thetas.shape
    kernel, d, m = case["kernel"], case["d"], case["m"]
    conds = []
    for c in range(cells):
        med, cond = preconditions(case, x, zs[c], variance[c], ls[c])
        assert 0.02 <= med <= 0.95, (c, med)
        conds.append(cond)
    if case["cond_scaled"]:
        assert max(conds) > 1e6  # (else the case does not need the scaled bound)
    else:
        assert max(conds) <= 1e6, conds
    h = make_handle(lib, case, x, y)
    try:
        losses, grads = batch(lib, h, units, thetas, zs, ALL)
        last_chunk = 0.0
        for c in range(cells):
            ref_loss, ref = ref_eval(case, x, y[:, units[c]], zs[c], thetas[c])
            loss_tol, tol = NONSMOOTH_EXPANDED_TOL if case["form"] == 1 and kernel in EXPANDED_ISO else (1e-9, 1e-7)
            tol *= max(1.0, conds[c] / 1e6)
            assert abs(losses[c] - ref_loss) <= loss_tol * abs(ref_loss), (c, losses[c], ref_loss)
            eh, ez = blockwise_error(grads[c], ref, nt)
            assert eh <= tol and ez <= tol, (c, eh, ez, conds[c])
            if case["ard"] and d > SF_DK:
                last_chunk = max(last_chunk, np.max(np.abs(ref[1 + SF_DK * ((d - 1) // SF_DK): 1 + d])) / np.max(np.abs(ref[:nt])))
        if case["ard"] and d > SF_DK:  # the last chunk of 16 dimensions contributes to what was compared
            assert last_chunk >= 1e-3, last_chunk
        def single(c):  # (every array passed by address stays bound for the call: ptr() does not keep it alive)
            th, zc = np.ascontiguousarray(thetas[c]), np.ascontiguousarray(zs[c])
            loss, g1 = C.c_double(), np.zeros(nt + m * d)
            check(lib.gprx_objective(h, int(units[c]), ptr(th), ptr(zc), ALL, C.byref(loss), ptr(g1)), h)
            return loss.value, g1

        for c in (0, cells - 1):
            l1, g1 = single(c)
            assert l1 == losses[c] and np.array_equal(g1, grads[c]), c
        check(lib.gprx_set_handle_tuning(h, b"sgpr_fused", 0), h)
        l0, g0 = batch(lib, h, units, thetas, zs, ALL)
        check(lib.gprx_set_handle_tuning(h, b"sgpr_fused", 1), h)
        scale = max(1.0, max(conds) / 1e6) if case["cond_scaled"] else 1.0
        assert np.max(np.abs(losses - l0) / np.abs(l0)) <= 1e-11
        assert np.max(np.abs(grads - g0) / np.max(np.abs(g0), axis=1, keepdims=True)) <= 1e-8 * scale
        assert not (np.array_equal(losses, l0) and np.array_equal(grads, g0))
        # predict from the factorisation a single objective leaves behind
        c = cells - 1
        single(c)
        xs = np.ascontiguousarray(np.random.default_rng(case["seed"]).standard_normal((200, d)))
        mean, var = np.zeros(200), np.zeros(200)
        check(lib.gprx_predict(h, ptr(xs), 200, ptr(mean), ptr(var), 1), h)
        rm, rv = osg.predict(kernel, x, y[:, units[c]], zs[c], float(variance[c]), ls_arg(case, ls[c]), float(noise[c]), xs, True,
                             form="expanded" if case["form"] else "direct")
        assert np.max(np.abs(mean - rm)) <= 1e-8 * np.max(np.abs(rm))
        assert np.max(np.abs(var - rv) / rv) <= 1e-8
    finally:
        lib.gprx_destroy(h)


# ---- 2. trainable masks on the fused path ---------------------------------------------------------------------------------------

MASK_CASES = [dict(id="Matern32-ard-np8-d14", kernel="Matern32", cls="ard", d=14, m=33, n=300, ard=True, form=0, cells=3, seed=101),
              dict(id="Exponential-expanded-np0-d33", kernel="Exponential", cls="expanded", d=33, m=20, n=257, ard=False, form=1, cells=3, seed=102)]


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [1, 2, 4, 8, 7, 14])
@pytest.mark.parametrize("case", MASK_CASES, ids=[c["id"] for c in MASK_CASES])
def test_fused_variant_with_a_trainable_mask(lib, case, mask):
    """The loss sums the priors of the trainable parameters only (the oracle with the same mask), frozen gradient entries are exactly
    0.0, trainable ones agree within 1e-7 of their block's largest entry."""
    x, y, thetas, zs, units, *_ = draw_inputs(case)
    cells, nt = thetas.shape
    flags = tuple(bool(mask & b) for b in (_lib.TRAIN_VARIANCE, _lib.TRAIN_LENGTHSCALE, _lib.TRAIN_NOISE, _lib.TRAIN_Z))
    trainable = np.concatenate([[flags[0]], np.full(nt - 2, flags[1]), [flags[2]], np.full(zs[0].size, flags[3])])
    h = make_handle(lib, case, x, y)
    try:
        losses, grads = batch(lib, h, units, thetas, zs, mask)
        for c in range(cells):
            ref_loss, ref = ref_eval(case, x, y[:, units[c]], zs[c], thetas[c], flags)
            assert abs(losses[c] - ref_loss) <= 1e-9 * abs(ref_loss), (c, losses[c], ref_loss)
            assert np.all(grads[c][~trainable] == 0.0)
            for blk in (slice(0, nt), slice(nt, None)):
                t = trainable[blk]
                if t.any():
                    got, want = grads[c][blk][t], ref[blk][t]
                    assert np.max(np.abs(got - want)) <= 1e-7 * np.max(np.abs(want)), (c, blk)
    finally:
        lib.gprx_destroy(h)


# ---- 3. resident Adam, bit for bit ----------------------------------------------------------------------------------------------


def adam_models(case, n=160, cells=3, at_optimum=1):
    """An Engine in the case's distance form and ``cells`` models on it; the first ``at_optimum`` models start at an L-BFGS optimum (under
    the case's mask), so they stop early, the others start at drawn values and keep going.  Returns (engine, factory) -- factory() builds a fresh set of
    models in the same state."""
    from scipy.optimize import minimize

    from gpras_amd.engine import Engine
    from gpras_amd.model import GPModel

    d, m = case["d"], case["m"]
    x, y, _ = make_regression(n, d, n_outputs=cells, n_test=0, config=32, unit=case["seed"])
    rng = np.random.default_rng(700 + case["seed"])
    eng = Engine(case["kernel"], x, y, m, ard=case["ard"], distance_form="expanded" if case["form"] else "difference")
    nl = d if case["ard"] else 1
    states = []
    for c in range(cells):
        z = x[rng.choice(n, size=m, replace=False)] + 1e-3 * rng.standard_normal((m, d))
        states.append((rng.uniform(0.5, 2.0), np.sqrt(d) * rng.uniform(0.6, 1.6, nl), 10.0 ** rng.uniform(-2.0, -0.5), z))

    def build(state_list):
        out = []
        for c, (v, l, s, z) in enumerate(state_list):
            mod = GPModel(eng, c, z, v, l, s)
            mod.mask = case["mask"]
            out.append(mod)
        return out

    raw = []
    for mod in build(states[:at_optimum]):
        def fun(vec, mod=mod):
            mod.set_vector(vec)
            return mod.loss_and_grad()

        for mask in (ALL, case["mask"]):  # (all variables first: Z alone under drawn hyperparameters stalls far from an optimum)
            mod.mask = mask
            res = minimize(fun, mod.get_vector(), jac=True, method="L-BFGS-B", options={"maxiter": 2000, "ftol": 1e-15, "gtol": 1e-10})
            mod.set_vector(res.x)
        raw.append((mod.w_var, mod.w_len.copy(), mod.w_noise, mod.Z.copy()))

    def factory():
        models = build(states)
        for mod, (wv, wl, wn, z) in zip(models, raw):
            mod.w_var, mod.w_len, mod.w_noise, mod.Z = wv, wl.copy(), wn, z.copy()
        for mod in models:
            mod.n_evals = 0
        return models

    return eng, factory


@pytest.mark.gpu
@pytest.mark.parametrize("case", ADAM_CASES, ids=[c["id"] for c in ADAM_CASES])
def test_resident_adam_equals_the_python_loop(lib, case):
    """sf_adam_prep_kernel<KID, FORM, ISO> for every (kernel, class): 60 steps -- two windows of 25 stop-flag checks and a tail -- of the
    library's resident loop give the variables, Z and evaluation counts of optimizers._adam_packed over host evaluations, bit for bit;
    the cell started at an optimum stops early beside cells that keep going."""
    from gpras_amd import optimizers

    eng, factory = adam_models(case)
    try:
        a, b = factory(), factory()
        optimizers._optimize_adam_many(a, 60)  # library loop (resident on the device: M <= 64)
        packed = optimizers._PackedBatch(b)
        optimizers._adam_packed(packed, np.stack([mod.get_vector() for mod in b]), 60, None)  # Python loop, batched host evaluations
        evals = [mod.n_evals for mod in a]
        assert evals == [mod.n_evals for mod in b]
        assert evals[0] < 60 and max(evals[1:]) == 60, evals
        for ma, mb in zip(a, b):
            assert np.array_equal(ma.theta(), mb.theta()) and np.array_equal(ma.Z, mb.Z)
        assert not np.array_equal(a[1].get_vector(), factory()[1].get_vector())  # (the loop moved the variables)
    finally:
        eng.close()


# ---- 4. the alpha table of the resident loop, and its failure contract ---------------------------------------------------------


@pytest.mark.gpu
def test_resident_adam_until_the_early_stop_does_not_size_by_max_iter(lib):
    """max_iter = 2^31 - 1 ("until the early stop"): the alpha table is one window of stop-flag checks, not max_iter entries (16 GB on
    the host and the device before).  Same variables and evaluation counts as max_iter = 5000, bit for bit, in comparable time."""
    case = dict(kernel="Matern52", d=4, m=16, ard=False, form=0, mask=15, seed=200)
    eng, factory = adam_models(case, n=200, cells=2, at_optimum=2)
    try:
        def run(max_iter):
            models = factory()
            thetas = np.stack([mod.theta() for mod in models])
            zs = np.stack([mod.Z for mod in models])
            t0 = time.perf_counter()
            th, z, ev, _ = eng.adam_batch(np.arange(2, dtype=np.int32), thetas, case["mask"], max_iter, zs=zs)
            return th, z, ev, time.perf_counter() - t0

        run(5000)  # (warm: the first call captures and compiles nothing later calls pay for)
        th_s, z_s, ev_s, t_s = run(5000)
        th_l, z_l, ev_l, t_l = run(2**31 - 1)
        assert np.array_equal(ev_s, ev_l) and (ev_s < 5000).all() and (ev_s > 0).all()
        assert np.array_equal(th_s, th_l) and np.array_equal(z_s, z_l)
        assert t_l <= 2.0 * t_s + 1.0, (t_s, t_l)
    finally:
        eng.close()
