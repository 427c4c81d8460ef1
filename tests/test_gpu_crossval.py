"""Held-out row ranges of the fused sparse evaluation (gprx_objective_batch_held, gprx_adam_batch_held, gprx_adadelta_batch_held,
gprx_predict_batch_held) and the event-fold cross-validation on top of them (gpras_amd.crossval).

Cases, holds and references: tests/crossval_cases.py; tests/test_crossval.py (no GPU) checks that the cases are well posed on every
cell's kept rows and that every hold moves the loss by far more than the tolerances here.  The reference of every comparison is the
oracle on ``x[keep], y[keep]``; the tolerances are those of test_gpu_sparse_variants.
"""

import ctypes as C

import numpy as np
import pytest

import crossval_cases as cc
from gpras_amd import _lib
from gpras_amd._lib import check, ptr
from oracle import kernels as okn
from oracle import sgpr as osg

ALL = _lib.TRAIN_VARIANCE | _lib.TRAIN_LENGTHSCALE | _lib.TRAIN_NOISE | _lib.TRAIN_Z
Z_ONLY = _lib.TRAIN_Z  # stage 1 of two-stage: no priors
LO = np.ascontiguousarray([h[0] for h in cc.HOLDS], dtype=np.int64)
HI = np.ascontiguousarray([h[1] for h in cc.HOLDS], dtype=np.int64)
XS_POINTS = 200


def make_handle(lib, case, x, y, m=None):
    h = C.c_void_p()
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    check(lib.gprx_create(0, x.shape[0], x.shape[1], case["m"] if m is None else m, okn.KERNEL_IDS[case["kernel"]], int(case["ard"]), C.byref(h)))
    check(lib.gprx_set_data(h, ptr(x), ptr(y), y.shape[1]), h)
    check(lib.gprx_set_distance_form(h, case["form"]), h)
    return h


def objective(lib, h, units, thetas, zs, mask, lo=None, hi=None):
    """gprx_objective_batch, or its held form when ranges are given.  Returns (losses, grads)."""
    units, thetas, zs = np.ascontiguousarray(units, dtype=np.int32), np.ascontiguousarray(thetas), np.ascontiguousarray(zs)
    cells, nt = thetas.shape
    losses, grads = np.zeros(cells), np.zeros((cells, nt + zs[0].size))
    if lo is None:
        check(lib.gprx_objective_batch(h, cells, ptr(units), ptr(thetas), ptr(zs), mask, ptr(losses), ptr(grads)), h)
    else:
        lo, hi = np.ascontiguousarray(lo, dtype=np.int64), np.ascontiguousarray(hi, dtype=np.int64)
        check(lib.gprx_objective_batch_held(h, cells, ptr(units), ptr(thetas), ptr(zs), mask, ptr(losses), ptr(grads), ptr(lo), ptr(hi)), h)
    return losses, grads


def predict(lib, h, units, thetas, zs, xs, lo=None, hi=None):
    units, thetas, zs = np.ascontiguousarray(units, dtype=np.int32), np.ascontiguousarray(thetas), np.ascontiguousarray(zs)
    cells = thetas.shape[0]
    means, variances = np.zeros((cells, xs.shape[0])), np.zeros((cells, xs.shape[0]))
    if lo is None:
        check(lib.gprx_predict_batch(h, cells, ptr(units), ptr(thetas), ptr(zs), ptr(xs), xs.shape[0], ptr(means), ptr(variances), 1), h)
    else:
        lo, hi = np.ascontiguousarray(lo, dtype=np.int64), np.ascontiguousarray(hi, dtype=np.int64)
        check(lib.gprx_predict_batch_held(h, cells, ptr(units), ptr(thetas), ptr(zs), ptr(xs), xs.shape[0], ptr(means), ptr(variances), 1,
                                          ptr(lo), ptr(hi)), h)
    return means, variances


def points_for(case):
    return np.ascontiguousarray(np.random.default_rng(case["seed"]).standard_normal((XS_POINTS, case["d"])))


def tolerances(case):
    return cc.NONSMOOTH_EXPANDED_TOL if case["form"] == 1 and case["kernel"] in cc.EXPANDED_ISO else (1e-9, 1e-7)


# ---- 1. parity per evaluation ---------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [ALL, Z_ONLY], ids=["mask15", "mask8"])
@pytest.mark.parametrize("case", cc.CASES, ids=[c["id"] for c in cc.CASES])
def test_held_objective_against_the_oracle_on_the_kept_rows(lib, case, mask):
    """Loss within 1e-9 and each gradient block within 1e-7 of its largest entry (the nonsmooth expanded class: its own bound), for all
    eight holds in one batch; with mask 8 the hyperparameter block is exactly zero and the loss carries no prior."""
    x, y, thetas, zs, units, *_ = cc.draw_inputs(case)
    nt = thetas.shape[1]
    loss_tol, tol = tolerances(case)
    h = make_handle(lib, case, x, y)
    try:
        losses, grads = objective(lib, h, units, thetas, zs, mask, LO, HI)
        for c in range(cc.CELLS):
            ref_loss, ref = cc.ref_cell(case, c, mask)
            print(case["id"], mask, c, abs(losses[c] - ref_loss) / abs(ref_loss))
            assert abs(losses[c] - ref_loss) <= loss_tol * abs(ref_loss), (c, losses[c], ref_loss)
            if mask == ALL:
                eh, ez = cc.blockwise_error(grads[c], ref, nt)
                print("   blocks", eh, ez)
                assert eh <= tol and ez <= tol, (c, eh, ez)
            else:
                assert np.all(grads[c][:nt] == 0.0) and np.all(ref[:nt] == 0.0)
                ez = float(np.max(np.abs(grads[c][nt:] - ref[nt:])) / np.max(np.abs(ref[nt:])))
                print("   Z block", ez)
                assert ez <= tol, (c, ez)
    finally:
        lib.gprx_destroy(h)


@pytest.mark.gpu
@pytest.mark.parametrize("case", cc.CASES, ids=[c["id"] for c in cc.CASES])
def test_held_predict_against_the_oracle_on_the_kept_rows(lib, case):
    """gprx_predict_batch_held at 200 test points against oracle.sgpr.predict on every cell's kept rows, within 1e-8."""
    x, y, thetas, zs, units, variance, ls, noise = cc.draw_inputs(case)
    xs = points_for(case)
    h = make_handle(lib, case, x, y)
    try:
        means, variances = predict(lib, h, units, thetas, zs, xs, LO, HI)
        for c, hold in enumerate(cc.HOLDS):
            keep = cc.keep_rows(hold)
            rm, rv = osg.predict(case["kernel"], x[keep], y[keep, units[c]], zs[c], float(variance[c]), cc.ls_arg(case, ls[c]), float(noise[c]), xs,
                                 True, form=cc.form_name(case))
            em, ev = np.max(np.abs(means[c] - rm)) / np.max(np.abs(rm)), np.max(np.abs(variances[c] - rv) / rv)
            print(case["id"], c, em, ev)
            assert em <= 1e-8 and ev <= 1e-8, (c, em, ev)
    finally:
        lib.gprx_destroy(h)


# ---- 2. bits --------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("case", cc.CASES, ids=[c["id"] for c in cc.CASES])
def test_held_bits(lib, case):
    """(a) the cell with the empty hold, and a whole call whose holds are all empty, have the bits of gprx_objective_batch; (b) the cell
    that holds the suffix [563, 600) out has the bits of the same cell on a handle created with the first 563 rows -- loss, gradient and
    predictions; (c) every held cell alone has the bits it has inside the batch of eight."""
    x, y, thetas, zs, units, *_ = cc.draw_inputs(case)
    xs = points_for(case)
    h = make_handle(lib, case, x, y)
    h563 = make_handle(lib, case, x[:563], y[:563])
    try:
        losses, grads = objective(lib, h, units, thetas, zs, ALL, LO, HI)
        plain_l, plain_g = objective(lib, h, units, thetas, zs, ALL)
        e = cc.EMPTY_CELL
        assert losses[e] == plain_l[e] and np.array_equal(grads[e], plain_g[e])
        assert not np.array_equal(losses[:e], plain_l[:e])  # (the other cells did hold rows out)
        zero = np.zeros(cc.CELLS, dtype=np.int64)
        for lo0 in (zero, zero + 300):
            el, eg = objective(lib, h, units, thetas, zs, ALL, lo0, lo0)
            assert np.array_equal(el, plain_l) and np.array_equal(eg, plain_g)
        # (b)
        s = cc.SUFFIX_CELL
        one = slice(s, s + 1)
        tl, tg = objective(lib, h563, units[one], thetas[one], zs[one], ALL)
        assert tl[0] == losses[s] and np.array_equal(tg[0], grads[s])
        hm, hv = predict(lib, h, units, thetas, zs, xs, LO, HI)
        tm, tv = predict(lib, h563, units[one], thetas[one], zs[one], xs)
        assert np.array_equal(tm[0], hm[s]) and np.array_equal(tv[0], hv[s])
        # (c)
        for c in range(cc.CELLS):
            cl, cg = objective(lib, h, units[c:c + 1], thetas[c:c + 1], zs[c:c + 1], ALL, LO[c:c + 1], HI[c:c + 1])
            assert cl[0] == losses[c] and np.array_equal(cg[0], grads[c]), c
            if c in (0, 3, s):
                cm, cv = predict(lib, h, units[c:c + 1], thetas[c:c + 1], zs[c:c + 1], xs, LO[c:c + 1], HI[c:c + 1])
                assert np.array_equal(cm[0], hm[c]) and np.array_equal(cv[0], hv[c]), c
    finally:
        lib.gprx_destroy(h)
        lib.gprx_destroy(h563)


# ---- 3. resident loops ----------------------------------------------------------------------------------------------------------


def run_loop(lib, h, kind, units, thetas, zs, mask, steps, lo=None, hi=None):
    """gprx_adam_batch / gprx_adadelta_batch (or their held forms) on copies.  Returns (theta, z, n_evals, route)."""
    units = np.ascontiguousarray(units, dtype=np.int32)
    th, z = np.array(thetas, dtype=np.float64, order="C"), np.array(zs, dtype=np.float64, order="C")
    cells = th.shape[0]
    n_evals, batches, losses = np.zeros(cells, dtype=np.int32), C.c_int(), np.zeros(cells)
    held = lo is not None
    if held:
        lo, hi = np.ascontiguousarray(lo, dtype=np.int64), np.ascontiguousarray(hi, dtype=np.int64)
    if kind == "adam":
        if held:
            check(lib.gprx_adam_batch_held(h, cells, ptr(units), ptr(th), ptr(z), mask, steps, ptr(n_evals), C.byref(batches), ptr(lo), ptr(hi)), h)
        else:
            check(lib.gprx_adam_batch(h, cells, ptr(units), ptr(th), ptr(z), mask, steps, ptr(n_evals), C.byref(batches)), h)
    else:
        if held:
            check(lib.gprx_adadelta_batch_held(h, cells, ptr(units), ptr(th), ptr(z), mask, steps, ptr(losses), ptr(n_evals), C.byref(batches),
                                               ptr(lo), ptr(hi)), h)
        else:
            check(lib.gprx_adadelta_batch(h, cells, ptr(units), ptr(th), ptr(z), mask, steps, ptr(losses), ptr(n_evals), C.byref(batches)), h)
    route, waits = C.c_int(), C.c_int()
    check(lib.gprx_last_optimizer_route(h, C.byref(route), C.byref(waits)), h)
    return th, z, n_evals, route.value


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [ALL, Z_ONLY], ids=["mask15", "mask8"])
@pytest.mark.parametrize("kind, steps", [("adam", 30), ("adadelta", 10)])
@pytest.mark.parametrize("case", cc.RESIDENT_CASES, ids=[c["id"] for c in cc.RESIDENT_CASES])
def test_held_resident_loops(lib, case, kind, steps, mask):
    """Eight cells with all eight holds: the resident loop (route 1) gives the variables, Z and evaluation counts of the host-stepped
    loop ("sgpr_resident" = 0, route 0) bit for bit; the suffix cell gives those of the same loop on the handle of the first 563 rows;
    split into two groups of cells on two streams, every cell keeps its own hold and its bits."""
    x, y, thetas, zs, units, *_ = cc.draw_inputs(case)
    h = make_handle(lib, case, x, y)
    h563 = make_handle(lib, case, x[:563], y[:563])
    try:
        th, z, ev, route = run_loop(lib, h, kind, units, thetas, zs, mask, steps, LO, HI)
        assert route == 1
        assert np.all(ev == steps)
        assert not np.array_equal(z if mask == Z_ONLY else th, zs if mask == Z_ONLY else thetas)  # (the loop moved the variables)
        check(lib.gprx_set_handle_tuning(h, b"sgpr_resident", 0), h)
        th0, z0, ev0, route0 = run_loop(lib, h, kind, units, thetas, zs, mask, steps, LO, HI)
        check(lib.gprx_set_handle_tuning(h, b"sgpr_resident", 1), h)
        assert route0 == 0
        assert np.array_equal(th, th0) and np.array_equal(z, z0) and np.array_equal(ev, ev0)
        # a loop without holds ends elsewhere for every cell but the empty one
        thp, zp, _, _ = run_loop(lib, h, kind, units, thetas, zs, mask, steps)
        e = cc.EMPTY_CELL
        assert np.array_equal(thp[e], th[e]) and np.array_equal(zp[e], z[e])
        assert all(not (np.array_equal(thp[c], th[c]) and np.array_equal(zp[c], z[c])) for c in range(cc.CELLS) if c != e)
        s = cc.SUFFIX_CELL
        one = slice(s, s + 1)
        tht, zt, evt, routet = run_loop(lib, h563, kind, units[one], thetas[one], zs[one], mask, steps)
        assert routet == 1 and np.array_equal(tht[0], th[s]) and np.array_equal(zt[0], z[s]) and evt[0] == ev[s]
        try:
            check(lib.gprx_set_tuning(b"sgpr_groups_from", 1))  # two groups whatever the size
            thg, zg, evg, routeg = run_loop(lib, h, kind, units, thetas, zs, mask, steps, LO, HI)
        finally:
            lib.gprx_set_tuning(b"sgpr_groups_from", 17)
        assert routeg == 1 and np.array_equal(thg, th) and np.array_equal(zg, z) and np.array_equal(evg, ev)
    finally:
        lib.gprx_destroy(h)
        lib.gprx_destroy(h563)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
def test_held_forms_refuse_what_they_do_not_serve(lib):
    """GPRX_EINVAL with the reason in the message: a handle with M = 70, an exact handle, lo > hi, hi > n, a hold of all rows -- from all
    four entry points."""
    case = cc.CASES[0]
    x, y, thetas, zs, units, *_ = cc.draw_inputs(case)
    xs = points_for(case)
    n = cc.N

    def calls(h, m, lo, hi):
        """The four held entry points on two cells; returns [(rc, message)]."""
        u = np.ascontiguousarray(units[:2])
        th, z = np.array(thetas[:2]), np.zeros((2, max(m, 1), case["d"])) + np.array(x[: max(m, 1)])
        lo, hi = np.ascontiguousarray(lo, dtype=np.int64), np.ascontiguousarray(hi, dtype=np.int64)
        zp = ptr(z) if m else None
        losses, grads = np.zeros(2), np.zeros((2, th.shape[1] + m * case["d"]))
        ev, b = np.zeros(2, dtype=np.int32), C.c_int()
        mu, vv = np.zeros((2, XS_POINTS)), np.zeros((2, XS_POINTS))
        out = []
        for rc in (
            lambda: lib.gprx_objective_batch_held(h, 2, ptr(u), ptr(th), zp, ALL, ptr(losses), ptr(grads), ptr(lo), ptr(hi)),
            lambda: lib.gprx_adam_batch_held(h, 2, ptr(u), ptr(th), zp, ALL, 3, ptr(ev), C.byref(b), ptr(lo), ptr(hi)),
            lambda: lib.gprx_adadelta_batch_held(h, 2, ptr(u), ptr(th), zp, ALL, 3, ptr(losses), ptr(ev), C.byref(b), ptr(lo), ptr(hi)),
            lambda: lib.gprx_predict_batch_held(h, 2, ptr(u), ptr(th), zp, ptr(xs), XS_POINTS, ptr(mu), ptr(vv), 1, ptr(lo), ptr(hi)),
        ):
            out.append((rc(), _lib.last_error(h)))
        return out

    for m, lo, hi, why in [
        (70, [0, 10], [5, 20], "64 inducing points"),
        (0, [0, 10], [5, 20], "exact model"),
        (case["m"], [0, 30], [5, 20], "hold_lo 30 > hold_hi 20"),
        (case["m"], [0, 10], [5, n + 1], "outside [0, 600]"),
        (case["m"], [0, -1], [5, 4], "outside [0, 600]"),
        (case["m"], [0, 0], [5, n], "keeps no row"),
    ]:
        h = make_handle(lib, case, x, y, m=m)
        try:
            for rc, msg in calls(h, m, lo, hi):
                assert rc == _lib.GPRX_EINVAL and why in msg, (m, lo, hi, rc, msg)
        finally:
            lib.gprx_destroy(h)
    # "sgpr_fused" = 0: the general launch sequence holds no rows out
    h = make_handle(lib, case, x, y)
    try:
        check(lib.gprx_set_handle_tuning(h, b"sgpr_fused", 0), h)
        for rc, msg in calls(h, case["m"], [0, 10], [5, 20]):
            assert rc == _lib.GPRX_EINVAL and "sgpr_fused" in msg, (rc, msg)
    finally:
        lib.gprx_destroy(h)


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------

E2E = dict(n=600, k=3, d=8, m=20, kernel="RBF", events=[(100 * e, 100 * (e + 1)) for e in range(6)])


@pytest.fixture(scope="module")
def e2e_data():
    from gpras_amd.synth import make_regression

    x, y, _ = make_regression(E2E["n"], E2E["d"], n_outputs=E2E["k"], n_test=0, config=31, unit=7)
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def _close(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.gpu
def test_cross_validate_routes_agree_at_the_initial_state(lib, e2e_data):
    """two-stage at max_iter = 0: no optimiser step, both routes predict from every fold's initial state (k-means on the fold's rows,
    lengthscale mean|x[keep]|, variance 1, noise 1) -- mean and variance within 1e-8."""
    from gpras_amd.crossval import cross_validate

    x, y = e2e_data
    held = cross_validate(E2E["kernel"], x, y, E2E["events"], E2E["m"], optimization_method="two-stage", route="held", max_iter=0)
    engines = cross_validate(E2E["kernel"], x, y, E2E["events"], E2E["m"], optimization_method="two-stage", route="engines", max_iter=0)
    assert held.route == "held" and engines.route == "engines"
    assert held.mean.shape == held.var.shape == (E2E["n"], E2E["k"]) and np.isfinite(held.mean).all() and np.isfinite(engines.mean).all()
    assert np.array_equal(held.Z, engines.Z) and np.array_equal(held.thetas, engines.thetas)  # the same initial state
    em, ev = _close(held.mean, engines.mean), float(np.max(np.abs(held.var - engines.var) / engines.var))
    print("routes at the initial state", em, ev)
    assert em <= 1e-8 and ev <= 1e-8
    assert _close(held.first_loss, engines.first_loss) <= 1e-9
    rmse, nlpd = held.scores(y)
    assert rmse.shape == nlpd.shape == (6, E2E["k"]) and np.isfinite(rmse).all() and np.isfinite(nlpd).all()


@pytest.mark.gpu
def test_cross_validate_held_equals_the_cells_driven_by_hand(lib, e2e_data):
    """two-stage at max_iter = 5 through cross_validate(route="auto") against the same 18 fold cells through Engine.adam_batch(holds=...)
    (Z, then the hyperparameters) and Engine.predict_batch(holds=...): bit for bit.  Every fold's last loss is finite and no larger
    than its first."""
    from gpras_amd.crossval import cross_validate, fold_cells
    from gpras_amd.engine import Engine
    from gpras_amd.gpr import GPRAS
    from gpras_amd.model import GPModel

    x, y = e2e_data
    n, k, m = E2E["n"], E2E["k"], E2E["m"]
    res = cross_validate(E2E["kernel"], x, y, E2E["events"], m, optimization_method="two-stage", max_iter=5)
    assert res.route == "held" and res.ranges == E2E["events"]
    assert res.thetas.shape == (6, k, 3) and res.Z.shape == (6, k, m, E2E["d"]) and res.n_evals.shape == (6, k)
    assert np.isfinite(res.last_loss).all() and np.all(res.last_loss <= res.first_loss), (res.first_loss, res.last_loss)
    assert set(res.last_timings_ms) >= {"fit_ms", "predict_ms", "total_ms"}
    helper = GPRAS(E2E["kernel"])
    eng = Engine(E2E["kernel"], x, y, m)
    try:
        cells = fold_cells(6, k)
        holds = [E2E["events"][e] for e, _ in cells]
        units = np.array([mode for _, mode in cells], dtype=np.int32)
        z0, th0 = [], []
        for e, mode in cells:
            a, b = E2E["events"][e]
            keep = np.r_[0:a, b:n]
            zi = helper._create_inducing(x[keep], m, "kmeans")
            z0.append(zi)
            th0.append(GPModel(eng, mode, zi, 1.0, np.mean(abs(x[keep])), 1.0).theta())
        th, zs, _, _ = eng.adam_batch(units, np.stack(th0), Z_ONLY, 5, zs=np.stack(z0), holds=holds)
        assert eng.last_optimizer_route()[0] == 1
        th, zs, _, _ = eng.adam_batch(units, th, ALL & ~Z_ONLY, 5, zs=zs, holds=holds)
        assert np.array_equal(th.reshape(6, k, -1), res.thetas) and np.array_equal(zs.reshape(6, k, m, -1), res.Z)
        for e, (a, b) in enumerate(E2E["events"]):
            sl = slice(e * k, (e + 1) * k)
            mu, vv = eng.predict_batch(units[sl], th[sl], x[a:b], zs=zs[sl], holds=holds[sl])
            assert np.array_equal(mu.T, res.mean[a:b]) and np.array_equal(vv.T, res.var[a:b]), e
    finally:
        eng.close()


@pytest.mark.gpu
def test_cross_validate_from_fitted_parameters_is_leave_event_out(lib, e2e_data):
    """adam at max_iter = 0 with the fitted parameters assigned to every fold: the held predictions are the model on the other rows at the
    same parameters, which is what leave_event_out(route="refactor") computes by definition -- within 1e-8."""
    from gpras_amd.gpr import GPRAS

    x, y = e2e_data
    g = GPRAS(E2E["kernel"])
    g.fit(x, y, E2E["m"], optimization_method="two-stage", max_iter=5)
    try:
        assert g.fit_args["n_inducing"] == E2E["m"] and g.fit_args["max_iter"] == 5
        res = g.cross_validate(E2E["events"], optimization_method="adam", max_iter=0, start=g, route="held")
        assert res.route == "held" and np.all(res.n_evals == 0)
        for e in range(6):
            assert np.array_equal(res.thetas[e], np.stack([mod.theta() for mod in g.models]))
        mean, var = g.leave_event_out(E2E["events"], route="refactor")
        em, ev = _close(res.mean, mean), float(np.max(np.abs(res.var - var) / var))
        print("held against refactor", em, ev)
        assert em <= 1e-8 and ev <= 1e-8
    finally:
        for eng in g.engines:
            eng.close()
