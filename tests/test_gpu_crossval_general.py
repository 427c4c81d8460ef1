"""Held-out row ranges in the GENERAL sparse launch sequence (handle tuning key "held_general" = 1: M > 64, and M <= 64 with
"sgpr_fused" = 0) through gprx_objective_batch_held, gprx_adam_batch_held, gprx_adadelta_batch_held and gprx_predict_batch_held, and
cross_validate(route="held_general") on top of them.

Cases, holds and references: tests/crossval_general_cases.py; tests/test_crossval_general.py (no GPU) checks that the cases are well
posed on every cell's kept rows and that every hold moves the loss by far more than the tolerances here.  The reference of every parity
comparison is the oracle on ``x[keep], y[keep]``; the tolerances are those of test_gpu_sparse_variants.  Every test sets "held_general"
= 1 first.  The suffix property of the fused route (a suffix-held cell has the bits of a handle on the short data) is NOT promised here
 and not tested.
"""

import ctypes as C

import numpy as np
import pytest
from test_gpu_crossval import E2E, make_handle, objective, points_for, predict, run_loop

import crossval_cases as cc
import crossval_general_cases as gc
from gpras_amd import _lib
from gpras_amd._lib import check, ptr
from oracle import sgpr as osg
from oracle import transforms as otr

ALL = _lib.TRAIN_VARIANCE | _lib.TRAIN_LENGTHSCALE | _lib.TRAIN_NOISE | _lib.TRAIN_Z
Z_ONLY = _lib.TRAIN_Z


def open_handle(lib, case, x, y):
    """A handle of the case on the general launch sequence with "held_general" = 1."""
    h = make_handle(lib, case, x, y)
    if case.get("unfused"):
        check(lib.gprx_set_handle_tuning(h, b"sgpr_fused", 0), h)
    check(lib.gprx_set_handle_tuning(h, b"held_general", 1), h)
    return h


# ---- 1. parity per evaluation ---------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [ALL, Z_ONLY], ids=["mask15", "mask8"])
@pytest.mark.parametrize("case", gc.CASES, ids=[c["id"] for c in gc.CASES])
def test_held_general_objective_against_the_oracle_on_the_kept_rows(lib, case, mask):
    """Loss within 1e-9 and each gradient block within 1e-7 of its largest entry (the nonsmooth expanded class: its own bound), for all
    eight holds in one batch; with mask 8 the hyperparameter block is exactly zero.  The same call three times -- eager launches, the
    capture, the replay -- gives the same bits."""
    x, y, thetas, zs, units, *_ = cc.draw_inputs(case)
    nt = thetas.shape[1]
    lo, hi = gc.hold_arrays(case)
    loss_tol, tol = gc.tolerances(case)
    h = open_handle(lib, case, x, y)
    try:
        losses, grads = objective(lib, h, units, thetas, zs, mask, lo, hi)
        for which in ("captured", "replayed"):
            l2, g2 = objective(lib, h, units, thetas, zs, mask, lo, hi)
            assert np.array_equal(l2, losses) and np.array_equal(g2, grads), which
        for c in range(gc.CELLS):
            ref_loss, ref = gc.ref_cell(case, c, mask)
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
@pytest.mark.parametrize("case", gc.CASES, ids=[c["id"] for c in gc.CASES])
def test_held_general_predict_against_the_oracle_on_the_kept_rows(lib, case):
    """gprx_predict_batch_held at 200 test points against oracle.sgpr.predict on every cell's kept rows, within 1e-8."""
    x, y, thetas, zs, units, variance, ls, noise = cc.draw_inputs(case)
    xs = points_for(case)
    lo, hi = gc.hold_arrays(case)
    h = open_handle(lib, case, x, y)
    try:
        means, variances = predict(lib, h, units, thetas, zs, xs, lo, hi)
        for c in range(gc.CELLS):
            keep = gc.keep_rows(case, c)
            rm, rv = osg.predict(case["kernel"], x[keep], y[keep, units[c]], zs[c], float(variance[c]), cc.ls_arg(case, ls[c]), float(noise[c]), xs,
                                 True, form=cc.form_name(case))
            em, ev = np.max(np.abs(means[c] - rm)) / np.max(np.abs(rm)), np.max(np.abs(variances[c] - rv) / rv)
            print(case["id"], c, em, ev)
            assert em <= 1e-8 and ev <= 1e-8, (c, em, ev)
    finally:
        lib.gprx_destroy(h)


# ---- 2. bits --------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("case", gc.CASES, ids=[c["id"] for c in gc.CASES])
def test_held_general_bits(lib, case):
    """(a) the cell with the empty hold, and a whole call whose holds are all empty, have the bits of gprx_objective_batch, the other
    seven cells do not; (b) every held cell alone has the bits it has inside the batch of eight; (c) holds A, a permutation B of them,
    A again on one shape: the first and the third call agree bit for bit and the second differs -- a replayed graph reads the table of
    its own call; (d) with "held_general" back at 0 the call is refused."""
    x, y, thetas, zs, units, *_ = cc.draw_inputs(case)
    lo, hi = gc.hold_arrays(case)
    h = open_handle(lib, case, x, y)
    try:
        losses, grads = objective(lib, h, units, thetas, zs, ALL, lo, hi)
        plain_l, plain_g = objective(lib, h, units, thetas, zs, ALL)
        e = gc.EMPTY_CELL
        assert losses[e] == plain_l[e] and np.array_equal(grads[e], plain_g[e])
        for c in range(gc.CELLS):
            if c != e:
                assert losses[c] != plain_l[c] and not np.array_equal(grads[c], plain_g[c]), c
        zero = np.zeros(gc.CELLS, dtype=np.int64)
        for lo0 in (zero, zero + 300):
            el, eg = objective(lib, h, units, thetas, zs, ALL, lo0, lo0)
            assert np.array_equal(el, plain_l) and np.array_equal(eg, plain_g)
        # (b)
        for c in range(gc.CELLS):
            cl, cg = objective(lib, h, units[c:c + 1], thetas[c:c + 1], zs[c:c + 1], ALL, lo[c:c + 1], hi[c:c + 1])
            assert cl[0] == losses[c] and np.array_equal(cg[0], grads[c]), c
    finally:
        lib.gprx_destroy(h)
    # (c) on a fresh handle: eager with A, captured with B, replayed with A
    perm = np.roll(np.arange(gc.CELLS), 3)
    h = open_handle(lib, case, x, y)
    try:
        a1 = objective(lib, h, units, thetas, zs, ALL, lo, hi)
        b = objective(lib, h, units, thetas, zs, ALL, lo[perm], hi[perm])
        a2 = objective(lib, h, units, thetas, zs, ALL, lo, hi)
        b2 = objective(lib, h, units, thetas, zs, ALL, lo[perm], hi[perm])
        assert np.array_equal(a1[0], losses) and np.array_equal(a1[1], grads)
        assert np.array_equal(a1[0], a2[0]) and np.array_equal(a1[1], a2[1])
        assert np.array_equal(b[0], b2[0]) and np.array_equal(b[1], b2[1])
        assert all(b[0][c] != a1[0][c] for c in range(gc.CELLS))  # (the rolled holds give every cell another range)
        # (d)
        check(lib.gprx_set_handle_tuning(h, b"held_general", 0), h)
        u, th, z = np.ascontiguousarray(units), np.ascontiguousarray(thetas), np.ascontiguousarray(zs)
        out_l, out_g = np.zeros(gc.CELLS), np.zeros_like(grads)
        rc = lib.gprx_objective_batch_held(h, gc.CELLS, ptr(u), ptr(th), ptr(z), ALL, ptr(out_l), ptr(out_g), ptr(lo), ptr(hi))
        msg = _lib.last_error(h)
        assert rc == _lib.GPRX_EINVAL and ("sgpr_fused" in msg if case["m"] <= 64 else "64 inducing points" in msg), (rc, msg)
    finally:
        lib.gprx_destroy(h)


# ---- 3. resident loops ----------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [ALL, Z_ONLY], ids=["mask15", "mask8"])
@pytest.mark.parametrize("kind, steps", [("adam", 30), ("adadelta", 10)])
@pytest.mark.parametrize("case", gc.RESIDENT_CASES, ids=[c["id"] for c in gc.RESIDENT_CASES])
def test_held_general_resident_loops(lib, case, kind, steps, mask):
    """Eight cells with all eight holds: the resident loop around the general launch sequence (route 2) gives the variables, Z and
    evaluation counts of the host-stepped loop ("sgpr_resident" = 0, route 0) bit for bit; every cell but the empty one ends somewhere
    other than in the loop without holds."""
    x, y, thetas, zs, units, *_ = cc.draw_inputs(case)
    lo, hi = gc.hold_arrays(case)
    h = open_handle(lib, case, x, y)
    try:
        th, z, ev, route = run_loop(lib, h, kind, units, thetas, zs, mask, steps, lo, hi)
        assert route == 2
        assert np.all(ev == steps)
        check(lib.gprx_set_handle_tuning(h, b"sgpr_resident", 0), h)
        th0, z0, ev0, route0 = run_loop(lib, h, kind, units, thetas, zs, mask, steps, lo, hi)
        check(lib.gprx_set_handle_tuning(h, b"sgpr_resident", 1), h)
        assert route0 == 0
        assert np.array_equal(th, th0) and np.array_equal(z, z0) and np.array_equal(ev, ev0)
        thp, zp, _, routep = run_loop(lib, h, kind, units, thetas, zs, mask, steps)
        assert routep == 2
        e = gc.EMPTY_CELL
        assert np.array_equal(thp[e], th[e]) and np.array_equal(zp[e], z[e])
        assert all(not (np.array_equal(thp[c], th[c]) and np.array_equal(zp[c], z[c])) for c in range(gc.CELLS) if c != e)
    finally:
        lib.gprx_destroy(h)


@pytest.mark.gpu
def test_held_general_shrinking_residency(lib):
    """The early-stop inputs of test_gpu_sparse_resident (M = 130, five cells, cells 0 and 3 start where the loss is flat), 80 Adam steps,
    every cell holding another range out.  Asserted first: a cell stops at or before evaluation 75 and a cell runs all 80 steps, so the
    read after step 75 reopened the residency for the survivors, whose table rows moved to new slots.  Routes 2 and 0 agree bit for bit,
    and every surviving cell has the bits of the same cell run alone with its hold."""
    from test_gpu_sparse_general import draw_inputs

    case = dict(kernel="Matern52", d=9, m=130, n=400, ard=False, form=0, cells=5, seed=70, cond_scaled=False)
    x, y, thetas, zs, *_ = draw_inputs(case, units=5)
    units = np.arange(5, dtype=np.int32)
    for c in (0, 3):
        thetas[c] = np.concatenate([np.atleast_1d(w) for w in otr.unconstrain(np.exp(-1.0), np.full(1, np.exp(-1.0)), 1e5)])
    lo = np.ascontiguousarray([70, 60, 250, 0, 128], dtype=np.int64)
    hi = np.ascontiguousarray([100, 70, 262, 37, 256], dtype=np.int64)
    h = open_handle(lib, case, x, y)
    try:
        th, z, ev, route = run_loop(lib, h, "adam", units, thetas, zs, ALL, 80, lo, hi)
        print("evaluations", ev.tolist())
        assert route == 2
        assert ev.min() <= 75 and ev.max() == 80  # (the residency was reopened with fewer cells)
        check(lib.gprx_set_handle_tuning(h, b"sgpr_resident", 0), h)
        th0, z0, ev0, route0 = run_loop(lib, h, "adam", units, thetas, zs, ALL, 80, lo, hi)
        check(lib.gprx_set_handle_tuning(h, b"sgpr_resident", 1), h)
        assert route0 == 0
        assert np.array_equal(th, th0) and np.array_equal(z, z0) and np.array_equal(ev, ev0)
        for c in np.flatnonzero(ev == 80):
            one = slice(c, c + 1)
            th1, z1, ev1, route1 = run_loop(lib, h, "adam", units[one], thetas[one], zs[one], ALL, 80, lo[one], hi[one])
            assert route1 == 2 and ev1[0] == 80
            assert np.array_equal(th1[0], th[c]) and np.array_equal(z1[0], z[c]), c
    finally:
        lib.gprx_destroy(h)


# ---- 4. end to end --------------------------------------------------------------------------------------------------------------

M_E2E = 70


@pytest.fixture(scope="module")
def e2e_data():
    from gpras_amd.synth import make_regression

    x, y, _ = make_regression(E2E["n"], E2E["d"], n_outputs=E2E["k"], n_test=0, config=31, unit=7)
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def _close(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.gpu
@pytest.mark.parametrize("method, kwargs", [("adam", dict(max_iter=6)), ("two-stage", dict(max_iter=4))], ids=["adam", "two-stage"])
def test_cross_validate_held_general(lib, e2e_data, method, kwargs):
    """M = 70 on the E2E shape of test_gpu_crossval.  At max_iter = 0 (every fold's initial state) route="held_general" and
    route="engines" agree within 1e-8 on loss and predictions; after a short fit the result names its route, has the shapes of the
    data and is finite; GPRAS.cross_validate(events, route="held_general") returns the function's bits."""
    from gpras_amd.crossval import cross_validate
    from gpras_amd.gpr import GPRAS

    x, y = e2e_data
    n, k, ev = E2E["n"], E2E["k"], E2E["events"]
    general = cross_validate(E2E["kernel"], x, y, ev, M_E2E, optimization_method=method, route="held_general", max_iter=0)
    engines = cross_validate(E2E["kernel"], x, y, ev, M_E2E, optimization_method=method, route="engines", max_iter=0)
    assert general.route == "held_general" and engines.route == "engines"
    assert np.array_equal(general.Z, engines.Z) and np.array_equal(general.thetas, engines.thetas)  # the same initial state
    em, evar = _close(general.mean, engines.mean), float(np.max(np.abs(general.var - engines.var) / engines.var))
    el = float(np.max(np.abs(general.first_loss - engines.first_loss) / np.abs(engines.first_loss)))
    print("routes at the initial state", em, evar, el)
    assert em <= 1e-8 and evar <= 1e-8 and el <= 1e-8
    res = cross_validate(E2E["kernel"], x, y, ev, M_E2E, optimization_method=method, route="held_general", **kwargs)
    assert res.route == "held_general" and res.ranges == ev
    assert res.mean.shape == res.var.shape == (n, k) and np.isfinite(res.mean).all() and np.isfinite(res.var).all()
    assert res.thetas.shape == (6, k, 3) and res.Z.shape == (6, k, M_E2E, E2E["d"]) and res.n_evals.shape == (6, k)
    assert np.all(res.n_evals > 0) and np.isfinite(res.last_loss).all()
    assert not np.array_equal(res.mean, general.mean)  # (the fit moved the folds)
    g = GPRAS(E2E["kernel"])
    g.fit(x, y, M_E2E, optimization_method=method, **kwargs)
    try:
        same = g.cross_validate(ev, route="held_general")
    finally:
        for eng in g.engines:
            eng.close()
    assert same.route == "held_general"
    assert np.array_equal(same.mean, res.mean) and np.array_equal(same.var, res.var)
    assert np.array_equal(same.thetas, res.thetas) and np.array_equal(same.Z, res.Z)
