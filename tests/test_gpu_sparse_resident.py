"""GPU tests of the device-resident Adam and Adadelta loops around the GENERAL sparse launch sequence (gp_resident.h sgpr_resident_general,
csrc/sgpr_step.hip): sparse models with M > 64, and M <= 64 with "sgpr_fused" = 0.  The contract is the host-stepped loop's: the same
variables, evaluation counts and losses as a Python loop over gprx_objective_batch, bit for bit, whatever the window, the replay state
of the step's graph or the size the batch has shrunk to.  gprx_last_optimizer_route tells which loop a call took (0 host-stepped,
1 resident fused, 2 resident general) and how often it waited for the stream."""

import ctypes as C
import math
import os

import numpy as np
import pytest
from test_gpu_drivers import _python_adadelta
from test_gpu_sparse_general import ALL, HYPER, ROOT, _python_adam, draw_inputs, make_handle

from gpras_amd import _lib, engine
from gpras_amd._lib import check, ptr
from gpras_amd.synth import make_regression
from oracle import kernels as okn
from oracle import transforms as otr

Z_ONLY = _lib.TRAIN_Z
CHECK_EVERY = 25  # gp_resident.h resident_check_every: steps between two reads of the stop flags (GPRX_ADAM_CHECK_EVERY)

# The smallest shapes that reach every branch of the step kernel and of the launch sequence around it (mp = M rounded up to 64).
B_FINISH = dict(kernel="RBF", d=3, m=65, n=300, ard=False, form=0, cells=3, seed=401)  # mp 128: sgpr_b_finish_kernel, no split-K
ADD_DIAG = dict(kernel="Matern52", d=9, m=130, n=400, ard=False, form=0, cells=5, seed=402)  # mp 192: add-diag route; m d = 1170 > 1024: second pass of the Z loop
ARD_SPLITK = dict(kernel="RBF", d=21, m=130, n=1100, ard=True, form=0, cells=3, seed=403)  # 23 hyperparameter threads; np >= 1024: split-K
EXPANDED = dict(kernel="Matern12", d=5, m=70, n=300, ard=False, form=1, cells=3, seed=404)  # the expanded distance form
ONE_TILE = dict(kernel="RBF", d=3, m=17, n=300, ard=False, form=0, cells=3, seed=405, unfused=True)  # "sgpr_fused" = 0: mp 64, sgpr_small_kernel
SHAPES = {"m65": B_FINISH, "m130": ADD_DIAG, "m130-ard": ARD_SPLITK, "m70-expanded": EXPANDED, "m17-unfused": ONE_TILE}
# (shape, mask, max_iter): every shape with everything trainable one step past a window; the masks; no step, one step, exactly one
# window, a ragged last window; the second pass of the Z loop with Z alone
LOOP_CASES = (
    [(s, ALL, 26) for s in SHAPES]
    + [("m65", HYPER, 26), ("m65", Z_ONLY, 26), ("m130", Z_ONLY, 26)]
    + [("m65", ALL, it) for it in (0, 1, 25, 60)]
)


def open_handle(lib, case, x, y):
    h = make_handle(lib, case, x, y)
    if case.get("unfused"):
        check(lib.gprx_set_handle_tuning(h, b"sgpr_fused", 0), h)
    return h


def run_library(lib, h, opt, units, thetas, zs, mask, max_iter):
    """One gprx_adam_batch / gprx_adadelta_batch call on copies of the variables: rc, theta, Z, n_evals, batches, losses (None for
    Adam), route, host_waits."""
    cells = units.size
    th, zz = thetas.copy(), zs.copy()
    n_evals, batches = np.full(cells, -1, dtype=np.int32), C.c_int(-1)
    losses = None
    if opt == "adam":
        rc = lib.gprx_adam_batch(h, cells, ptr(units), ptr(th), ptr(zz), mask, max_iter, ptr(n_evals), C.byref(batches))
    else:
        losses = np.zeros(cells)
        rc = lib.gprx_adadelta_batch(h, cells, ptr(units), ptr(th), ptr(zz), mask, max_iter, ptr(losses), ptr(n_evals), C.byref(batches))
    route, waits = C.c_int(-1), C.c_int(-1)
    assert lib.gprx_last_optimizer_route(h, C.byref(route), C.byref(waits)) == _lib.GPRX_OK
    return rc, th, zz, n_evals, batches.value, losses, route.value, waits.value


def same_bits(a, b):
    """theta, Z, n_evals, batches and (Adadelta) the losses of two run_library results."""
    ok = np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4] == b[4]
    if a[5] is not None:
        ok = ok and np.array_equal(a[5], b[5], equal_nan=True)
    return ok


# ---- 1. the loop against a Python loop over batched evaluations -----------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["adam", "adadelta"])
@pytest.mark.parametrize("shape,mask,max_iter", LOOP_CASES, ids=[f"{s}-mask{k}-{it}" for s, k, it in LOOP_CASES])
def test_resident_general_loop_equals_a_loop_over_batched_evaluations(lib, shape, mask, max_iter, opt):
    """theta, Z, evaluation counts, batches and the Adadelta losses of the resident loop equal the same loop written in Python over
    gprx_objective_batch, bit for bit; variables outside the mask stay as they went in; the call took route 2 (max_iter = 0 makes no
    step and, by the routing rule max_iter > 0, reports the host-stepped route 0)."""
    case = SHAPES[shape]
    x, y, thetas, zs, units, *_ = draw_inputs(case, units=3)
    h = open_handle(lib, case, x, y)
    try:
        rc, th, zz, n_evals, batches, losses, route, waits = run_library(lib, h, opt, units, thetas, zs, mask, max_iter)
        assert rc == _lib.GPRX_OK, lib.gprx_last_error(h)
        assert route == (2 if max_iter > 0 else 0)
        if opt == "adam":
            th_py, zs_py, ev_py, batches_py = _python_adam(lib, h, units, thetas.copy(), zs.copy(), mask, max_iter)
        else:
            th_py, zs_py, ev_py, batches_py, losses_py = _python_adadelta(lib, h, units, thetas.copy(), zs.copy(), mask, max_iter)
            assert np.array_equal(losses, losses_py, equal_nan=True)
            assert np.isnan(losses).all() if max_iter == 0 else np.isfinite(losses).all()
        assert n_evals.tolist() == ev_py.tolist() and batches == batches_py == int(n_evals.max())
        assert n_evals.max() == max_iter  # (Adadelta: every cell; Adam: nothing here is flat enough to stop all cells within 60 steps)
        if opt == "adadelta":
            assert (n_evals == max_iter).all()
        assert np.array_equal(th, th_py) and np.array_equal(zz, zs_py)
        assert np.array_equal(th, thetas) == (max_iter == 0 or not (mask & HYPER))
        assert np.array_equal(zz, zs) == (max_iter == 0 or not (mask & Z_ONLY))
    finally:
        lib.gprx_destroy(h)


# ---- 2. early stop and the shrinking batch ----------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter,expected", [(60, [52, 60, 60, 52, 60]), (80, [52, 80, 80, 52, 80])], ids=["60", "80-shrinks"])
def test_early_stop_on_both_routes_of_one_handle(lib, max_iter, expected):
    """The inputs of test_host_stepped_adam_equals_a_loop_over_batched_evaluations (M = 130, cells 0 and 3 start where the loss is flat
    and stop after 52 evaluations) with "sgpr_resident" = 1 and = 0 on one handle: routes 2 and 0, identical bits.  With 60 steps the
    two cells stop inside the last window; with 80 the read after step 75 finds them stopped and the residency is reopened for the three
    survivors, whose bits must not change with their new slots and batch size."""
    case = dict(kernel="Matern52", d=9, m=130, n=400, ard=False, form=0, cells=5, seed=70, cond_scaled=False)
    x, y, thetas, zs, *_ = draw_inputs(case, units=5)
    units = np.arange(5, dtype=np.int32)
    for c in (0, 3):
        thetas[c] = np.concatenate([np.atleast_1d(w) for w in otr.unconstrain(np.exp(-1.0), np.full(1, np.exp(-1.0)), 1e5)])
    h = make_handle(lib, case, x, y)
    try:
        resident = run_library(lib, h, "adam", units, thetas, zs, ALL, max_iter)
        check(lib.gprx_set_handle_tuning(h, b"sgpr_resident", 0), h)
        stepped = run_library(lib, h, "adam", units, thetas, zs, ALL, max_iter)
        assert resident[0] == stepped[0] == _lib.GPRX_OK
        assert (resident[6], stepped[6]) == (2, 0)
        assert resident[3].tolist() == expected and resident[4] == max_iter
        assert same_bits(resident, stepped)
        assert not np.array_equal(resident[1], thetas) and not np.array_equal(resident[2], zs)
    finally:
        lib.gprx_destroy(h)


# ---- 3. few host waits --------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
def test_resident_general_loop_waits_once_per_window(lib):
    """Adadelta, 60 steps in windows of 25: the resident loop waits for the stream at most ceil(60 / 25) + 2 times (three windows, the
    opening upload, the final download); the host-stepped loop of the same call waits at least once per step."""
    if os.environ.get("GPRX_ADAM_CHECK_EVERY"):
        pytest.skip("GPRX_ADAM_CHECK_EVERY changes the window")
    x, y, thetas, zs, units, *_ = draw_inputs(B_FINISH, units=3)
    h = open_handle(lib, B_FINISH, x, y)
    try:
        resident = run_library(lib, h, "adadelta", units, thetas, zs, ALL, 60)
        check(lib.gprx_set_handle_tuning(h, b"sgpr_resident", 0), h)
        stepped = run_library(lib, h, "adadelta", units, thetas, zs, ALL, 60)
        assert resident[0] == stepped[0] == _lib.GPRX_OK and (resident[6], stepped[6]) == (2, 0)
        print("host waits: resident", resident[7], "host-stepped", stepped[7])
        assert 1 <= resident[7] <= math.ceil(60 / CHECK_EVERY) + 2
        assert stepped[7] >= 60
        assert same_bits(resident, stepped)
    finally:
        lib.gprx_destroy(h)


# ---- 4. eager, captured and replayed steps ------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["adam", "adadelta"])
def test_replayed_steps_equal_eager_and_captured_ones(lib, opt):
    """Two consecutive calls on one handle (the first sends its first step eagerly, captures the second and replays the rest; the second
    call replays every step) and one call on a fresh handle give identical bits."""
    x, y, thetas, zs, units, *_ = draw_inputs(ADD_DIAG, units=3)
    out = []
    h = open_handle(lib, ADD_DIAG, x, y)
    try:
        out.append(run_library(lib, h, opt, units, thetas, zs, ALL, 26))
        out.append(run_library(lib, h, opt, units, thetas, zs, ALL, 26))
    finally:
        lib.gprx_destroy(h)
    h = open_handle(lib, ADD_DIAG, x, y)
    try:
        out.append(run_library(lib, h, opt, units, thetas, zs, ALL, 26))
    finally:
        lib.gprx_destroy(h)
    for r in out:
        assert r[0] == _lib.GPRX_OK and r[6] == 2 and (r[3] == 26).all()
    assert same_bits(out[0], out[1]) and same_bits(out[0], out[2])
    assert not np.array_equal(out[0][1], thetas) and not np.array_equal(out[0][2], zs)


# ---- 4b. both resident routes alternating on one handle ----------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["adam", "adadelta"])
def test_both_resident_routes_alternate_on_one_handle(lib, opt):
    """The two resident loops share one state-block layout and one pinned block on a handle.  M = 17 with "sgpr_fused" = 0: three cells
    twice on route 2 (the second call replays the captured step); "sgpr_fused" = 1: nineteen cells on route 1, a larger state block,
    so it is reallocated and the captured steps are dropped; "sgpr_fused" = 0 again: the three cells on route 2.  The last route-2
    result equals the first and the route-1 result equals the same call on a fresh handle, bit for bit."""
    case = dict(ONE_TILE, cells=19)
    x, y, thetas, zs, units, *_ = draw_inputs(case, units=3)
    few = (units[:3].copy(), thetas[:3].copy(), zs[:3].copy())
    h = make_handle(lib, case, x, y)
    try:
        check(lib.gprx_set_handle_tuning(h, b"sgpr_fused", 0), h)
        general = [run_library(lib, h, opt, *few, ALL, 26) for _ in range(2)]
        check(lib.gprx_set_handle_tuning(h, b"sgpr_fused", 1), h)
        fused = run_library(lib, h, opt, units, thetas, zs, ALL, 26)
        check(lib.gprx_set_handle_tuning(h, b"sgpr_fused", 0), h)
        general.append(run_library(lib, h, opt, *few, ALL, 26))
    finally:
        lib.gprx_destroy(h)
    h = make_handle(lib, case, x, y)
    try:
        fresh = run_library(lib, h, opt, units, thetas, zs, ALL, 26)
    finally:
        lib.gprx_destroy(h)
    for r in general:
        assert r[0] == _lib.GPRX_OK and r[6] == 2
    for r in (fused, fresh):
        assert r[0] == _lib.GPRX_OK and r[6] == 1
    assert same_bits(general[0], general[1]) and same_bits(general[0], general[2])
    assert same_bits(fused, fresh)
    assert not np.array_equal(general[0][1], few[1]) and not np.array_equal(fused[2], zs)


# ---- 5. a cell that is not positive definite ----------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["adam", "adadelta"])
def test_resident_general_loop_reports_a_cell_that_is_not_positive_definite(lib, opt):
    """M = 130, cell 1 with a Kuu that is numerically singular from the first step on (a numerical status: every launch completes): the
    call ends with GPRX_ENOTPD at the first read of the error word and names the cell, which comes back as it went in with its one
    evaluation counted and a NaN loss; the other cells equal a clean run stopped at their evaluation count; a clean run afterwards
    equals the reference run."""
    n, d, m, cells = 500, 3, 130, 3
    x, y, _ = make_regression(n, d, n_outputs=3, n_test=0, config=14, unit=5)
    h = C.c_void_p()
    check(lib.gprx_create(0, n, d, m, okn.KERNEL_IDS["RBF"], 0, C.byref(h)))
    check(lib.gprx_set_data(h, ptr(x), ptr(y), 3), h)
    try:
        rng = np.random.default_rng(9)
        units = np.arange(cells, dtype=np.int32)
        good = np.ascontiguousarray(rng.normal(0.2, 0.3, size=(cells, 3)))
        zs0 = np.ascontiguousarray(np.stack([x[rng.choice(n, size=m, replace=False)] for _ in range(cells)]))
        ref = run_library(lib, h, opt, units, good, zs0, ALL, 30)
        assert ref[0] == _lib.GPRX_OK and ref[6] == 2 and (ref[3] == 30).all()
        bad = good.copy()
        bad[1] = [1e12, 1e6, 0.0]
        rc, th, zs, ev, _, lo, route, _ = run_library(lib, h, opt, units, bad, zs0, ALL, 30)
        assert rc == _lib.GPRX_ENOTPD and route == 2
        assert b"cell 1" in lib.gprx_last_error(h)
        assert ev[1] == 1 and np.array_equal(th[1], bad[1]) and np.array_equal(zs[1], zs0[1])
        if lo is not None:
            assert np.isnan(lo[1])
        assert ev[0] == ev[2] and 1 < ev[0] <= 30
        clean = run_library(lib, h, opt, units, good, zs0, ALL, int(ev[0]))
        assert clean[0] == _lib.GPRX_OK and (clean[3] == ev[0]).all()
        for c in (0, 2):
            assert np.array_equal(th[c], clean[1][c]) and np.array_equal(zs[c], clean[2][c]), c
            if lo is not None:
                assert lo[c] == clean[5][c], c
        again = run_library(lib, h, opt, units, good, zs0, ALL, 30)
        assert again[0] == _lib.GPRX_OK and same_bits(again, ref)
    finally:
        lib.gprx_destroy(h)


# ---- 6. the interface, without a GPU ------------------------------------------------------------------------------------------------


def test_route_export_and_tuning_key_are_declared():
    """gprx_last_optimizer_route and the tuning key "sgpr_resident" in the ctypes tables and in the public header."""
    assert _lib.PROTOTYPES["gprx_last_optimizer_route"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)])
    assert "sgpr_resident" in _lib.TUNING_KEYS
    with open(os.path.join(ROOT, "include", "gprx.h")) as f:
        header = f.read()
    assert "int gprx_last_optimizer_route(gprx_handle h, int* route, int* host_waits);" in header
    assert '"sgpr_resident"' in header


def test_engine_methods_that_drive_the_handle_hold_its_lock():
    """A handle is not thread-safe: the optimiser loops run its one stream, its staging blocks and its graph captures for thousands of
    steps, so Engine.adam_batch, Engine.adadelta_batch and the new Engine.last_optimizer_route are wrapped by engine._locked like the
    evaluation and predict calls beside them (functools.wraps leaves the plain method in __wrapped__)."""
    probe = engine._locked(lambda self: None)
    for name in ("objective_batch", "adam_batch", "adadelta_batch", "last_optimizer_route", "predict_batch"):
        method = vars(engine.Engine)[name]
        assert hasattr(method, "__wrapped__"), f"Engine.{name} does not take the engine's lock"
        assert method.__code__ is probe.__code__, f"Engine.{name} is wrapped by something other than engine._locked"


# ---- 7. the same through the Python engine ------------------------------------------------------------------------------------------


@pytest.mark.gpu
def test_engine_reports_the_route_of_its_batched_loops(lib):
    """Engine.adam_batch / Engine.adadelta_batch at M = 65 equal the C calls bit for bit and Engine.last_optimizer_route reports the
    resident general loop with its few waits; with "sgpr_resident" = 0 on the engine's handle the same call is host-stepped."""
    if os.environ.get("GPRX_ADAM_CHECK_EVERY"):
        pytest.skip("GPRX_ADAM_CHECK_EVERY changes the window")
    x, y, thetas, zs, units, *_ = draw_inputs(B_FINISH, units=3)
    eng = engine.Engine("RBF", x, y, n_inducing=B_FINISH["m"])
    h = open_handle(lib, B_FINISH, x, y)
    try:
        th, zz, n_evals, batches = eng.adam_batch(units, thetas, ALL, 26, zs=zs)
        assert eng.last_optimizer_route() == (2, math.ceil(26 / CHECK_EVERY) + 2)
        ref = run_library(lib, h, "adam", units, thetas, zs, ALL, 26)
        assert np.array_equal(th, ref[1]) and np.array_equal(zz, ref[2]) and np.array_equal(n_evals, ref[3]) and batches == ref[4]
        th, zz, n_evals, batches, losses = eng.adadelta_batch(units, thetas, ALL, 26, zs=zs)
        assert eng.last_optimizer_route() == (2, math.ceil(26 / CHECK_EVERY) + 2)
        ref = run_library(lib, h, "adadelta", units, thetas, zs, ALL, 26)
        assert np.array_equal(th, ref[1]) and np.array_equal(zz, ref[2]) and np.array_equal(n_evals, ref[3]) and batches == ref[4]
        assert np.array_equal(losses, ref[5])
        check(lib.gprx_set_handle_tuning(eng._h, b"sgpr_resident", 0), eng._h)
        th2, zz2, *_ = eng.adadelta_batch(units, thetas, ALL, 26, zs=zs)
        route, waits = eng.last_optimizer_route()
        assert route == 0 and waits >= 26
        assert np.array_equal(th2, th) and np.array_equal(zz2, zz)
    finally:
        lib.gprx_destroy(h)
        eng.close()
