"""GPU tests of the optimiser drivers beyond ``adam`` / ``two-stage`` on the HIP engine: Adadelta inside the library
(``gprx_adadelta_batch``: resident on the device for sparse models with M <= 64, host-stepped otherwise) against Python loops over
the library's own evaluations, bit for bit; and ``adadelta``, ``three-stage``, ``stochastic`` and ``diffential_evolution`` end to end
against the oracle's CPU restatement and against their own serial form."""

import ctypes as C

import numpy as np
import pytest
from test_gpu_sparse_variants import ALL, HYPER, batch, draw_inputs, make_handle

from gpras_amd import _lib, model, optimizers
from gpras_amd._lib import check, ptr
from gpras_amd.gpr import GPRAS
from gpras_amd.synth import make_hydrograph_features, make_regression
from oracle import gpras_oracle
from oracle import kernels as okn

pytestmark = pytest.mark.gpu

Z_ONLY = _lib.TRAIN_Z


def _python_adadelta(lib, h, units, thetas, zs, mask, max_iter):
    """optimizers._optimize_adadelta restated over gprx_objective_batch: Keras's Adadelta defaults on the trainable columns, exactly
    max_iter steps, one batched evaluation of all cells per step.  Returns the variables, the evaluation counts, the number of
    batched evaluations and the loss of each cell's last evaluation (NaN where none was made)."""
    lr, rho, eps = 1e-3, 0.95, 1e-7
    cells, nt = thetas.shape
    m, d = zs.shape[1:]
    xv = np.concatenate([thetas, zs.reshape(cells, -1)], axis=1)
    flags = [bool(mask & b) for b in (_lib.TRAIN_VARIANCE, _lib.TRAIN_LENGTHSCALE, _lib.TRAIN_NOISE, _lib.TRAIN_Z)]
    cols = np.flatnonzero(np.concatenate([[flags[0]], np.full(nt - 2, flags[1]), [flags[2]], np.full(m * d, flags[3])]))
    acc_grad, acc_delta = np.zeros((cells, cols.size)), np.zeros((cells, cols.size))
    n_evals, batches, last = np.zeros(cells, dtype=np.int32), 0, np.full(cells, np.nan)
    for _ in range(max_iter):
        th = np.ascontiguousarray(xv[:, :nt])
        zz = np.ascontiguousarray(xv[:, nt:].reshape(cells, m, d))
        last, grads = batch(lib, h, units, th, zz, mask)
        batches += 1
        n_evals += 1
        g = grads[:, cols]
        acc_grad = rho * acc_grad + (1.0 - rho) * g * g
        delta = -np.sqrt(acc_delta + eps) * g / np.sqrt(acc_grad + eps)
        acc_delta = rho * acc_delta + (1.0 - rho) * delta * delta
        xv[:, cols] = xv[:, cols] + lr * delta
    return xv[:, :nt].copy(), xv[:, nt:].reshape(cells, m, d).copy(), n_evals, batches, last


def _library_adadelta(lib, h, units, thetas, zs, mask, max_iter):
    cells = units.size
    th, zz = thetas.copy(), zs.copy()
    n_evals, batches, losses = np.full(cells, -1, dtype=np.int32), C.c_int(-1), np.zeros(cells)
    rc = lib.gprx_adadelta_batch(h, cells, ptr(units), ptr(th), ptr(zz), mask, max_iter, ptr(losses), ptr(n_evals), C.byref(batches))
    return rc, th, zz, n_evals, batches.value, losses


# ---- 1. the three loops ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_inducing", [None, 16, 100])
def test_adadelta_inside_the_library_equals_the_python_loops(n_inducing):
    """gprx_adadelta_batch against the packed Python loop and against the serial per-model driver, 5 modes, 60 steps (the resident
    loop's windows of 25, 25 and 10): the same variables bit for bit, 60 evaluations per model.  No inducing points run the
    host-stepped loop on exact models, 16 the loop resident on the device, 100 (M > 64) the host-stepped loop over the general
    launch sequence."""
    x, y = make_hydrograph_features(260, 3, n_outputs=5, config=1, unit=11)

    def prepared():
        g = GPRAS("Matern52")
        g.x, g.y = x, y
        g._init_models(x, y, n_inducing, "grid")
        for k, m in enumerate(g.models):  # (every mode starts somewhere else)
            m.set_vector(m.get_vector() + 0.1 * k)
        return g

    a, b, c = prepared(), prepared(), prepared()
    start = [m.get_vector() for m in a.models]
    assert hasattr(a.engine, "adadelta_batch")
    stats = {"batches": 0}
    losses_a = optimizers._optimize_adadelta_many(a.models, 60, stats)  # library loop
    packed = optimizers._PackedBatch(b.models)
    losses_b = optimizers._adadelta_packed(packed, np.stack([m.get_vector() for m in b.models]), 60, None)  # Python loop, batched evaluations
    losses_c = [optimizers._optimize_adadelta(m, 60) for m in c.models]  # serial driver
    assert stats["batches"] == 60
    assert [m.n_evals for m in a.models] == [m.n_evals for m in b.models] == [m.n_evals for m in c.models] == [60] * 5
    for ma, mb, mc, v0 in zip(a.models, b.models, c.models, start):
        va, vb, vc = ma.get_vector(), mb.get_vector(), mc.get_vector()
        assert np.array_equal(va, vb) and np.array_equal(va, vc)
        assert not np.array_equal(va, v0)  # (the loop moved the variables)
    assert np.array_equal(losses_a, losses_b) and np.array_equal(losses_a, np.array(losses_c))


# ---- 2. the resident loop's edges -----------------------------------------------------------------------------------------------

SMALL = dict(kernel="RBF", d=3, m=17, n=300, ard=False, form=0, cells=3, seed=301)  # m d = 51 < 1024: one pass of the Z loop
TAIL = dict(kernel="RBF", d=21, m=50, n=300, ard=False, form=0, cells=3, seed=302)  # m d = 1050: the clamped tail of a second pass
TAIL_ARD = dict(kernel="RBF", d=21, m=50, n=300, ard=True, form=0, cells=3, seed=303)  # ... with 23 hyperparameter threads, d > 16 restaged
EXPANDED = dict(kernel="Matern12", d=5, m=33, n=300, ard=False, form=1, cells=3, seed=304)  # the expanded-form kernels
RESIDENT_CASES = [
    ("one-pass", SMALL, ALL, 26), ("tail", TAIL, ALL, 26), ("tail-ard", TAIL_ARD, ALL, 26), ("expanded", EXPANDED, ALL, 26),
    ("hyper-only", SMALL, HYPER, 26), ("z-only", SMALL, Z_ONLY, 26), ("tail-z-only", TAIL, Z_ONLY, 3),
    ("one-step", SMALL, ALL, 1), ("one-window", SMALL, ALL, 25), ("no-step", SMALL, ALL, 0),
]


@pytest.mark.parametrize("name,case,mask,max_iter", RESIDENT_CASES, ids=[c[0] for c in RESIDENT_CASES])
def test_resident_adadelta_equals_a_loop_over_batched_evaluations(lib, name, case, mask, max_iter):
    """The Adadelta instantiations of sf_adam_prep_kernel at the smallest shapes at which they can go wrong, 3 cells with mixed
    units: variables, Z, evaluation counts and the returned last losses equal the same loop written here over
    gprx_objective_batch, bit for bit; variables outside the mask stay as they went in; zero steps change nothing."""
    x, y, thetas, zs, units, *_ = draw_inputs(case, units=3)
    h = make_handle(lib, case, x, y)
    try:
        rc, th, zz, n_evals, batches, losses = _library_adadelta(lib, h, units, thetas, zs, mask, max_iter)
        assert rc == _lib.GPRX_OK, lib.gprx_last_error(h)
        th_py, zs_py, ev_py, batches_py, losses_py = _python_adadelta(lib, h, units, thetas.copy(), zs.copy(), mask, max_iter)
        assert n_evals.tolist() == ev_py.tolist() == [max_iter] * 3 and batches == batches_py == max_iter
        assert np.array_equal(th, th_py) and np.array_equal(zz, zs_py)
        assert np.array_equal(losses, losses_py, equal_nan=True)
        assert np.isnan(losses).all() if max_iter == 0 else np.isfinite(losses).all()
        assert np.array_equal(th, thetas) == (max_iter == 0 or not (mask & HYPER))
        assert np.array_equal(zz, zs) == (max_iter == 0 or not (mask & Z_ONLY))
    finally:
        lib.gprx_destroy(h)


# ---- 3. two groups of cells -----------------------------------------------------------------------------------------------------


def test_resident_adadelta_in_two_groups_of_cells_equals_one_group(lib):
    """19 cells forced into two groups on two streams ("sgpr_groups_from" = 1) against the grouping switched off (0): the same
    variables, losses and evaluation counts bit for bit."""
    n, d, m, cells, outs = 400, 3, 20, 19, 4
    x, y, _ = make_regression(n, d, n_outputs=outs, n_test=0, config=14, unit=19)
    h = C.c_void_p()
    check(lib.gprx_create(0, n, d, m, okn.KERNEL_IDS["Matern32"], 0, C.byref(h)))
    check(lib.gprx_set_data(h, ptr(x), ptr(y), outs), h)
    try:
        rng = np.random.default_rng(19)
        units = np.ascontiguousarray(rng.integers(0, outs, size=cells), dtype=np.int32)
        th0 = np.ascontiguousarray(rng.normal(0.2, 0.3, size=(cells, 3)))
        zs0 = np.ascontiguousarray(np.stack([x[rng.choice(n, size=m, replace=False)] for _ in range(cells)]))
        out = []
        for groups_from in (0, 1):
            check(lib.gprx_set_tuning(b"sgpr_groups_from", groups_from))
            out.append(_library_adadelta(lib, h, units, th0, zs0, ALL, 40))
        (rc1, th1, zs1, ev1, b1, lo1), (rc2, th2, zs2, ev2, b2, lo2) = out
        assert rc1 == rc2 == _lib.GPRX_OK
        assert np.array_equal(th1, th2) and np.array_equal(zs1, zs2) and np.array_equal(lo1, lo2)
        assert (ev1 == 40).all() and (ev2 == 40).all() and b1 == b2 == 40
        assert not np.array_equal(th1, th0) and not np.array_equal(zs1, zs0) and np.isfinite(lo1).all()
    finally:
        lib.gprx_set_tuning(b"sgpr_groups_from", 17)
        lib.gprx_destroy(h)


# ---- 4. a cell that stops being positive definite -----------------------------------------------------------------------------


def test_resident_adadelta_reports_a_cell_that_stops_being_positive_definite(lib):
    """A cell whose Kuu is numerically singular from the first step on (a numerical status: every launch completes) ends the call
    with GPRX_ENOTPD at the first read of the error word and is named; it comes back as it went in with its one evaluation
    counted; the other cells equal a clean run stopped at their evaluation count; the handle serves a clean run afterwards."""
    n, d, m, cells = 500, 3, 24, 3
    x, y, _ = make_regression(n, d, n_outputs=3, n_test=0, config=14, unit=5)
    h = C.c_void_p()
    check(lib.gprx_create(0, n, d, m, okn.KERNEL_IDS["RBF"], 0, C.byref(h)))
    check(lib.gprx_set_data(h, ptr(x), ptr(y), 3), h)
    try:
        rng = np.random.default_rng(9)
        units = np.arange(cells, dtype=np.int32)
        good = np.ascontiguousarray(rng.normal(0.2, 0.3, size=(cells, 3)))
        zs0 = np.ascontiguousarray(np.stack([x[rng.choice(n, size=m, replace=False)] for _ in range(cells)]))
        rc, th_ref, zs_ref, ev_ref, _, lo_ref = _library_adadelta(lib, h, units, good, zs0, ALL, 30)
        assert rc == _lib.GPRX_OK and (ev_ref == 30).all()
        bad = good.copy()
        bad[1] = [1e12, 1e6, 0.0]
        rc, th, zs, ev, _, lo = _library_adadelta(lib, h, units, bad, zs0, ALL, 30)
        assert rc == _lib.GPRX_ENOTPD
        assert b"cell 1" in lib.gprx_last_error(h)
        assert ev[1] == 1 and np.array_equal(th[1], bad[1]) and np.array_equal(zs[1], zs0[1]) and np.isnan(lo[1])
        assert ev[0] == ev[2] and 1 < ev[0] <= 30
        rc, th_k, zs_k, ev_k, _, lo_k = _library_adadelta(lib, h, units, good, zs0, ALL, int(ev[0]))
        assert rc == _lib.GPRX_OK and (ev_k == ev[0]).all()
        for c in (0, 2):
            assert np.array_equal(th[c], th_k[c]) and np.array_equal(zs[c], zs_k[c]) and lo[c] == lo_k[c], c
        rc, th2, zs2, ev2, _, lo2 = _library_adadelta(lib, h, units, good, zs0, ALL, 30)
        assert rc == _lib.GPRX_OK and np.array_equal(th2, th_ref) and np.array_equal(zs2, zs_ref) and np.array_equal(ev2, ev_ref)
        assert np.array_equal(lo2, lo_ref)
    finally:
        lib.gprx_destroy(h)


# ---- 5. the drivers against the oracle --------------------------------------------------------------------------------------------

DRIVER_KWARGS = {
    "adadelta": lambda: {"max_iter": 30},
    "three-stage": lambda: {"max_iter": 6},
    "stochastic": lambda: {"n_starts": 3, "iter_initial": 5, "iter_final": 6, "rng": np.random.default_rng(5)},
    "diffential_evolution": lambda: {"popsize": 3, "max_iter": 2, "seed": 3, "adam_iter": 30, "verbose": False},
}


@pytest.fixture(scope="module")
def problem():
    x, y, xs = make_regression(300, 3, n_outputs=3, n_test=40, config=21, unit=3)
    return x, y, xs


def _both(problem, method):
    x, y, _ = problem
    g = GPRAS("Matern52")
    g.fit(x, y, n_inducing=20, inducing_initializer="kmeans", optimization_method=method, **DRIVER_KWARGS[method]())
    kw = DRIVER_KWARGS[method]()
    kw.pop("verbose", None)
    ref = gpras_oracle.GPRASOracle("Matern52")
    ref.fit(x, y, n_inducing=20, inducing_initializer="kmeans", optimization_method=method, **kw)
    return g, ref


def test_adadelta_on_the_engine_against_the_oracle(problem):
    x, y, xs = problem
    g, ref = _both(problem, "adadelta")
    start = GPRAS("Matern52")
    start.x, start.y = x, y
    start._init_models(x, y, 20, "kmeans")
    for a, b, s in zip(g.models, ref.models, start.models):
        assert a.variance == pytest.approx(b.variance, rel=1e-8)
        assert a.lengthscales == pytest.approx(b.lengthscales, rel=1e-8)
        assert a.noise == pytest.approx(b.noise, rel=1e-8)
        assert np.allclose(a.inducing_variable.Z, b.Z, rtol=1e-8, atol=1e-10)
        moved = np.abs(a.theta() - s.theta())
        print("adadelta moved the variables by", moved)
        assert (moved >= 1e-5).all(), moved
        assert a.n_evals == 30
    mean, var = g.predict(xs)
    rmean, rvar = ref.predict(xs)
    assert np.max(np.abs(mean - rmean)) <= 1e-8 * np.max(np.abs(rmean))
    assert np.max(np.abs(var - rvar) / rvar) <= 1e-8


@pytest.mark.parametrize("method", ["three-stage", "stochastic"])
def test_drivers_that_end_in_lbfgs_reach_the_oracles_objective(problem, method):
    g, ref = _both(problem, method)
    for a, b in zip(g.models, ref.models):
        la, lb = a.training_loss(), b.training_loss()
        print(method, "training loss", la, lb, abs(la - lb) / abs(lb))
        assert la == pytest.approx(lb, rel=1e-6)


def test_differential_evolution_on_the_engine_against_the_oracle(problem):
    g, ref = _both(problem, "diffential_evolution")
    for a, b in zip(g.models, ref.models):
        assert np.allclose(a.inducing_variable.Z, b.Z, rtol=1e-8, atol=1e-10)  # (only the Adam stage moves Z)
        assert a.mask == model.TRAIN_Z
        assert -1 <= np.log10(a.variance) <= 1 and -1 <= np.log10(a.lengthscales) <= 1 and -3 <= np.log10(a.noise) <= 1e-3


# ---- 6. the batched route against the serial drivers ----------------------------------------------------------------------------


@pytest.mark.parametrize("modes", [3, 1])
@pytest.mark.parametrize("method", list(DRIVER_KWARGS))
def test_batched_route_equals_the_serial_driver_on_the_engine(problem, method, modes):
    x, y, _ = problem
    assert method in optimizers.BATCHED_OPTIMIZERS
    a = GPRAS("Matern52")
    a.fit(x, y[:, :modes], 20, "kmeans", method, **DRIVER_KWARGS[method]())
    b = GPRAS("Matern52")
    b.fit(x, y[:, :modes], 20, "kmeans", method, lockstep=False, **DRIVER_KWARGS[method]())
    for ma, mb in zip(a.models, b.models):
        assert np.array_equal(ma.theta(), mb.theta()) and np.array_equal(ma.Z, mb.Z)
        assert ma.n_evals == mb.n_evals and ma.mask == mb.mask
    assert a.lockstep_stats["evaluations"] == sum(m.n_evals for m in a.models)
    if modes > 1:
        assert a.lockstep_stats["batches"] < a.lockstep_stats["evaluations"]
