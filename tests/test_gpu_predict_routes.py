"""Every route of the exact-model prediction (csrc/gp_predict.h) through the C ABI against the longdouble prediction of
tests/predict_reference.py: the inverse and the substitution route of a single model, their pass loops, the choice between them, the
cached L^-1 across refactorisations, and gprx_predict_batch with its fallbacks.  A result may be off by 8 x what a float64 restatement
of its route reaches on the same data (tests/golden/predict_bounds.json); every comparison prints `error / recorded ratio` first."""

import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import predict_reference as pr
from gpras_amd import _lib
from gpras_amd._lib import check, ptr
from gpras_amd.synth import make_regression
from oracle import exact as oex

pytestmark = pytest.mark.gpu

ALL = _lib.TRAIN_VARIANCE | _lib.TRAIN_LENGTHSCALE | _lib.TRAIN_NOISE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVERSE, SUBSTITUTION = 1, 2


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
class Model:
    """A handle on one case's data; destroyed on exit."""

    def __init__(self, lib, cid=None, *, kernel=None, ard=False, x=None, y=None):
        if cid is not None:
            c = pr.CASES[cid]
            kernel, ard = c.kernel, c.ard
            x, y, _ = pr.data(cid)
        self.lib, self.x, self.y = lib, np.ascontiguousarray(x), np.ascontiguousarray(y)
        self.h = C.c_void_p()
        check(lib.gprx_create(0, x.shape[0], x.shape[1], 0, pr.KERNEL_IDS[kernel], int(ard), C.byref(self.h)))
        check(lib.gprx_set_data(self.h, ptr(self.x), ptr(self.y), self.y.shape[1]), self.h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.gprx_destroy(self.h)

    def tune(self, key, value):
        check(self.lib.gprx_set_handle_tuning(self.h, key, value), self.h)

    def factorize(self, theta, unit=0):
        loss = C.c_double()
        check(self.lib.gprx_factorize(self.h, unit, ptr(np.ascontiguousarray(theta)), None, ALL, C.byref(loss)), self.h)
        return loss.value

    def predict(self, xs, include_noise=1):
        """(mean, var), written into canary-filled buffers."""
        xs = np.ascontiguousarray(xs)
        mean, var = pr.canary(xs.shape[0]), pr.canary(xs.shape[0])
        check(self.lib.gprx_predict(self.h, ptr(xs), xs.shape[0], ptr(mean), ptr(var), include_noise), self.h)
        return mean, var

    def predict_batch(self, units, thetas, xs, include_noise=1, transposed=False, expect=_lib.GPRX_OK):
        units, thetas, xs = np.ascontiguousarray(units, dtype=np.int32), np.ascontiguousarray(thetas), np.ascontiguousarray(xs)
        shape = (xs.shape[0], len(units)) if transposed else (len(units), xs.shape[0])
        means, vars_ = pr.canary(shape), pr.canary(shape)
        fn = self.lib.gprx_predict_batch_t if transposed else self.lib.gprx_predict_batch
        rc = fn(self.h, len(units), ptr(units), ptr(thetas), None, ptr(xs), xs.shape[0], ptr(means), ptr(vars_), include_noise)
        assert rc == expect, (rc, _lib.last_error(self.h))
        return means, vars_


def hold(mean, var, cid, cell, route, what, margin=1.0):
    """mean and var_y of one cell against the longdouble reference under 8 x the recorded ratio of its route."""
    ref_mean, ref_var = pr.reference(cid, cell)
    assert not np.any(np.isnan(mean)) and not np.any(np.isnan(var)), f"{what}: NaN (an output nobody wrote?)"
    em, ev = pr.mean_err(mean, ref_mean), pr.var_err(var, ref_var)
    am, av = pr.allowed(cid, cell, route, "mean"), pr.allowed(cid, cell, route, "var")
    print(f"{what} [{cid}/c{cell}/{route}]: mean {em:.3e} = {em / am * pr.MARGIN:.2f} x ratio, var {ev:.3e} = {ev / av * pr.MARGIN:.2f} x ratio")
    assert em <= margin * am, f"{what}: mean off by {em:.3e}, allowed {margin * am:.3e}"
    assert ev <= margin * av, f"{what}: variance off by {ev:.3e}, allowed {margin * av:.3e}"


def hold_latent(var_y, var_f, cid, cell, what):
    """include_noise = 0 changes only `base`: (var_y - var_f) is s up to the roundings of v + s, the two results and their difference."""
    v, _, s = pr.hyper(cid, cell)
    assert not np.any(np.isnan(var_f)), what
    assert np.max(np.abs((var_y - var_f) - s)) <= 4 * pr.U * (v + s), what


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(p).view(np.uint64), np.ascontiguousarray(q).view(np.uint64)) for p, q in zip(a, b))


# ---- a single model --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in pr.SINGLE])
def test_single_model_both_routes_against_longdouble(lib, cid):
    """S1-S7, each route forced on the handle; S7 is two passes at the N <= 1024 pass size with a 65-point last pass, so the offsets
    into the test points and both outputs are exercised on both routes.  The default is the inverse route at these sizes, bit for bit."""
    _, _, xs = pr.data(cid)
    theta = pr.thetas(cid)[0]
    got = {}
    with Model(lib, cid) as m:
        for path in (INVERSE, SUBSTITUTION, 0):
            m.tune(b"predict_path", path)
            m.factorize(theta)
            mean, var = m.predict(xs, 1)
            _, var_f = m.predict(xs, 0)
            route = pr.ROUTES[path or INVERSE]
            hold(mean, var, cid, 0, route, f"predict_path={path}")
            hold_latent(var, var_f, cid, 0, f"predict_path={path}")
            got[path] = (mean, var, var_f)
    assert same_bits(got[0], got[INVERSE])


@pytest.mark.parametrize("n,ns", [(1088, 16384 + 65), (2112, 8192 + 65)])
@pytest.mark.parametrize("path", [INVERSE, SUBSTITUTION])
def test_a_point_gets_the_same_bits_in_whichever_pass_it_falls(lib, n, ns, path):
    """The other two pass sizes of pred_tile_for (1024 < np <= 2048: 16384 points, np > 2048: 8192): all points in one call -- two
    passes, the second of 65 points -- against the first pass and the rest as two calls, where each is the first pass of its call."""
    tile = ns - 65
    x, y, xs = make_regression(n, 2, n_outputs=1, n_test=ns, config=42, unit=n)
    with Model(lib, kernel="RBF", x=x, y=y) as m:
        m.tune(b"predict_path", path)
        m.factorize(pr.theta_of(1.0, 0.8, 0.1))
        for include_noise in (1, 0):
            whole = m.predict(xs, include_noise)
            head, tail = m.predict(xs[:tile], include_noise), m.predict(xs[tile:], include_noise)
            assert not np.any(np.isnan(whole[0])) and not np.any(np.isnan(whole[1]))
            assert same_bits(whole, (np.concatenate([head[0], tail[0]]), np.concatenate([head[1], tail[1]])))


def test_route_choice_beyond_4096_rows(lib):
    """np > 4096: few points take the substitution, 2 N* >= N the inverse, and few points right after that (no refactorisation in
    between) the inverse again, from the cached L^-1.  Each default call is the forced route's bits; 100 points meet the oracle."""
    n, few, many = 4160, 100, 2100
    x, y, xs = make_regression(n, 2, n_outputs=1, n_test=many, config=42, unit=n)
    variance, ls, noise = 1.0, 0.8, 0.1
    theta = pr.theta_of(variance, ls, noise)
    with Model(lib, kernel="RBF", x=x, y=y) as m:
        def run(path, *counts):
            m.tune(b"predict_path", path)
            m.factorize(theta)
            return [m.predict(xs[:k], 1) for k in counts]

        default_few, = run(0, few)
        forced_sub_few, = run(SUBSTITUTION, few)
        default_many, default_few_cached = run(0, many, few)
        forced_inv_many, forced_inv_few = run(INVERSE, many, few)
    assert same_bits(default_few, forced_sub_few)
    assert same_bits(default_many, forced_inv_many)
    assert same_bits(default_few_cached, forced_inv_few)
    v, l, s = pr.constrain(theta)
    ref_mean, ref_var = oex.predict("RBF", x, y[:, 0], v, float(l[0]), s, xs[:few], True)
    for mean, var in (default_few, forced_inv_few):
        assert np.max(np.abs(mean - ref_mean)) <= 1e-8 * np.max(np.abs(ref_mean)) and np.max(np.abs(var - ref_var) / ref_var) <= 1e-8


def test_no_prediction_uses_the_inverse_of_an_earlier_factorisation(lib):
    """have_linv: every way the current factorisation changes under a cached L^-1 -- another gprx_factorize, an evaluation with a
    gradient (which leaves its own, not zeroed above the diagonal, in the same buffer), a batch, a slot selected from it -- is followed
    by a predict that must meet the reference of the NEW factorisation; the inverse of the old one misses it by orders of magnitude."""
    a, b, c = pr.thetas("S3")[0], pr.thetas("S3b")[0], pr.thetas("S3c")[0]
    _, _, xs = pr.data("S3")
    with Model(lib, "S3") as m:
        m.factorize(a)
        first = m.predict(xs)
        hold(*first, "S3", 0, "inverse", "after factorize(A)")
        assert same_bits(m.predict(xs), first)  # (from the cached L^-1)
        m.factorize(b)
        hold(*m.predict(xs), "S3b", 0, "inverse", "after factorize(B)")
        loss, grad = C.c_double(), np.zeros(a.size)
        check(lib.gprx_objective(m.h, 0, ptr(c), None, ALL, C.byref(loss), ptr(grad)), m.h)
        hold(*m.predict(xs), "S3c", 0, "inverse", "after objective(C) with gradient")
        means, vars_ = m.predict_batch([0, 0], np.stack([a, b]), xs)
        hold(means[0], vars_[0], "S3", 0, "inverse", "batch [A, B], cell 0")
        hold(means[1], vars_[1], "S3b", 0, "inverse", "batch [A, B], cell 1")
        check(lib.gprx_select_slot(m.h, 1), m.h)
        hold(*m.predict(xs), "S3b", 0, "inverse", "after select_slot(1)")
        m.factorize(a)
        assert same_bits(m.predict(xs), first)


# ---- gprx_predict_batch on exact handles -------------------------------------------------------------------------------------------
def hold_batch(means, vars_, cid, route, what, cells=None, vars_f=None):
    for cell in (range(len(pr.CASES[cid].units)) if cells is None else cells):
        hold(means[cell], vars_[cell], cid, cell, route, f"{what}, cell {cell}")
        if vars_f is not None:
            hold_latent(vars_[cell], vars_f[cell], cid, cell, f"{what}, cell {cell}")


def test_batch_ard_repeated_unit_both_layouts_and_the_slot_loop(lib, monkeypatch):
    """B1: ARD lengthscales through the cell-parameter table, a unit used twice, include_noise 1 and 0; the transposed entry point whole
    and in slabs of 2, 2, 1 cells; and with predict_path = 2 the loop over gprx_select_slot through the substitution route."""
    c = pr.CASES["B1"]
    _, _, xs = pr.data("B1")
    th = pr.thetas("B1")
    with Model(lib, "B1") as m:
        means, vars_ = m.predict_batch(c.units, th, xs, 1)
        _, vars_f = m.predict_batch(c.units, th, xs, 0)
        hold_batch(means, vars_, "B1", "inverse", "batch", vars_f=vars_f)
        monkeypatch.delenv("GPRX_PREDICT_SLAB", raising=False)
        whole = m.predict_batch(c.units, th, xs, 1, transposed=True)
        monkeypatch.setenv("GPRX_PREDICT_SLAB", "2")
        slabs = m.predict_batch(c.units, th, xs, 1, transposed=True)
        monkeypatch.delenv("GPRX_PREDICT_SLAB")
        assert same_bits(whole, (means.T, vars_.T)) and same_bits(slabs, (means.T, vars_.T))
        m.tune(b"predict_path", SUBSTITUTION)
        means2, vars2 = m.predict_batch(c.units, th, xs, 1)
        _, vars2_f = m.predict_batch(c.units, th, xs, 0)
        hold_batch(means2, vars2, "B1", "substitution", "slot loop", vars_f=vars2_f)
        assert not same_bits((means2,), (means,))  # (another route: another summation order)


@pytest.mark.parametrize("kernel", list(pr.KERNEL_IDS))
def test_batch_every_kernel_one_point(lib, kernel):
    cid = f"B2-{kernel}"
    with Model(lib, cid) as m:
        means, vars_ = m.predict_batch(pr.CASES[cid].units, pr.thetas(cid), pr.data(cid)[2], 1)
    hold_batch(means, vars_, cid, "inverse", "batch")


def test_batch_two_passes(lib):
    """B3: 8192 + 65 points, two passes of the batch's fixed pass size in every cell."""
    with Model(lib, "B3") as m:
        means, vars_ = m.predict_batch(pr.CASES["B3"].units, pr.thetas("B3"), pr.data("B3")[2], 1)
    hold_batch(means, vars_, "B3", "inverse", "batch")


def test_batch_after_the_cell_kernel_and_after_the_split_panel(lib):
    """B4, 33 cells of N = 128: by default the one-workgroup-per-cell factorisation feeds the batched trtri_lower; with cell_kernel = -1
    the launch sequence does, with the split panel and the right-hand side as a vector.  Cells 0, 16 and 32 against the reference in
    both; all cells of the two runs agree within twice the bound (each is within the bound of the reference)."""
    c = pr.CASES["B4"]
    th, xs = pr.thetas("B4"), pr.data("B4")[2]
    got = {}
    for cell_kernel in (0, -1):
        with Model(lib, "B4") as m:
            m.tune(b"cell_kernel", cell_kernel)
            got[cell_kernel] = m.predict_batch(c.units, th, xs, 1)
        hold_batch(*got[cell_kernel], "B4", "inverse", f"cell_kernel={cell_kernel}", cells=(0, 16, 32))
    (m0, v0), (m1, v1) = got[0], got[-1]
    assert not np.any(np.isnan(m0)) and not np.any(np.isnan(v0)) and not np.any(np.isnan(m1)) and not np.any(np.isnan(v1))
    for cell in range(len(c.units)):
        assert np.max(np.abs(m1[cell] - m0[cell])) <= 2 * pr.allowed("B4", cell, "inverse", "mean") * np.max(np.abs(m0[cell])), cell
        assert np.max(np.abs(v1[cell] - v0[cell]) / v0[cell]) <= 2 * pr.allowed("B4", cell, "inverse", "var"), cell


def test_batch_wider_than_the_parameter_table(lib):
    """B5, d = 65: the lengthscales do not fit a row of the cell-parameter table, each cell is evaluated and predicted on its own."""
    with Model(lib, "B5") as m:
        means, vars_ = m.predict_batch(pr.CASES["B5"].units, pr.thetas("B5"), pr.data("B5")[2], 1)
    hold_batch(means, vars_, "B5", "inverse", "per-cell loop")


def test_batch_with_a_non_positive_definite_cell_is_an_error_code_and_the_handle_lives_on(lib):
    """B6: duplicated rows, v = 2^40 beside s = 1e-6 in the second cell: the second pivot is exactly zero (the oracle's Cholesky raises,
    checked first).  The call answers GPRX_ENOTPD; the next one on the same handle, four good cells, answers with the reference."""
    c = pr.CASES["B6"]
    x, y, xs = pr.data("B6")
    th = pr.thetas("B6")
    bad = np.array([2.0 ** 40, th[1, 1], -800.0])
    with pytest.raises(np.linalg.LinAlgError, match="2-th leading minor"):
        oex.loss("RBF", x, y[:, 1], bad[0], bad[1], bad[2])
    with Model(lib, "B6") as m:
        m.predict_batch(c.units, np.stack([th[0], bad, th[2], th[3]]), xs, 1, expect=_lib.GPRX_ENOTPD)
        means, vars_ = m.predict_batch(c.units, th, xs, 1)
    hold_batch(means, vars_, "B6", "inverse", "after ENOTPD")


def test_batch_of_no_points_writes_nothing(lib):
    c = pr.CASES["B1"]
    units, th = np.ascontiguousarray(c.units, dtype=np.int32), pr.thetas("B1")
    means, vars_ = pr.canary((5, 4)), pr.canary((5, 4))
    with Model(lib, "B1") as m:
        for fn in (lib.gprx_predict_batch, lib.gprx_predict_batch_t):
            assert fn(m.h, 5, ptr(units), ptr(th), None, None, 0, ptr(means), ptr(vars_), 1) == _lib.GPRX_OK
    assert np.all(pr.is_canary(means)) and np.all(pr.is_canary(vars_))


# ---- the 128-wide tile of the variance GEMM ----------------------------------------------------------------------------------------
TILE128 = r"""
import json, sys
sys.path[:0] = [{root!r}, {tests!r}]
import predict_reference as pr
import test_gpu_predict_routes as t
from gpras_amd import _lib
lib = _lib.load()
out = {{}}
with t.Model(lib, "S4") as m:
    m.tune(b"predict_path", t.INVERSE)
    m.factorize(pr.thetas("S4")[0])
    out["S4"] = [[float.hex(v) for v in a] for a in m.predict(pr.data("S4")[2], 1)]
with t.Model(lib, "B1") as m:
    means, vars_ = m.predict_batch(pr.CASES["B1"].units, pr.thetas("B1"), pr.data("B1")[2], 1)
    out["B1"] = [[[float.hex(v) for v in row] for row in a] for a in (means, vars_)]
print(json.dumps(out))
"""


def test_variance_gemm_at_128_wide_tiles():
    """GPRX_PREDICT_TILE=128 (read once per process, hence a child): the register-staged 128 x 128 kernel with the rowsq epilogue, two
    slabs per 128 columns.  S4 (np = 256: two tile columns) and B1 (np = 192: a ragged second one) under the bounds of the inverse route."""
    env = dict(os.environ, GPRX_PREDICT_TILE="128")
    res = subprocess.run([sys.executable, "-c", TILE128.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300,
                         env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    unhex = lambda a: np.array([[float.fromhex(v) for v in row] for row in a])
    mean, var = unhex(out["S4"])
    hold(mean, var, "S4", 0, "inverse", "128-wide tile")
    hold_batch(unhex(out["B1"][0]), unhex(out["B1"][1]), "B1", "inverse", "128-wide tile, batch")
