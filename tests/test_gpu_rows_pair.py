"""The rows below a pair of panels in one launch (potrf.h: potrf_rows_pair_kernel, tuning key "rows_pair", default 1 where the split panel
runs) against one rows launch per panel ("rows_pair" = 0), against the lone factorisation of every cell, and against longdouble.

Two levels.  The probe gprx_potrf_batched (route 1, the split panel; it reads "rows_pair" from the process defaults) works on the canary
images of test_gpu_potrf_batched.py: the whole arena -- matrix padding, staging area, inverse blocks, right-hand side -- starts as NaN
patterns and only the block-lower part of K is uploaded, so a staged diagonal block that is not flushed, or a row that no workgroup
solved, shows as a NaN or as a difference.  There the factor is compared element by element, and the log-determinant as the sum the
library forms from the factor's diagonal.  gprx_factorize_batch (the threshold of 24 cells, the handle's own tuning copy) gives the loss,
which holds y^T K^-1 y, and the predictive mean, which holds alpha.

24 cells (the split-panel threshold) of one RBF data set in three dimensions with hyperparameters of their own.  Shapes:
  192   one pair whose rows launch has 64 rows, then a lone panel
  256   two pairs; the second has no rows beyond its diagonal group (with the right-hand side as a vector: no rows launch at all)
  300   padded to 320; a masked partial workgroup
  448   rows below the pairs that are no multiple of 128
  1088  crosses the 1024-column outer block: HEAD update, then a lone 64-column block

Bounds.  The factor, the inverse blocks, the log-determinant and -- with the right-hand side as a 64-row tile ("rhs_vector" = -1) --
everything else are the same BITS under "rows_pair" = 1 and 0 and in the lone call: the pair kernel repeats both rows kernels operation
for operation.  With the right-hand side as a vector, 64 entries of y per pair are updated in the diagonal workgroup in another summation
order (DESIGN.md 7c.3 for the vector form): beta to 1e-12 of its largest entry, y^T K^-1 y and the loss to 1e-14.  Against longdouble
(blocks_reference.chol_ld / solve_lower_ld): the noise is at least 0.5 of a variance near 1, so cond(K) is a few hundred and n u cond(K)
stays below 1e-12; beta, alpha and y^T K^-1 y are held to the 1e-11 that test_gpu_potrf_batched.py holds its well-conditioned matrices
to, the loss and the predictive mean to the 1e-9 / 1e-8 of test_gpu_exact.py against the oracle."""

import ctypes as C
import functools

import numpy as np
import pytest

import blocks_reference as br
import test_gpu_potrf_batched as pb
from gpras_amd import _lib
from gpras_amd._lib import check, ptr
from gpras_amd.synth import make_regression
from oracle import exact as oex
from oracle import transforms as otr

pytestmark = pytest.mark.gpu

NB, LD = br.NB, br.LD
CELLS = 24  # potrf_split_panel: the split panel from 24 cells per launch on
SHAPES = (192, 256, 300, 448, 1088)
ALL = _lib.TRAIN_VARIANCE | _lib.TRAIN_LENGTHSCALE | _lib.TRAIN_NOISE


def hypers(c):
    """(variance, lengthscale, noise) of cell c."""
    return 1.0 + 0.02 * c, 0.9 + 0.02 * c, 0.5 + 0.01 * c


@functools.lru_cache(maxsize=None)
def data(n):
    """x (n, 3), y (n, CELLS): one output per cell.  Read-only."""
    x, y, _ = make_regression(n, 3, n_outputs=CELLS, n_test=0, config=2, unit=n)
    for a in (x, y):
        a.setflags(write=False)
    return x, y


def padded(n):
    return -(-n // NB) * NB


@functools.lru_cache(maxsize=None)
def inputs(n, cells=CELLS):
    """Per cell K + s I padded to a multiple of 64 with a unit diagonal, and y padded with zeros -- as the library pads them."""
    x, y = data(n)
    r2 = np.sum((x[:, None, :] - x[None, :, :]) ** 2, axis=2)
    mats, ys = [], []
    for c in range(cells):
        v, ls, s = hypers(c)
        k = np.eye(padded(n))
        k[:n, :n] = v * np.exp(-0.5 * r2 / (ls * ls)) + s * np.eye(n)
        yp = np.zeros(padded(n))
        yp[:n] = y[:, c]
        mats.append(k)
        ys.append(yp)
    return mats, ys


def tile_rows(ys):
    """The right-hand side as the library's 64-row tile: y in its first row."""
    out = []
    for y in ys:
        rows = np.zeros((NB, y.size))
        rows[0] = y
        out.append(rows)
    return out


@functools.lru_cache(maxsize=None)
def reference(n, c):
    """(beta, y^T K^-1 y, alpha) of cell c in longdouble."""
    mats, ys = inputs(n)
    low = br.chol_ld(mats[c])
    beta = br.solve_lower_ld(low, ys[c])
    return beta, np.sum(beta * beta), br.solve_lower_ld(low, beta, transpose=True)


class rows_pair:
    """The process default of "rows_pair" for the probe, put back to 1 afterwards."""

    def __init__(self, lib, value):
        self.lib, self.value = lib, value

    def __enter__(self):
        check(self.lib.gprx_set_tuning(b"rows_pair", self.value))

    def __exit__(self, *exc):
        check(self.lib.gprx_set_tuning(b"rows_pair", 1))


def probe(lib, n, pair, vector, **kw):
    mats, ys = inputs(n)
    with rows_pair(lib, pair):
        if vector:
            return pb.factorise(lib, mats, route=1, y=ys, **kw)
        return pb.factorise(lib, mats, tile_rows(ys), route=1, extra=NB, **kw)


def logdet(low):
    """log det K from the factor's diagonal, summed in index order."""
    return 2.0 * float(np.add.reduce(np.log(np.diag(low))))


def quad(beta):
    return float(np.add.reduce(beta * beta))


@pytest.mark.parametrize("n", SHAPES)
def test_pair_launch_against_a_launch_per_panel_the_lone_call_and_longdouble(lib, n):
    mats, ys = inputs(n)
    rows = tile_rows(ys)
    got = {}
    for vector in (True, False):
        for pair in (1, 0):
            out, info = probe(lib, n, pair, vector)
            assert np.all(info == 0), (n, pair, vector, info)
            got[pair, vector] = out
    failures = []
    for c in range(CELLS):
        for vector in (True, False):
            a, b = got[1, vector][c], got[0, vector][c]
            where = f"n={n} {'vector' if vector else 'tile rows'}, cell {c}: rows_pair 1 against 0"
            pb.assert_same_cell(a, b, where, keys=("L", "inv") if vector else ("L", "inv", "rows"))
            assert logdet(a["L"]) == logdet(b["L"]), where
        # the right-hand side as a vector: another summation order in 64 entries per pair
        a, b = got[1, True][c]["y"], got[0, True][c]["y"]
        eb, eq = float(np.max(np.abs(a - b)) / np.max(np.abs(b))), abs(quad(a) - quad(b)) / quad(b)
        print(f"n={n} cell {c}: beta of rows_pair 1 against 0 {eb:.2e} (allowed 1e-12), y^T K^-1 y {eq:.2e} (allowed 1e-14)")
        if not (eb <= 1e-12 and eq <= 1e-14):
            failures.append(f"n={n} cell {c}: vector right-hand side, rows_pair 1 against 0: beta {eb:.3e}, y^T K^-1 y {eq:.3e}")
        # the lone call: fused panel, right-hand side as tile rows
        lone, info = pb.factorise(lib, mats[c:c + 1], rows[c:c + 1], route=0, extra=NB)
        assert info[0] == 0
        pb.assert_same_cell(got[1, False][c], lone[0], f"n={n} cell {c}: rows_pair 1 (tile rows) against the lone call")
        pb.assert_same_cell(got[1, True][c], lone[0], f"n={n} cell {c}: rows_pair 1 (vector) against the lone call", keys=("L", "inv"))
        assert logdet(got[1, False][c]["L"]) == logdet(lone[0]["L"]) and logdet(got[1, True][c]["L"]) == logdet(lone[0]["L"])
    for c in ((0, CELLS - 1) if n < 1000 else (CELLS - 1,)):  # (the longdouble factorisation of n = 1088 takes seconds: one cell)
        beta_ref, quad_ref, alpha_ref = reference(n, c)
        for vector in (True, False):
            res = got[1, vector][c]
            beta = res["y"] if vector else res["rows"][0]
            alpha = br.solve_lower_ld(res["L"], beta, transpose=True)  # (the device's factor and beta, substituted in longdouble)
            fig = {"beta": br.rel_err(beta, beta_ref), "alpha": br.rel_err(alpha, alpha_ref), "y^T K^-1 y": float(abs(LD(quad(beta)) - quad_ref) / quad_ref)}
            print(f"n={n} cell {c} {'vector' if vector else 'tile rows'} against longdouble: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()) + " (allowed 1e-11)")
            failures += [f"n={n} cell {c} {'vector' if vector else 'tile rows'}: {k} is {v:.3e} from the longdouble reference" for k, v in fig.items() if not v < 1e-11]
    pb.assert_none(failures)


def thetas_of(cells):
    return np.ascontiguousarray([[float(w) for w in otr.unconstrain(*hypers(c))] for c in range(cells)])


def batch_losses(lib, n, cells, tuning, slots=()):
    """Losses of gprx_factorize_batch on a fresh handle under its own tuning; per slot in `slots` the predictive mean at 40 points;
    the loss of gprx_factorize on every cell alone."""
    x, y = data(n)
    xs = make_regression(n, 3, n_outputs=1, n_test=40, config=2, unit=n)[2]
    thetas, units = thetas_of(cells), np.arange(cells, dtype=np.int32)
    h = C.c_void_p()
    check(lib.gprx_create(0, n, 3, 0, _lib.KERNEL_IDS["RBF"], 0, C.byref(h)))
    try:
        for key, value in tuning.items():
            check(lib.gprx_set_handle_tuning(h, key.encode(), value), h)
        check(lib.gprx_set_data(h, ptr(np.ascontiguousarray(x)), ptr(np.ascontiguousarray(y)), CELLS), h)
        losses, status = np.zeros(cells), np.zeros(cells, dtype=np.int32)
        check(lib.gprx_factorize_batch(h, cells, ptr(units), ptr(thetas), ALL, ptr(losses), ptr(status)), h)
        assert not status.any()
        means = {}
        for c in slots:
            check(lib.gprx_select_slot(h, c), h)
            mean, var = np.zeros(40), np.zeros(40)
            check(lib.gprx_predict(h, ptr(xs), 40, ptr(mean), ptr(var), 1), h)
            means[c] = mean
        single = np.zeros(cells)
        for c in range(cells):
            one = C.c_double()
            check(lib.gprx_factorize(h, c, ptr(np.ascontiguousarray(thetas[c])), None, ALL, C.byref(one)), h)
            single[c] = one.value
        return losses, means, single, xs
    finally:
        lib.gprx_destroy(h)


@pytest.mark.parametrize("n", SHAPES)
def test_losses_and_means_of_a_batch_of_24(lib, n):
    """gprx_factorize_batch at the threshold: the loss (log det + y^T K^-1 y) and the predictive mean (alpha) under "rows_pair" = 1 and 0
    and both forms of the right-hand side, against the single calls and against the oracle."""
    x, y = data(n)
    slots = (0, CELLS - 1)
    got = {(pair, rhs): batch_losses(lib, n, CELLS, {"rows_pair": pair, "rhs_vector": rhs}, slots) for pair in (1, 0) for rhs in (0, -1)}
    tile1, tile0, vec1, vec0 = got[1, -1], got[0, -1], got[1, 0], got[0, 0]
    assert np.array_equal(tile1[0], tile0[0]) and np.array_equal(tile1[0], tile1[2])  # tile rows: the same bits, the single call's too
    for c in slots:
        assert np.array_equal(tile1[1][c], tile0[1][c])
    ev = np.max(np.abs(vec1[0] - vec0[0]) / np.abs(vec0[0]))
    es = np.max(np.abs(vec1[0] - vec1[2]) / np.abs(vec1[2]))
    print(f"n={n}: loss, vector right-hand side: rows_pair 1 against 0 {ev:.2e}, against the single calls {es:.2e} (allowed 1e-14)")
    assert ev <= 1e-14 and es <= 1e-14
    for c in slots:
        v, ls, s = hypers(c)
        th = thetas_of(CELLS)[c]
        ref = oex.loss("RBF", x, y[:, c], float(th[0]), float(th[1]), float(th[2]))
        rm, _ = oex.predict("RBF", x, y[:, c], v, ls, s, vec1[3])
        for name, res in (("vector", vec1), ("tile rows", tile1)):
            el, em = abs(res[0][c] - ref) / abs(ref), np.max(np.abs(res[1][c] - rm)) / np.max(np.abs(rm))
            print(f"n={n} cell {c} {name}: loss {el:.2e} from the oracle (allowed 1e-9), mean {em:.2e} (allowed 1e-8)")
            assert el <= 1e-9 and em <= 1e-8


def test_23_cells_do_not_see_the_key(lib):
    """One cell below the threshold the panel is fused: the key changes nothing, bit for bit."""
    n = 300
    unset = batch_losses(lib, n, CELLS - 1, {})
    for pair in (1, 0):
        with_key = batch_losses(lib, n, CELLS - 1, {"rows_pair": pair})
        assert np.array_equal(unset[0], with_key[0]) and np.array_equal(unset[2], with_key[2]), pair
    assert np.array_equal(unset[0], unset[2])  # (and the batch is its single calls)


@pytest.mark.parametrize("row,why", [(10, "left panel of the pair"), (70, "right panel of the pair"), (100, "right panel, past its first sub-panels"),
                                     (150, "the lone panel behind the pair")])
def test_an_indefinite_cell_reports_the_same_pivot(lib, row, why):
    """n = 192, cell 5 with a negative diagonal entry (as test_gpu_potrf_batched.py makes its failing cell): the 1-based pivot index is
    the one "rows_pair" = 0 reports, and the other cells keep their bits."""
    n, cell, col_base = 192, 5, 1000
    mats, ys = inputs(n)
    bad = list(mats)
    bad[cell] = mats[cell].copy()
    bad[cell][row, row] = -1.0
    infos, outs = {}, {}
    for pair in (1, 0):
        with rows_pair(lib, pair):
            outs[pair], infos[pair] = pb.factorise(lib, bad, tile_rows(ys), route=1, extra=NB, col_base=col_base, expect=_lib.GPRX_ENOTPD, unchecked=(cell,))
    expected = [col_base + row + 1 if c == cell else 0 for c in range(CELLS)]
    assert list(infos[1]) == list(infos[0]) == expected, (why, list(infos[1]), list(infos[0]))
    for c in range(CELLS):
        if c != cell:
            pb.assert_same_cell(outs[1][c], outs[0][c], f"cell {c} beside an indefinite cell ({why}): rows_pair 1 against 0")
