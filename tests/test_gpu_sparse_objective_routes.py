"""Every route of the sparse model's loss and gradient (csrc/sgpr_fused.h, gp_sparse.h, sgpr_held.hip, sgpr_asm.h) through the C ABI against
the longdouble objective of tests/sparse_objective_reference.py: the five fused launches for a lone model and for a batch, the launch
sequence at M <= 64 and at M > 64 -- eager, captured and replayed --, 24 cells (the split panel of the batched Cholesky), d = 70 (the
hyperparameters in the launch arguments), the masks, held-out rows on both routes, inducing points ON training rows, and two
ill-conditioned models that a block-maximum measure cannot carry.  Every error is measured on the natural scale of its own number (the
loss's terms, each hyperparameter component's and each Z entry's own sum of magnitudes) and may be 8 x what a float64 restatement of the
device's algebra reaches on the same data (tests/golden/sparse_objective_bounds.json); every comparison prints `error / recorded ratio`
first, and every test closes with the largest share of the 8 x it used."""

import ctypes as C

import numpy as np
import pytest

import sparse_objective_reference as sr
from gpras_amd import _lib
from gpras_amd._lib import check, ptr

pytestmark = pytest.mark.gpu

ALL = sr.ALL
DP = C.POINTER(C.c_double)
USED = {}  # route -> the largest error / recorded ratio seen


class Sparse:
    """A handle on one case's data with the case's distance form and the given tuning; destroyed on exit."""

    def __init__(self, lib, cid, **tuning):
        c = sr.CASES[cid]
        x, y, zs = sr.data(cid)
        self.lib, self.cid, self.case = lib, cid, c
        self.x, self.y, self.zs = np.ascontiguousarray(x), np.ascontiguousarray(y), np.ascontiguousarray(zs)
        self.thetas, self.units = np.ascontiguousarray(sr.thetas(cid)), sr.units(cid)
        self.nt, self.width = c.nlen + 2, c.nlen + 2 + c.m * c.d
        self.h = C.c_void_p()
        check(lib.gprx_create(0, c.n, c.d, c.m, sr.KERNEL_IDS[c.kernel], int(c.ard), C.byref(self.h)))
        check(lib.gprx_set_data(self.h, ptr(self.x), ptr(self.y), self.y.shape[1]), self.h)
        check(lib.gprx_set_distance_form(self.h, _lib.DISTANCE_FORMS[c.form]), self.h)
        for key, value in tuning.items():
            check(lib.gprx_set_handle_tuning(self.h, key.encode(), value), self.h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.gprx_destroy(self.h)

    def lone(self, cell, mask=ALL):
        """gprx_objective of one cell: (loss, grad), both written into canary-filled buffers."""
        theta, z = np.ascontiguousarray(self.thetas[cell]), np.ascontiguousarray(self.zs[cell])
        loss, grad = sr.canary(1), sr.canary(self.width)
        check(self.lib.gprx_objective(self.h, int(self.units[cell]), ptr(theta), ptr(z), mask, loss.ctypes.data_as(DP), ptr(grad)), self.h)
        return loss[0], grad

    def batch(self, cells=None, mask=ALL, held=False):
        """gprx_objective_batch (held: gprx_objective_batch_held with the case's ranges) of the given cells, default all: (losses, grads)."""
        cells = list(range(self.case.cells)) if cells is None else list(cells)
        units, thetas, zs = (np.ascontiguousarray(a[cells]) for a in (self.units, self.thetas, self.zs))
        losses, grads = sr.canary(len(cells)), sr.canary((len(cells), self.width))
        if held:
            lo, hi = (np.ascontiguousarray([self.case.holds[c][j] for c in cells], dtype=np.int64) for j in (0, 1))
            check(self.lib.gprx_objective_batch_held(self.h, len(cells), ptr(units), ptr(thetas), ptr(zs), mask, ptr(losses), ptr(grads), ptr(lo),
                                                     ptr(hi)), self.h)
        else:
            check(self.lib.gprx_objective_batch(self.h, len(cells), ptr(units), ptr(thetas), ptr(zs), mask, ptr(losses), ptr(grads)), self.h)
        return losses, grads


def hold(route, loss, grad, cid, cell, what, mask=ALL):
    """Loss, every hyperparameter component and every entry of Z of one cell against the longdouble reference, each on its natural scale
    under 8 x the recorded ratio; no canary survives; untrained components exactly 0.0."""
    c = sr.CASES[cid]
    grad = np.asarray(grad)
    nt = c.nlen + 2
    assert not np.any(sr.is_canary(np.array([loss]))) and not np.any(sr.is_canary(grad)), f"{what}: an output nobody wrote"
    assert not np.isnan(loss) and not np.any(np.isnan(grad)), f"{what}: NaN"
    on = np.concatenate([sr.trained(mask, c.nlen), np.full(c.m * c.d, bool(mask & sr.TRAIN_Z))])
    assert np.all(grad[~on] == 0.0), f"{what}: an untrained component is not exactly 0"
    got = sr.ratios(loss, grad[:nt], grad[nt:].reshape(c.m, c.d), cid, cell, mask)
    used = {q: val / sr.recorded(cid, cell, mask, q) for q, val in got.items()}
    worst = max(used, key=used.get)
    print(f"{what} [{cid}/c{cell}/m{mask}]: loss {got['loss']:.3e} = {used['loss']:.2f} x ratio, worst {worst} {got[worst]:.3e} = {used[worst]:.2f} x ratio")
    USED[route] = max(USED.get(route, 0.0), used[worst])
    for q, val in used.items():
        assert val <= sr.MARGIN, f"{what}: {q} off by {got[q]:.3e} of its scale, allowed {sr.MARGIN * sr.recorded(cid, cell, mask, q):.3e}"


def hold_batch(route, losses, grads, cid, what, cells=None, mask=ALL):
    assert not np.any(sr.is_canary(losses)) and not np.any(sr.is_canary(grads)), f"{what}: an output nobody wrote"
    for i, cell in enumerate(range(sr.CASES[cid].cells) if cells is None else cells):
        hold(route, losses[i], grads[i], cid, cell, f"{what}, cell {cell}", mask)


def report(route):
    print(f"route {route}: used {USED.get(route, 0.0):.2f} of {sr.MARGIN:.0f} x recorded")


def bits(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist() for a in arrays]


def same_bits(a, b):
    return bits(*a) == bits(*b)


def lone_bits_equal_the_batch(model, losses, grads, cells, mask=ALL):
    for i, cell in enumerate(cells):
        assert same_bits(model.lone(cell, mask), (losses[i], grads[i])), (model.cid, cell)


# ---- 1, 2: the five fused launches --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sr.ROUTES["fused_lone"])
def test_fused_lone_model_against_longdouble(lib, cid):
    """gprx_objective at M <= 64 on every (kernel, class) pair of the fused table -- every NP variant of the two passes, M = 1 .. 64,
    N < M, one to three chunks -- and on the ill-conditioned RBF model at d = 3."""
    with Sparse(lib, cid) as m:
        for cell in range(m.case.cells):
            hold("fused_lone", *m.lone(cell), cid, cell, f"lone, cell {cell}")
    report("fused_lone")


@pytest.mark.parametrize("cid", sr.ROUTES["fused_batch"])
def test_fused_batch_against_longdouble_and_lone_bits(lib, cid):
    """gprx_objective_batch on the same cases: three cells of different theta and Z with the units reversed, each against its own
    reference; a cell evaluated alone gives the batch's bits."""
    with Sparse(lib, cid) as m:
        losses, grads = m.batch()
        hold_batch("fused_batch", losses, grads, cid, "batch")
        lone_bits_equal_the_batch(m, losses, grads, range(m.case.cells))
    report("fused_batch")


# ---- 3, 4: the launch sequence ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sr.ROUTES["sequence_small"])
def test_launch_sequence_at_64_or_fewer_inducing_points(lib, cid):
    """"sgpr_fused" = 0: the launch sequence of gp_sparse.h with one 64 x 64 block (sgpr_small_kernel) on three fused cases."""
    with Sparse(lib, cid, sgpr_fused=0) as m:
        losses, grads = m.batch()
        hold_batch("sequence_small", losses, grads, cid, "batch")
        lone_bits_equal_the_batch(m, losses, grads, range(m.case.cells))
    report("sequence_small")


@pytest.mark.parametrize("cid", sr.ROUTES["sequence_general"])
def test_launch_sequence_above_64_inducing_points_eager_captured_replayed(lib, cid):
    """M > 64 on every (kernel, class) pair of the general table -- both sides of mp = 128, two row chunks, N < M, split-K -- and on the
    ill-conditioned Matern52 model: the same (cells, gradient) shape three times with fresh canaries (the first call goes out eagerly,
    the second is captured, the third replayed), each held to the reference and all three the same bits; then gprx_objective per cell,
    to the reference and to the batch's bits."""
    with Sparse(lib, cid) as m:
        seen = []
        for call in ("eager", "captured", "replayed"):
            losses, grads = m.batch()
            hold_batch("sequence_general", losses, grads, cid, call)
            seen.append((losses, grads))
        assert same_bits(seen[1], seen[0]) and same_bits(seen[2], seen[0])
        for cell in range(m.case.cells):
            loss, grad = m.lone(cell)
            hold("sequence_general", loss, grad, cid, cell, f"lone, cell {cell}")
            assert same_bits((loss, grad), (seen[0][0][cell], seen[0][1][cell])), cell
    report("sequence_general")


# ---- 5, 6: many cells, many dimensions ---------------------------------------------------------------------------------------------------
def test_24_cells_take_the_split_panel(lib):
    """From 24 cells on the batched Cholesky factorises with the split panel (potrf.h): M = 65, N = 257, every cell to its reference; the
    first and the last cell alone give the batch's bits."""
    with Sparse(lib, "C24") as m:
        losses, grads = m.batch()
        hold_batch("cells24", losses, grads, "C24", "24 cells")
        for cell in (0, 23):
            assert same_bits(m.lone(cell), (losses[cell], grads[cell])), cell
    report("cells24")


def test_more_lengthscales_than_the_parameter_table_holds(lib):
    """d = 70, ARD: the hyperparameters travel in the launch arguments and the cells of a batch run one at a time -- a lone call and a
    3-cell batch, each cell to its reference, the batch's cells the bits of lone calls."""
    with Sparse(lib, "D70") as m:
        loss, grad = m.lone(1)
        hold("wide", loss, grad, "D70", 1, "lone, cell 1")
        losses, grads = m.batch()
        hold_batch("wide", losses, grads, "D70", "batch")
        assert same_bits((loss, grad), (losses[1], grads[1]))
    report("wide")


# ---- 7: masks -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sr.ROUTES["masks"])
def test_masks(lib, cid):
    """15, 8, 7 and each single bit on one fused and one general case, against sparse_objective_ld(mask): the priors enter the loss and the
    gradient for trained parameters only (bounds recorded per mask), untrained components are exactly 0.0 (hold() asserts it)."""
    with Sparse(lib, cid) as m:
        for mask in sr.MASKS:
            losses, grads = m.batch(mask=mask)
            hold_batch("masks", losses, grads, cid, f"mask {mask}", mask=mask)
            hold("masks", *m.lone(0, mask), cid, 0, f"mask {mask}, lone", mask)
    report("masks")


# ---- 8: held-out rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,tuning", [("H-fused", {}), ("H-general", {"held_general": 1})])
def test_held_rows_against_the_model_on_the_kept_rows(lib, cid, tuning):
    """gprx_objective_batch_held on the fused launches and, with "held_general" = 1, on the launch sequence: the cells hold a prefix, a
    suffix, a middle range across the 256-column chunk edge, a single row and nothing; the reference and the recorded bound of a cell
    are those of the model on the rows it keeps.  The cell that holds nothing gives the bits of the call without ranges."""
    with Sparse(lib, cid, **tuning) as m:
        losses, grads = m.batch(held=True)
        hold_batch("held", losses, grads, cid, "held")
        nothing = [i for i, (lo, hi) in enumerate(m.case.holds) if lo == hi]
        plain = m.batch(cells=nothing)
        assert same_bits(plain, (losses[nothing], grads[nothing]))
    report("held")


# ---- 9: coincident inducing points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sr.ROUTES["coincident"])
def test_inducing_points_on_training_rows(lib, cid):
    """Every other inducing point IS a training row (exactly: the data are on the 2^-20 grid), as k-means with many centres leaves them:
    r2 = 0 off the diagonal of Kuf, where the convention is h = 0 (csrc/kfun.h) -- for every kernel, in the difference form."""
    with Sparse(lib, cid) as m:
        hold("coincident", *m.lone(0), cid, 0, "lone")
        losses, grads = m.batch()
        hold_batch("coincident", losses, grads, cid, "batch")
    report("coincident")
