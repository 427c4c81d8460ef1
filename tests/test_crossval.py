"""The case table of tests/test_gpu_crossval.py and the host logic of gpras_amd.crossval, without a GPU.

The GPU parity test compares the held-out forms against the oracle on the KEPT rows of every cell; that comparison is only as good as its
inputs.  Here: the preconditions of the existing parity test (test_gpu_sparse_variants) on every cell's kept rows, and that holding the
rows out moves the loss by far more than the parity tolerance -- a mask that did nothing would not pass.
"""

import numpy as np
import pytest

import crossval_cases as cc
from gpras_amd import _lib, crossval


@pytest.mark.parametrize("case", cc.CASES, ids=[c["id"] for c in cc.CASES])
def test_every_cell_is_well_posed_on_its_kept_rows(case):
    """Median of Kuf / variance in [0.02, 0.95] and cond(Kuu + 1e-6 I) <= 1e6 for all eight cells, each on the rows it keeps."""
    x, y, thetas, zs, units, variance, ls, noise = cc.draw_inputs(case)
    assert x.shape == (cc.N, case["d"]) and zs.shape == (cc.CELLS, case["m"], case["d"])
    for c, hold in enumerate(cc.HOLDS):
        keep = cc.keep_rows(hold)
        assert keep.size == cc.N - (hold[1] - hold[0]) and keep.size >= 1
        med, cond = cc.preconditions(case, x[keep], zs[c], variance[c], ls[c])
        assert 0.02 <= med <= 0.95, (c, med)
        assert cond <= 1e6, (c, cond)


@pytest.mark.parametrize("case", cc.CASES, ids=[c["id"] for c in cc.CASES])
def test_every_hold_moves_the_loss(case):
    """For every non-empty hold the oracle's loss on the kept rows differs from the loss on all rows by more than 1e-3 relative (1e6
    parity tolerances); the empty hold keeps every row."""
    x, y, thetas, zs, units, *_ = cc.draw_inputs(case)
    for c, hold in enumerate(cc.HOLDS):
        kept_loss, _ = cc.ref_cell(case, c)
        if hold[0] == hold[1]:
            assert cc.keep_rows(hold).size == cc.N
            continue
        full_loss, _ = cc.ref_eval(case, x, y[:, units[c]], zs[c], thetas[c])
        assert abs(kept_loss - full_loss) > 1e-3 * abs(full_loss), (c, kept_loss, full_loss)


def test_the_case_table_reaches_what_it_claims():
    nps = {6 if c["d"] <= 12 else (8 if c["d"] <= 16 else 0) for c in cc.CASES}
    assert nps == {6, 8, 0}
    assert {int(not c["ard"] and c["form"] == 0) for c in cc.CASES} == {0, 1}
    assert {c["form"] for c in cc.CASES} == {0, 1}
    assert max(c["d"] for c in cc.CASES) > 16 and all(c["m"] <= 64 for c in cc.CASES)
    assert [c["seed"] for c in cc.CASES] == [100, 101, 102, 103, 104]
    assert cc.HOLDS[cc.SUFFIX_CELL] == (563, cc.N) and cc.HOLDS[cc.EMPTY_CELL] == (300, 300)
    assert cc.N // 256 == 2 and cc.N % 256 != 0  # three chunks, the last one partial


def test_fold_cells_are_fold_major():
    cells = crossval.fold_cells(3, 2)
    assert cells == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]
    for i, (e, k) in enumerate(crossval.fold_cells(35, 10)):
        assert i == e * 10 + k
    assert crossval.fold_cells(0, 4) == []


def test_held_route_applicability():
    assert crossval.held_applies(50, 10, "two-stage") is None
    assert crossval.held_applies(64, 64, "adam") is None
    assert "exact" in crossval.held_applies(None, 10, "adam")
    assert "inducing" in crossval.held_applies(65, 10, "adam")
    assert "features" in crossval.held_applies(50, 65, "adam")
    assert "L-BFGS-B" in crossval.held_applies(50, 10, "L-BFGS-B")


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", refuse)


def _data(n=40, d=3, k=2):
    rng = np.random.default_rng(0)
    return rng.standard_normal((n, d)), rng.standard_normal((n, k))


GOOD = dict(events=[(0, 10), (10, 40)], n_inducing=8)


@pytest.mark.parametrize("kw, why", [
    (dict(events=[(0, 5), (3, 8)]), "sorted"),
    (dict(events=[(5, 8), (0, 3)]), "sorted"),
    (dict(events=[(0, 3), (3, 3)]), None),
    (dict(events=[0] * 10 + [1] * 10 + [0] * 20), "contiguous"),
    (dict(events=[(0, 40)]), "every row"),
    (dict(events=[]), None),
    (dict(route="fast"), "route"),
    (dict(optimization_method="sgd"), "optimization_method"),
    (dict(inducing_initializer="random"), "initializer"),
    (dict(n_inducing=0), "n_inducing"),
    (dict(n_inducing=2.5), "n_inducing"),
    (dict(route="held", n_inducing=70), "inducing points"),
    (dict(route="held", n_inducing=None), "exact"),
    (dict(route="held", optimization_method="L-BFGS-B"), "L-BFGS-B"),
])
def test_argument_errors_raise_before_any_library_call(no_library, kw, why):
    x, y = _data()
    args = dict(GOOD, **kw)
    with pytest.raises(ValueError, match=why):
        crossval.cross_validate("RBF", x, y, **args)


def test_more_argument_errors_before_any_library_call(no_library):
    x, y = _data()
    with pytest.raises(ValueError, match="kernel"):
        crossval.cross_validate("Linear", x, y, **GOOD)
    with pytest.raises(ValueError, match="kernel"):
        crossval.cross_validate("Cubic", x, y, **GOOD)
    with pytest.raises(ValueError, match="matching N"):
        crossval.cross_validate("RBF", x, y[:-1], **GOOD)
    xw, yw = _data(d=65)
    with pytest.raises(ValueError, match="features"):
        crossval.cross_validate("RBF", xw, yw, route="held", **GOOD)

    class _Unfitted:
        models = []

    with pytest.raises(ValueError, match="start"):
        crossval.cross_validate("RBF", x, y, start=_Unfitted(), **GOOD)


def test_gpras_cross_validate_needs_a_fit(no_library):
    from gpras_amd.gpr import GPRAS

    with pytest.raises(ValueError, match="fit"):
        GPRAS("RBF").cross_validate([(0, 10)])
