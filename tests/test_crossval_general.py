"""The case table of tests/test_gpu_crossval_general.py and the host logic of route="held_general", without a GPU.

The GPU parity tests compare the held forms on the general launch sequence against the oracle on the KEPT rows of every cell; here the
preconditions of that comparison on all 48 cells -- Kuf away from underflow, Kuu well conditioned, and every non-empty hold moving the
oracle's loss by far more than the parity tolerance, so that a mask that did nothing would not pass.
"""

import numpy as np
import pytest

import crossval_cases as cc
import crossval_general_cases as gc
from gpras_amd import _lib, crossval


@pytest.mark.parametrize("case", gc.CASES, ids=[c["id"] for c in gc.CASES])
def test_every_cell_is_well_posed_on_its_kept_rows(case):
    """Median of Kuf / variance >= 0.05 and cond(Kuu + 1e-6 I) <= 1e6 for all eight cells, each on the rows it keeps."""
    x, y, thetas, zs, units, variance, ls, noise = cc.draw_inputs(case)
    assert x.shape == (case["n"], case["d"]) and zs.shape == (gc.CELLS, case["m"], case["d"])
    for c, hold in enumerate(gc.holds_for(case["n"])):
        keep = gc.keep_rows(case, c)
        assert keep.size == case["n"] - (hold[1] - hold[0]) and keep.size >= 1
        med, cond = cc.preconditions(case, x[keep], zs[c], variance[c], ls[c])
        print(case["id"], c, med, cond)
        assert med >= 0.05, (c, med)
        assert cond <= 1e6, (c, cond)


@pytest.mark.parametrize("case", gc.CASES, ids=[c["id"] for c in gc.CASES])
def test_every_hold_moves_the_loss(case):
    """For every non-empty hold the oracle's loss on the kept rows differs from the loss on all rows by at least 1e-3 relative (1e6 parity
    tolerances); the empty hold keeps every row."""
    x, y, thetas, zs, units, *_ = cc.draw_inputs(case)
    for c, hold in enumerate(gc.holds_for(case["n"])):
        kept_loss, _ = gc.ref_cell(case, c)
        if hold[0] == hold[1]:
            assert gc.keep_rows(case, c).size == case["n"]
            continue
        full_loss, _ = cc.ref_eval(case, x, y[:, units[c]], zs[c], thetas[c])
        print(case["id"], c, abs(kept_loss - full_loss) / abs(full_loss))
        assert abs(kept_loss - full_loss) >= 1e-3 * abs(full_loss), (c, kept_loss, full_loss)


def test_the_case_table_reaches_what_it_claims():
    assert [c["seed"] for c in gc.CASES] == [200, 201, 202, 203, 204, 205]
    assert [(c["m"], c["n"]) for c in gc.CASES] == [(50, 600), (100, 600), (65, 600), (130, 1100), (300, 1100), (129, 1100)]
    mp = [-(-c["m"] // 64) * 64 for c in gc.CASES]
    assert mp == [64, 128, 128, 192, 320, 192]  # one block; b-finish; add-diag from 192 on
    assert [c["unfused"] for c in gc.CASES] == [True, False, False, False, False, False]
    np_ = [-(-c["n"] // 64) * 64 for c in gc.CASES]
    assert {p >= 1024 for p in np_} == {True, False} and 1152 % 256 != 0  # both GEMM routes; a partial last split-K chunk
    assert {c["form"] for c in gc.CASES} == {0, 1} and {c["ard"] for c in gc.CASES} == {True, False}
    assert max(c["d"] for c in gc.CASES) > 8  # more than one staging pass of the build (KM_DC = 8)
    for c in gc.CASES:
        holds = gc.holds_for(c["n"])
        assert len(holds) == gc.CELLS == c["cells"]
        assert holds[gc.EMPTY_CELL] == (300, 300) and holds[gc.SUFFIX_CELL] == (c["n"] - 37, c["n"])
        assert holds[3] == (256, 512) and c["n"] - (holds[6][1] - holds[6][0]) == 5
    assert [c["m"] for c in gc.RESIDENT_CASES] == [100, 130]


def test_held_general_route_applicability():
    assert crossval.held_general_applies(100, 10, "adam") is None
    assert crossval.held_general_applies(320, 64, "two-stage") is None
    assert crossval.held_general_applies(65, 1, "adadelta") is None
    assert "inducing" in crossval.held_general_applies(64, 10, "adam")
    assert "inducing" in crossval.held_general_applies(321, 10, "adam")
    assert "features" in crossval.held_general_applies(100, 65, "adam")
    assert "exact" in crossval.held_general_applies(None, 10, "adam")
    assert "L-BFGS-B" in crossval.held_general_applies(100, 10, "L-BFGS-B")
    # held_applies is what it was
    assert crossval.held_applies(64, 64, "adam") is None and "inducing" in crossval.held_applies(65, 10, "adam")
    assert "held_general" in crossval.ROUTES and "held_general" in _lib.TUNING_KEYS


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", refuse)


def _data(n=400, d=3, k=2):
    rng = np.random.default_rng(0)
    return rng.standard_normal((n, d)), rng.standard_normal((n, k))


@pytest.mark.parametrize("kw, d, why", [
    (dict(n_inducing=64), 3, "inducing points"),
    (dict(n_inducing=321), 3, "inducing points"),
    (dict(n_inducing=100), 65, "features"),
    (dict(n_inducing=None), 3, "exact"),
    (dict(n_inducing=100, optimization_method="L-BFGS-B"), 3, "L-BFGS-B"),
])
def test_held_general_refusals_raise_before_any_library_call(no_library, kw, d, why):
    x, y = _data(d=d)
    with pytest.raises(ValueError, match=why):
        crossval.cross_validate("RBF", x, y, events=[(0, 100), (100, 400)], route="held_general", **kw)


def test_auto_still_runs_the_engines_route_above_64_inducing_points(no_library):
    x, y = _data()
    *_, use = crossval._checked("RBF", x, y, [(0, 100), (100, 400)], 100, "kmeans", "adam", "auto", None)
    assert use == "engines"
    *_, use = crossval._checked("RBF", x, y, [(0, 100), (100, 400)], 100, "kmeans", "adam", "held_general", None)
    assert use == "held_general"
    *_, use = crossval._checked("RBF", x, y, [(0, 100), (100, 400)], 50, "kmeans", "adam", "auto", None)
    assert use == "held"
