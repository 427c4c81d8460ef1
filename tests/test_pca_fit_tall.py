"""The covariance route of PreProcessor.fit, on the CPU: the numpy restatement against the reference's own fit on more samples than
wet cells (tests/golden/pca_fit_tall_ref_golden.npz), the order in which numpy sums a long contiguous column (which the device
replays for ``input_mean``), and the argument checks that run before any device work."""

import os
import sys

import numpy as np
import pytest

from gpras_amd.preprocess import PreProcessor, check_fit_args
from pca_fit_tall_numpy import assert_tall_fit_close, chunked_pairwise_sum, fit_reference_tall, single_tree_sum

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_pca_fit_ref import THRESHOLD  # noqa: E402
from make_golden_pca_fit_tall_ref import pca_fit_tall_ref_cases  # noqa: E402

FIX = np.load(os.path.join(GOLDEN, "pca_fit_tall_ref_golden.npz"))
CASES = pca_fit_tall_ref_cases()
KEYS = ("wetness_classes", "input_mean", "weights", "eofs", "eigenvalues", "spatial_mode_count", "n_samples_fit", "x_mean", "x_std", "transform")


def fixture_fit(name):
    return {a: FIX[f"{name}/{a}"] for a in KEYS if f"{name}/{a}" in FIX.files}


def test_fixture_covers_the_kinds_of_tall_input():
    kinds = {c["kind"] for c in CASES.values()}
    assert kinds == {"plus1", "onebatch", "twobatch", "manybatch", "deep"}
    for name, c in CASES.items():
        n_s, n_wet = c["x"].shape[0], c["n_wet"]
        assert n_s > n_wet and n_wet % 16 != 0
        assert FIX[f"{name}/eigenvalues"].shape == (n_wet,) and int(FIX[f"{name}/n_samples_fit"]) == n_s
        want = {"plus1": n_s == n_wet + 1, "onebatch": n_wet < n_s <= 5 * n_wet, "twobatch": n_s == 5 * n_wet + 1, "manybatch": n_s > 10 * n_wet,
                "deep": c["x"].shape == (8201, 29)}
        assert want[c["kind"]], name
    assert "wse_u_k_deep/transform" not in FIX.files


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_reference(name):
    c = CASES[name]
    got = fit_reference_tall(c["x"], c["elevations"], c["weights"], c["k"], c["mode"], THRESHOLD)
    fig = {}
    try:
        assert_tall_fit_close(got, fixture_fit(name), report=fig)
    finally:
        print(name, fig)


@pytest.mark.parametrize("n", [129, 1031, 8192, 8193, 16385, 20001])
def test_numpy_sums_a_long_column_in_pieces_of_8192(n):
    rng = np.random.default_rng(n)
    x = np.asfortranarray(11.0 + rng.standard_normal((n, 3)) * np.array([1.0, 1e-3, 40.0]))
    want = x.mean(axis=0)
    for j in range(3):
        assert chunked_pairwise_sum(x[:, j]) / n == want[j], (n, j)
    if n <= 8192:  # one piece: the single tree of the Gram route is the same order
        assert all(single_tree_sum(x[:, j]) == chunked_pairwise_sum(x[:, j]) for j in range(3))


def test_beyond_one_piece_a_single_tree_is_another_order():
    rng = np.random.default_rng(5)
    x = np.asfortranarray(11.0 + rng.standard_normal((20001, 16)))
    assert any(single_tree_sum(x[:, j]) != chunked_pairwise_sum(x[:, j]) for j in range(16))


def test_check_fit_args_allow_tall_lifts_only_the_sample_bound():
    x = np.ones((11, 10))
    elev = np.zeros(10)
    with pytest.raises(ValueError):
        check_fit_args(x, elev, None, None, "wse")
    xc, ec, wc = check_fit_args(x, elev, None, 10, "wse", allow_tall=True)
    assert xc.shape == (11, 10) and wc is None
    with pytest.raises(ValueError):
        check_fit_args(np.ones((30, 10)), elev, None, 11, "wse", allow_tall=True)  # k <= min(n_samples - 1, n_cells)
    with pytest.raises(ValueError):
        check_fit_args(np.ones((1, 10)), elev, None, None, "wse", allow_tall=True)
    with pytest.raises(ValueError):
        check_fit_args(x, None, None, None, "wse", allow_tall=True)  # the other checks stay
    with pytest.raises(ValueError):
        check_fit_args(x, elev, np.ones(9), None, "wse", allow_tall=True)


def test_unknown_sample_route_raises_before_device_work(monkeypatch):
    import gpras_amd._lib as lib_mod

    def no_device():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(lib_mod, "load", no_device)
    pre = PreProcessor(hydraulic_parameter="velocity")
    assert PreProcessor.sample_route == "gram" and pre.last_route is None
    pre.sample_route = "covariance"
    with pytest.raises(ValueError, match="sample_route"):
        pre.fit(np.ones((11, 10)), None)
    pre.sample_route = "gram"
    with pytest.raises(ValueError, match="samples <= cells"):
        pre.fit(np.ones((11, 10)), None)
