"""Host logic of gpras_amd/diagnostics.py and the numpy restatement of its kernels (tests/diag_numpy.py), without a GPU.

Bounds.  The sum of squares in the device's order against ``math.fsum`` of the same rounded squares: every term is non-negative and the
longest path of the tree has D(n) additions (csrc/diag.h), each with a relative error of at most 2^-53, so the sum lies within
D * 2^-53 relative to first order; (D + 1) * 2^-53 leaves room for the second-order terms and for fsum's own rounding.  The rmse is
sqrt(S / n): the division and the square root add 2^-53 each and the square root halves the error of S, hence half the bound of the
sum plus 2^-52.
"""

import math
import os
import sys

import numpy as np
import pandas as pd
import pytest

import diag_numpy
from gpras_amd import diagnostics as dg

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_diag_ref import DETECT_EVENTS, DETECT_THRESHOLDS, FIELD_SHAPES, detect_index, diag_ref_cases, input_checksums  # noqa: E402

FIX = np.load(os.path.join(GOLDEN, "diag_ref_golden.npz"))
FIELDS, DETECT = diag_ref_cases()
RANGES = [(lo, hi) for _, lo, hi in DETECT_EVENTS]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64)[~np.isnan(b)], b.view(np.int64)[~np.isnan(b)]) and np.array_equal(np.isnan(a), np.isnan(b))


# ---- ranks and percentages -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 10, 2047, 2048, 2049, 70001])
@pytest.mark.parametrize("n_points", [1, 2, 7, 2048])
def test_ranks_are_the_rounded_linspace_and_pcts_the_reference_linspace(n, n_points):
    ranks = dg.cdf_ranks(n, n_points)
    assert ranks.dtype == np.int64
    if n_points >= n:
        assert np.array_equal(ranks, np.arange(n))
    else:
        assert np.array_equal(ranks, np.linspace(0, n - 1, n_points).round().astype(np.int64))
        assert ranks.size == n_points and ranks[0] == 0 and (n_points == 1 or ranks[-1] == n - 1)
    assert np.all(np.diff(ranks) >= 0) and ranks.min() >= 0 and ranks.max() <= n - 1
    assert np.array_equal(dg.cdf_pcts(n, ranks), np.linspace(0, 100, n)[ranks])


def test_n_points_equal_to_n_and_above_give_the_whole_curve():
    for n_points in (5, 6, 500):
        assert np.array_equal(dg.cdf_ranks(5, n_points), np.arange(5))
    assert np.array_equal(dg.cdf_ranks(5, 1), [0])
    with pytest.raises(ValueError):
        dg.cdf_ranks(5, 0)
    with pytest.raises(ValueError):
        dg.cdf_ranks(0, 5)


# ---- events ------------------------------------------------------------------------------------------------------------------------------
def test_event_ranges_follow_the_two_level_index():
    index = pd.MultiIndex.from_tuples(detect_index())
    names, ranges = dg.event_ranges(index)
    assert names == [n for n, _, _ in DETECT_EVENTS] and ranges == RANGES
    index = pd.MultiIndex.from_tuples([("b", 0), ("b", 1), ("a", 0)])
    assert dg.event_ranges(index) == (["b", "a"], [(0, 2), (2, 3)])  # first appearance, not sorted


def test_non_contiguous_events_are_refused_like_export_metric_summary():
    index = pd.MultiIndex.from_tuples([("a", 0), ("b", 0), ("a", 1)])
    with pytest.raises(ValueError, match=r"the rows of event 'a' are not contiguous in hf_test_data_df \(sort the index by event first\)"):
        dg.event_ranges(index)


def test_row_ranges_are_checked_before_anything_goes_up():
    lo, hi = dg.check_ranges([(0, 1), (1, 20)], 20)
    assert lo.dtype == hi.dtype == np.int64 and lo.tolist() == [0, 1] and hi.tolist() == [1, 20]
    for bad in ([], [(0, 0)], [(-1, 2)], [(3, 2)], [(0, 21)]):
        with pytest.raises(ValueError):
            dg.check_ranges(bad, 20)
    fd = dg.FieldDiagnostics()
    with pytest.raises(ValueError):  # no device is touched: the handle is created at its first use
        fd.detection_categories(np.zeros((4, 3)), np.zeros((4, 3)), [(0, 5)])
    with pytest.raises(ValueError):
        fd.detection_categories(np.zeros((4, 3)), np.zeros((4, 2)), [(0, 4)])


def test_category_names_are_the_reference_strings():
    assert dg.CATEGORY_NAMES == ("", "Detected", "Miss", "False Alarm", "Correct Negative") == diag_numpy.CATEGORY_NAMES
    assert dg.DG_SUM_CHUNK == diag_numpy.SUM_CHUNK
    for n in (1, 8192, 8193, 8192 * 256 + 1, 140_000_000):
        assert dg.sum_depth(n) == diag_numpy.sum_depth(n)
    assert dg.sum_depth(1) == 51 and dg.sum_depth(8192 * 256 + 1) == 52


def test_the_constants_follow_the_header():
    with open(os.path.join(os.path.dirname(dg.__file__), "csrc", "diag.h")) as f:
        text = f.read()
    assert "DG_KPT = 16;" in text and "DG_TILE = DG_NT * DG_KPT;" in text and "DG_NT = 256;" in text and dg.DG_TILE == 256 * 16
    assert f"DG_RT = {dg.DG_RT};" in text
    assert "DG_SUM_PT = 32;" in text and dg.DG_SUM_CHUNK == 256 * 32


# ---- the summation order -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 255, 256, 257, 8191, 8192, 8193, 70001, 8192 * 256 + 5])
def test_sum_of_squares_in_the_device_order_against_fsum(n):
    rng = np.random.default_rng(n)
    p, hf = 100.0 + rng.normal(size=n), 100.0 + rng.normal(size=n)
    r = p - hf
    exact = math.fsum((r * r).tolist())
    got = diag_numpy.sum_sq(p, hf)
    bound = (diag_numpy.sum_depth(n) + 1) * 2.0**-53
    rel = abs(got - exact) / exact
    print(f"n = {n}: relative error of the sum {rel:.3e}, bound {bound:.3e}")
    assert rel <= bound
    rmse_exact = math.sqrt(exact / n)
    rel = abs(diag_numpy.scatter_summary(p, hf)["rmse"] - rmse_exact) / rmse_exact
    print(f"n = {n}: relative error of the rmse {rel:.3e}, bound {0.5 * bound + 2.0**-52:.3e}")
    assert rel <= 0.5 * bound + 2.0**-52


def test_padding_slots_do_not_enter_the_sum():
    p, hf = np.array([3.0, 1.0, -2.0]), np.array([1.0, 1.0, 2.0])
    assert diag_numpy.sum_sq(p, hf) == 20.0
    assert diag_numpy.scatter_summary(p, hf) == {"ll": -2.0, "ur": 3.0, "rmse": (20.0 / 3.0) ** 0.5, "sum_sq": 20.0, "n": 3}


# ---- the restatement against the reference's recorded outputs ---------------------------------------------------------------------------
def test_fixture_inputs_are_the_ones_recorded():
    import json

    meta = json.loads(str(FIX["meta_json"]))
    assert meta["input_checksums"] == input_checksums(FIELDS, DETECT)
    assert meta["restated_functions"] == [] and set(FIELD_SHAPES) < set(FIELDS)


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_restated_curves_and_scatter_numbers_equal_the_reference(name):
    c = FIELDS[name]
    n = c["hf"].size
    for key, side in (("lf", c["lf"]), ("upskill", c["upskill"])):
        assert same_bits(diag_numpy.sorted_abs_residual(side, c["hf"]), FIX[f"fields/{name}/cdf_{key}"])
        mine = diag_numpy.scatter_summary(side, c["hf"])
        ends, label = FIX[f"fields/{name}/scatter_{key}/ends"], str(FIX[f"fields/{name}/scatter_{key}/label"])
        assert np.array_equal([mine["ll"], mine["ur"]], ends, equal_nan=True)
        assert label == f"rmse: {round(mine['rmse'], 2)}"
    assert np.array_equal(FIX[f"fields/{name}/pcts"], np.linspace(0, 100, n))
    ranks = dg.cdf_ranks(n, 257)
    assert np.array_equal(dg.cdf_pcts(n, ranks), FIX[f"fields/{name}/pcts"][ranks])


@pytest.mark.parametrize("name", [n for n in sorted(DETECT) if n != "negative"])
def test_restated_detection_codes_equal_the_reference(name):
    c = DETECT[name]
    for cn in (0, 1):
        for k, thr in enumerate(DETECT_THRESHOLDS):
            assert np.array_equal(diag_numpy.detection_codes(c["y_true"], c["y_pred"], RANGES, thr, bool(cn)), FIX[f"detect/{name}/cn{cn}/thr{k}/codes"])


def test_negative_maximum_raises_like_the_reference():
    c = DETECT["negative"]
    assert str(FIX["detect/negative/raises"]) == "y_true and y_pred must be non-negative."
    with pytest.raises(ValueError, match="y_true and y_pred must be non-negative."):
        diag_numpy.detection_codes(c["y_true"], c["y_pred"], RANGES, 0.0, True)
