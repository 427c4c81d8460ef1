"""The pseudo-surface low-fidelity model (gpras/preprocess.py:454-697): CPU pins.  The numpy restatement (tests/pseudo_numpy.py)
against the reference's own outputs (tests/golden/pseudo_ref_golden.npz, make_golden_pseudo_ref.py); the host side of
``RatingCurve`` and ``PseudoSurface`` (filter, sort, errors, storage, the argument checks that run before any device work)."""

import json
import os
import sys

import numpy as np
import pytest

import pseudo_numpy
from gpras_amd.pseudo_surface import PseudoSurface, RatingCurve, check_spline, spline_arrays

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_pseudo_ref import N_CELLS, N_CENTERLINE, input_checksums, pseudo_ref_cases  # noqa: E402

FIX = np.load(os.path.join(GOLDEN, "pseudo_ref_golden.npz"))
META = json.loads(str(FIX["meta_json"]))
CASES = pseudo_ref_cases()
QUERIES = ("below", "inside", "above", "column", "knots")


def queries(name):
    return dict(CASES["curves"][name]["queries"], knots=FIX[f"curve/{name}/knots"])


def test_fixture_covers_the_issue_cases():
    for name in ("us", "ds"):
        c = CASES["curves"][name]
        kept = FIX[f"curve/{name}/q"]
        assert np.sum(~np.isfinite(c["q"])) >= 2 and np.sum(c["q"] <= 0) >= 2 and np.sum(c["q"] >= 10e10) >= 1 and np.sum((c["q"] > 0) & (c["q"] <= 10)) >= 1
        q = queries(name)
        assert q["below"].max() < kept[0] and q["above"].min() > kept[-1] and kept[0] < q["inside"].min() and q["inside"].max() < kept[-1]
        assert q["column"].shape == (57, 1) and FIX[f"curve/{name}/predict/column"].shape == (57, 1)
    assert META["few_points_raises"] == "ValueError"
    cs = META["cases"]
    assert cs["odd"]["kept"] % 2 == 1 and cs["even"]["kept"] % 2 == 0 and cs["odd"]["kept"] < cs["odd"]["rows"]
    assert cs["nan_column"]["nan_columns"] == 1 and N_CENTERLINE % 32 != 0 and N_CELLS % 2 == 1
    for name, c in CASES["fits"].items():
        keep = (c["us_q"] > 0) | (c["ds_q"] > 0)
        assert np.any(keep & (c["us_wse"] == c["ds_wse"])), name  # a flat row among the kept ones
    assert min(cs["surface_a"]["wins"]) > 0 and cs["surface_a"]["nan"] == 2
    assert META["eps_spline"] == float(FIX["eps_spline"])


def test_generator_inputs_regenerate():
    assert input_checksums(CASES) == META["input_checksums"]
    again = pseudo_ref_cases()
    assert np.array_equal(again["fits"]["even"]["wse"], CASES["fits"]["even"]["wse"])


@pytest.mark.parametrize("name", ["us", "ds"])
def test_spline_restatement_equals_the_reference_within_eps(name):
    knots, coef = FIX[f"curve/{name}/knots"], FIX[f"curve/{name}/coefficients"]
    worst = 0.0
    for qn, qv in queries(name).items():
        want = FIX[f"curve/{name}/predict/{qn}"]
        got = pseudo_numpy.spline_eval(knots, coef, qv)
        assert got.shape == want.shape
        worst = max(worst, float(np.max(np.abs(got - want) / np.abs(want))))
    assert worst <= float(FIX["eps_spline"])


def test_spline_restatement_against_scipy_and_nan():
    from scipy.interpolate import BSpline

    knots, coef = FIX["curve/us/knots"], FIX["curve/us/coefficients"]
    x = np.linspace(knots[0] * 0.5, knots[-1] * 1.5, 501)
    want = BSpline(knots, coef, 3, extrapolate=True)(x)
    np.testing.assert_allclose(pseudo_numpy.spline_eval(knots, coef, x), want, rtol=1e-11)
    assert np.isnan(pseudo_numpy.spline_eval(knots, coef, np.array([np.nan, 100.0]))).tolist() == [True, False]


@pytest.mark.parametrize("name", ["odd", "even", "nan_column", "ties"])
def test_median_restatement_equals_the_reference_bit_for_bit(name):
    c = CASES["fits"][name]
    got = pseudo_numpy.fit_centerline(c["us_wse"], c["ds_wse"], c["us_q"], c["ds_q"], c["wse"])
    want = FIX[f"fit/{name}/cl_interpolater"]
    assert np.array_equal(got.view(np.int64)[~np.isnan(want)], want.view(np.int64)[~np.isnan(want)])
    assert np.array_equal(np.isnan(got), np.isnan(want))


def test_the_flat_row_does_not_move_the_median():
    c = CASES["fits"]["odd"]
    keep = (c["us_q"] > 0) | (c["ds_q"] > 0)
    flat = np.flatnonzero(keep & (c["us_wse"] == c["ds_wse"]))[0]
    with np.errstate(divide="ignore"):
        ratio = (c["us_wse"][flat] - c["wse"][flat]) / (c["us_wse"][flat] - c["ds_wse"][flat])
    assert np.all(np.isinf(ratio))
    assert np.all(np.isfinite(FIX["fit/odd/cl_interpolater"]))


@pytest.mark.parametrize("name", ["a", "b"])
def test_surface_restatement_equals_the_reference_bit_for_bit(name):
    c = CASES["surfaces"][name]
    w = FIX[f"fit/{c['fit']}/cl_interpolater"]
    us, ds = FIX[f"surface/{name}/us_wse"], FIX[f"surface/{name}/ds_wse"]
    cl = pseudo_numpy.interpolate_centerline(us, ds, w)
    assert np.array_equal(cl, FIX[f"surface/{name}/centerline"])
    assert np.array_equal(cl[:, c["idx"]], FIX[f"surface/{name}/gathered"])
    assert np.array_equal(pseudo_numpy.surface(us, ds, w, c["idx"], c["elev"], c["fluvial"]), FIX[f"surface/{name}/lf_plan_data"], equal_nan=True)


# ---- the host side of the classes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["us", "ds"])
def test_rating_curve_filters_sorts_and_fits_as_the_reference(name):
    c = CASES["curves"][name]
    rc = RatingCurve(c["q"], c["wse"])
    assert np.array_equal(rc.q, FIX[f"curve/{name}/q"]) and np.array_equal(rc.wse, FIX[f"curve/{name}/wse"])
    assert np.all(np.diff(rc.q) >= 0) and rc.q.min() > 10 and np.all(np.isfinite(rc.wse))
    assert rc.n_knots == 7 and rc.knots.shape == (15,) and rc.coefficients.shape == (11,)
    # the same scipy routine on the same data: the same knots and coefficients
    assert np.array_equal(rc.knots, FIX[f"curve/{name}/knots"])
    np.testing.assert_allclose(rc.coefficients, FIX[f"curve/{name}/coefficients"], rtol=1e-12)
    t, coef = spline_arrays(rc.spline)
    assert np.array_equal(t, rc.knots) and np.array_equal(coef, rc.coefficients)


def test_rating_curve_options_and_errors():
    c = CASES["curves"]["us"]
    keep_all = RatingCurve(c["q"], c["wse"], drop_nonpos=False, qmin=None, qmax=None)
    assert keep_all.q.min() <= 0 and keep_all.q.max() > 10e10 and np.all(np.isfinite(keep_all.q))
    few = CASES["curves"]["few"]
    with pytest.raises(ValueError, match="Not enough points"):
        RatingCurve(few["q"], few["wse"])
    assert len(RatingCurve(few["q"], few["wse"], n_knots=3).knots) == 11
    with pytest.raises(ValueError):
        RatingCurve(c["q"], c["wse"], n_knots=65)
    with pytest.raises(ValueError):
        check_spline(np.arange(15.0), np.zeros(12))
    with pytest.raises(ValueError):
        check_spline(np.r_[np.zeros(4), 3.0, 2.0, np.full(4, 5.0)], np.zeros(6))
    rc = RatingCurve.from_arrays(FIX["curve/us/knots"], FIX["curve/us/coefficients"])
    assert rc.n_knots == 7 and rc.q is None
    with pytest.raises(ValueError):
        rc.fit_stats


def _estimator(**kw):
    c = CASES["surfaces"]["a"]
    curves = [RatingCurve.from_arrays(FIX[f"curve/{n}/knots"], FIX[f"curve/{n}/coefficients"]) for n in ("us", "ds")]
    return PseudoSurface(c["elev"], c["idx"], curves[0], curves[1], FIX["fit/odd/cl_interpolater"], **kw)


def test_pseudo_surface_argument_checks_run_before_any_device_work():
    c = CASES["surfaces"]["a"]
    w = FIX["fit/odd/cl_interpolater"]
    for bad in (c["idx"].astype(float), c["idx"][:-1], np.where(np.arange(N_CELLS) == 4, N_CENTERLINE, c["idx"]), np.where(np.arange(N_CELLS) == 4, -1, c["idx"])):
        with pytest.raises(ValueError):
            PseudoSurface(c["elev"], bad, None, None, w)
    with pytest.raises(ValueError):
        PseudoSurface(c["elev"], c["idx"], RatingCurve.from_arrays(FIX["curve/us/knots"], FIX["curve/us/coefficients"]), None, w)
    ps = _estimator()
    assert ps.n_cells == N_CELLS and ps.n_centerline == N_CENTERLINE and ps.cell_interpolater.dtype == np.int32
    with pytest.raises(ValueError):
        ps.fit_centerline(np.ones(5), np.ones(5), np.ones(5), np.ones(5), np.ones((5, N_CENTERLINE + 1)))
    with pytest.raises(ValueError):
        ps.fit_centerline(np.ones(4), np.ones(5), np.ones(5), np.ones(5), np.ones((5, N_CENTERLINE)))
    with pytest.raises(ValueError, match="positive"):
        ps.fit_centerline(np.ones(5), np.ones(5), np.zeros(5), -np.ones(5), np.ones((5, N_CENTERLINE)))
    with pytest.raises(ValueError):
        ps.interpolate_surface(np.ones((3, N_CENTERLINE - 1)))
    unfitted = PseudoSurface(c["elev"], c["idx"], None, None)
    assert unfitted.n_centerline == int(c["idx"].max()) + 1
    with pytest.raises(ValueError, match="not fitted"):
        unfitted.interpolate_centerline(np.ones(3), np.ones(3))
    with pytest.raises(ValueError, match="not fitted"):
        unfitted.lf_plan_data(np.ones(3), np.ones(3))


def test_to_dict_round_trip_and_npz_file(tmp_path):
    ps = _estimator()
    d = ps.to_dict()
    assert all(isinstance(v, np.ndarray) for v in d.values())
    path = tmp_path / "pseudo.npz"
    ps.to_file(path)
    back = PseudoSurface.from_file(path)
    with np.load(path, allow_pickle=False) as z:  # plain arrays only
        assert set(z.files) == set(d) | {"format"}
    for key, v in d.items():
        assert np.array_equal(np.asarray(back.to_dict()[key]), v), key
    assert back.us_rating_curve.n_knots == 7 and back.cell_interpolater.dtype == np.int32
    bare = PseudoSurface.from_dict(PseudoSurface(d["cell_elevations"], d["cell_interpolater"], None, None, n_centerline=N_CENTERLINE).to_dict())
    other = tmp_path / "other.npz"
    np.savez(other, x=np.zeros(3))
    with pytest.raises(ValueError, match="not a pseudo-surface file"):
        PseudoSurface.from_file(other)
    assert bare.cl_interpolater is None and bare.us_rating_curve is None and bare.n_centerline == N_CENTERLINE
