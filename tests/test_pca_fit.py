"""Fitting the EOF preprocessor (PreProcessor.fit, gpras/preprocess.py:947-1007): CPU pins.  The numpy restatement of the
single-batch IncrementalPCA fit (tests/pca_fit_numpy.py) against the reference's own outputs (tests/golden/
pca_fit_ref_golden.npz, make_golden_pca_fit_ref.py) and against scikit-learn; North's rule; the pickle format; the domain
checks that run before any device work."""

import json
import os
import pickle
import sys

import numpy as np
import pytest

from gpras_amd.preprocess import PCAFit, PreProcessor, check_fit_args, compute_norths_rule
from pca_fit_numpy import assert_fit_close, fit_reference, single_batch_pca

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_pca_fit_ref import THRESHOLD, norths_rule_cases, pca_fit_ref_cases  # noqa: E402

FIX = np.load(os.path.join(GOLDEN, "pca_fit_ref_golden.npz"))
META = json.loads(str(FIX["meta_json"]))
CASES = pca_fit_ref_cases()
ATTRS = ("wetness_classes", "input_mean", "weights", "eofs", "eigenvalues", "spatial_mode_count", "n_samples_fit", "x_mean", "x_std")


def recorded(name):
    return {a: FIX[f"{name}/{a}"] for a in ATTRS}


def test_fixture_covers_the_issue_cases():
    modes = {(c["mode"], c["weighted"], c["k"] is None) for c in CASES.values()}
    assert len(modes) == 12
    assert any(FIX[f"{n}/wetness_classes"].tolist().count("") for n in CASES), "no cell sits exactly at the threshold"
    assert any((FIX[f"{n}/wetness_classes"] == "AD").any() for n in CASES)
    assert int(FIX["wse_u_zero/spatial_mode_count"]) == 0
    assert all(FIX[f"{n}/input_mean"].size % 16 for n in CASES if n != "wse_w_k")
    assert {c["x"].shape[0] for c in CASES.values()} >= {7, 60}


@pytest.mark.parametrize("name", sorted(CASES))
def test_numpy_restatement_equals_reference(name):
    c = CASES[name]
    got = fit_reference(c["x"], c["elevations"], c["weights"], c["k"], c["mode"], THRESHOLD)
    assert_fit_close(got, recorded(name))


@pytest.mark.parametrize("name", sorted(CASES))
def test_numpy_restatement_equals_sklearn(name):
    sk = pytest.importorskip("sklearn.decomposition")
    c = CASES[name]
    rec = recorded(name)
    dry = rec["wetness_classes"] == "AD"
    x = np.maximum(c["x"] - c["elevations"], 0.0) if c["mode"] == "depth" else c["x"]
    xw = x[:, ~dry] - rec["input_mean"]
    if c["weights"] is not None:
        xw = xw * c["weights"][~dry]
    pca = sk.IncrementalPCA().fit(xw.copy())
    comps, ev = single_batch_pca(xw)
    lam_max = ev[0]
    assert np.max(np.abs(ev - pca.explained_variance_)) <= 1e-12 * lam_max
    for i in range(int(rec["spatial_mode_count"])):
        assert np.max(np.abs(comps[i] - pca.components_[i])) <= 1e-13 * lam_max / ev[i]
    assert compute_norths_rule(pca) == compute_norths_rule(PCAFit(ev, x.shape[0]))


@pytest.mark.parametrize("name", sorted(norths_rule_cases()))
def test_norths_rule_equals_reference(name):
    ev, n = norths_rule_cases()[name]
    want = int(FIX[f"norths/{name}"])
    if want == -1:  # the reference's np.argmax of an empty comparison
        with pytest.raises(ValueError):
            compute_norths_rule(PCAFit(ev, n))
        return
    assert compute_norths_rule(PCAFit(ev, n)) == want

    class LikePCA:  # sklearn.decomposition.PCA spells the sample count n_samples_
        explained_variance_ = ev
        n_samples_ = n

    assert compute_norths_rule(LikePCA()) == want


def test_norths_rule_of_anything_else_is_zero():
    assert compute_norths_rule(object()) == int(FIX["norths/not_a_pca"]) == 0


def test_pickle_round_trip_keys_equal_reference(tmp_path):
    rec = recorded("depth_w_north")
    pre = PreProcessor(spatial_mode_count=int(rec["spatial_mode_count"]), input_mean=rec["input_mean"], wet_threshold=THRESHOLD,
                       elevations=CASES["depth_w_north"]["elevations"], hydraulic_parameter="depth", wetness_classes=rec["wetness_classes"],
                       weights=rec["weights"], eofs=rec["eofs"], eigenvalues=rec["eigenvalues"], n_samples_fit=int(rec["n_samples_fit"]),
                       x_mean=rec["x_mean"], x_std=rec["x_std"])
    assert sorted(pre.to_dict()) == META["to_dict_keys"]
    path = tmp_path / "pre.pkl"
    pre.to_file(path)
    with open(path, "rb") as f:
        d = pickle.load(f)
    assert sorted(d) == META["to_dict_keys"]
    back = PreProcessor.from_file(path)
    for key, v in pre.to_dict().items():
        assert np.array_equal(np.asarray(getattr(back, key)), np.asarray(v)), key
    assert np.array_equal(back.dry_indices, rec["wetness_classes"] == "AD")
    assert back.eof is back.eofs


def test_constructor_defaults_match_reference():
    pre = PreProcessor()
    assert pre.spatial_mode_count == 0 and pre.wet_threshold == 0.03 and pre.hydraulic_parameter == "wse"
    for key in ("input_mean", "elevations", "wetness_classes", "weights", "eofs", "eigenvalues", "x_mean", "x_std"):
        assert np.asarray(getattr(pre, key)).shape == (0,), key
    assert pre.n_samples_fit == 0


@pytest.mark.parametrize(
    "x, elev, w, k, mode",
    [
        (np.zeros((1, 10)), np.zeros(10), None, None, "wse"),        # one sample
        (np.zeros((11, 10)), np.zeros(10), None, None, "wse"),       # more samples than cells
        (np.zeros((3, 10)), None, None, None, "depth"),              # no elevations
        (np.zeros((3, 10)), np.zeros(9), None, None, "wse"),         # elevations of the wrong length
        (np.zeros((3, 10)), np.zeros(10), np.ones(9), None, "wse"),  # weights of the wrong length
        (np.zeros((3, 10)), np.zeros(10), None, 3, "wse"),           # k beyond the rank left after centring
        (np.zeros((3, 10)), np.zeros(10), None, -1, "wse"),
        (np.zeros((3, 10)), np.zeros(10), None, None, "stage"),      # unknown parameter
        (np.zeros(10), np.zeros(10), None, None, "wse"),             # not 2-D
    ],
)
def test_domain_checks_raise_before_device_work(x, elev, w, k, mode):
    with pytest.raises(ValueError):
        check_fit_args(x, elev, w, k, mode)
    pre = PreProcessor(hydraulic_parameter=mode)
    with pytest.raises(ValueError):
        pre.fit(x, elev, w, k)  # no library call happens: this passes without a device


def test_domain_accepts_the_production_shape():
    x, elev, w = check_fit_args(np.zeros((4, 10), dtype=np.float32), np.zeros(10), np.ones(10), 3, "wse")
    assert x.dtype == np.float64 and x.flags.c_contiguous
    x, elev, w = check_fit_args(np.zeros((4, 10)), None, None, None, "velocity")
    assert elev is None and w is None
