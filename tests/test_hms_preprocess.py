"""HmsPreProcessor (gpras/preprocess.py:1165-1320): CPU pins.  The numpy restatement (tests/hms_numpy.py) against the
reference's own outputs (tests/golden/hms_ref_golden.npz, make_golden_hms_ref.py) and against scikit-learn; the API
weights; the pickle format; the domain checks that run before any device work."""

import json
import os
import pickle
import sys

import numpy as np
import pytest

from gpras_amd.preprocess import HmsPreProcessor, PCAFit, api_weights, compute_norths_rule
from hms_numpy import api, assert_close, assert_fit_close, fit_reference, incremental_pca, transform_reference

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_hms_ref import api_case, hms_ref_cases  # noqa: E402

FIX = np.load(os.path.join(GOLDEN, "hms_ref_golden.npz"))
META = json.loads(str(FIX["meta_json"]))
CASES = hms_ref_cases()
ATTRS = ("input_mean", "eofs", "eigenvalues", "precip_spatial_mode_count", "n_samples_fit", "x_mean", "x_std")


def recorded(name):
    return {a: FIX[f"{name}/{a}"] for a in ATTRS}


def test_fixture_covers_the_issue_cases():
    shapes = {n: c["x"].shape[0] / int(np.sum(np.ones(c["x"].shape[1])[c["precip_mask"]])) for n, c in CASES.items()}
    assert any(r < 1 for r in shapes.values()) and any(1 < r <= 5 for r in shapes.values()) and any(r > 5 for r in shapes.values())
    assert any(c["k"] is None for c in CASES.values()) and any(c["k"] is not None for c in CASES.values())
    assert any(np.asarray(c["precip_mask"]).dtype != bool for c in CASES.values())
    assert np.isnan(FIX["zero_bc/x_std"]).sum() == 1
    a, k, window = api_case()
    assert window < len(a)
    assert META["cases"]["t_gt_5p"]["shape"][0] % (5 * META["cases"]["t_gt_5p"]["p"]) == 1  # a final batch of one row


@pytest.mark.parametrize("name", sorted(CASES))
def test_numpy_restatement_equals_reference(name):
    c = CASES[name]
    got = fit_reference(c["x"], c["bc_mask"], c["precip_mask"], c["k"])
    assert_fit_close(got, recorded(name), c["x"])
    state = dict(got, bc_mask=c["bc_mask"], precip_mask=c["precip_mask"])
    assert_close(transform_reference(state, c["x"]), FIX[f"{name}/transform"], 1e-10, "transform")


@pytest.mark.parametrize("name", sorted(CASES))
def test_numpy_restatement_equals_sklearn(name):
    sk = pytest.importorskip("sklearn.decomposition")
    c = CASES[name]
    x = c["x"]
    xp = (x - x.mean(axis=0))[:, np.arange(x.shape[1])[c["precip_mask"]]]
    pca = sk.IncrementalPCA().fit(xp.copy())
    comps, ev = incremental_pca(xp)
    assert pca.n_components_ == min(xp.shape) == len(ev)
    lam_max = ev[0]
    assert np.max(np.abs(ev - pca.explained_variance_)) <= 1e-12 * lam_max
    k = int(FIX[f"{name}/precip_spatial_mode_count"])
    for i in range(k):
        gap = min(abs(ev[i] - ev[j]) for j in (i - 1, i + 1) if 0 <= j < len(ev))
        assert np.max(np.abs(comps[i] - pca.components_[i])) <= 1e-12 * lam_max / gap
    assert compute_norths_rule(pca) == compute_norths_rule(PCAFit(ev, xp.shape[0]))


def test_api_restatement_equals_reference():
    a, k, window = api_case()
    assert np.array_equal(api(a, k, window), FIX["api/window"])
    assert np.array_equal(api(a), FIX["api/default"])


@pytest.mark.parametrize("k, window", [(0.85, 10000), (0.85, 3), (1, 500), (0.5, 2000), (-0.7, 3000), (0, 5), (1.01, 100)])
def test_api_weights_are_the_reference_expression_without_the_zero_tail(k, window):
    full = np.array([k**i for i in range(window)], dtype=np.float64)
    w = api_weights(k, window)
    assert np.array_equal(w, full[: w.size])
    assert not np.any(full[w.size :])
    if w.size < window:
        assert w[-1] != 0


def test_pickle_keys_equal_reference_and_hold_no_project_types(tmp_path):
    c, rec = CASES["interleaved"], recorded("interleaved")
    pre = HmsPreProcessor(precip_spatial_mode_count=int(rec["precip_spatial_mode_count"]), bc_mask=c["bc_mask"],
                          precip_mask=c["precip_mask"], eofs=rec["eofs"], eigenvalues=rec["eigenvalues"],
                          n_samples_fit=np.int64(rec["n_samples_fit"]), x_mean=rec["x_mean"], x_std=rec["x_std"],
                          input_mean=rec["input_mean"])
    assert sorted(pre.to_dict()) == META["to_dict_keys"]
    path = tmp_path / "hms.pkl"
    pre.to_file(path)
    blob = path.read_bytes()
    assert b"gpras_amd" not in blob  # the reference's from_file can load it: plain numpy objects only
    back = HmsPreProcessor.from_file(path)
    for key, v in pre.to_dict().items():
        assert np.array_equal(np.asarray(getattr(back, key)), np.asarray(v)), key


def test_reference_format_dict_loads(tmp_path):
    c, rec = CASES["t_mid"], recorded("t_mid")
    d = {"precip_spatial_mode_count": int(rec["precip_spatial_mode_count"]), "bc_mask": c["bc_mask"], "precip_mask": c["precip_mask"],
         "eofs": rec["eofs"], "eigenvalues": rec["eigenvalues"], "n_samples_fit": np.int64(rec["n_samples_fit"]), "x_mean": rec["x_mean"],
         "x_std": rec["x_std"], "input_mean": rec["input_mean"]}
    assert sorted(d) == META["to_dict_keys"]
    path = tmp_path / "ref.pkl"
    with open(path, "wb") as f:
        pickle.dump(d, f)
    back = HmsPreProcessor.from_file(path)
    for key, v in d.items():
        assert np.array_equal(np.asarray(getattr(back, key)), np.asarray(v)), key


def test_constructor_defaults_match_reference():
    pre = HmsPreProcessor()
    assert pre.precip_spatial_mode_count == 0 and pre.n_samples_fit == 0
    for key in ("bc_mask", "precip_mask", "eofs", "eigenvalues", "x_mean", "x_std", "input_mean"):
        assert np.asarray(getattr(pre, key)).shape == (0,), key


_M = np.array([True, False, False, True, True, False])


@pytest.mark.parametrize(
    "x, bc, pr, k",
    [
        (np.zeros(6), ~_M, _M, None),                           # not 2-D
        (np.zeros((5, 6)), ~_M[:5], _M, None),                  # bc mask of the wrong length
        (np.zeros((5, 6)), ~_M, np.append(_M, True), None),     # precip mask of the wrong length
        (np.zeros((5, 6)), ~_M, np.zeros(6, dtype=bool), None),  # no precip column
        (np.zeros((5, 6)), ~_M, np.array([], dtype=np.int64), None),
        (np.zeros((5, 6)), ~_M, np.array([1, 9]), None),        # index out of range
        (np.zeros((1, 6)), ~_M, _M, None),                      # one sample
        (np.zeros((5, 6)), ~_M, _M, -1),                        # negative mode count
        (np.zeros((5, 6)), ~_M, _M, 1.5),
    ],
)
def test_domain_checks_raise_before_device_work(x, bc, pr, k):
    with pytest.raises(ValueError):
        HmsPreProcessor.check_fit_args(x, bc, pr, k)
    with pytest.raises(ValueError):
        HmsPreProcessor().fit(x, bc, pr, k)  # no library call happens: this passes without a device


@pytest.mark.parametrize("a, window", [(np.zeros(5), 0), (np.zeros(5), -2), (np.zeros(0), None), (np.zeros((3, 2)), None)])
def test_api_domain_raises_before_device_work(a, window):
    with pytest.raises(ValueError):
        HmsPreProcessor().calc_antecedent_precipitation_index(a, window=window)
    if np.ndim(a) == 1 and (window == 0 or len(a) == 0):
        with pytest.raises(ValueError):
            api(a, window=window)  # np.convolve raises on an empty operand, as the reference does


def test_domain_keeps_the_memory_order_and_casts():
    x = np.asfortranarray(np.zeros((4, 6)))
    xx, ld, fortran = HmsPreProcessor.check_fit_args(x, ~_M, _M)[:3]
    assert xx is x and fortran == 1 and ld == 4
    xx, ld, fortran = HmsPreProcessor.check_fit_args(np.zeros((4, 6), dtype=np.float32), ~_M, _M)[:3]
    assert xx.dtype == np.float64 and fortran == 0 and ld == 6
    bc, pc = HmsPreProcessor.check_fit_args(np.zeros((4, 6)), np.array([5, 0]), _M)[3:]
    assert bc.tolist() == [5, 0] and pc.tolist() == [0, 3, 4]
