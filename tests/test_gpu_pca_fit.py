"""Fitting the EOF preprocessor on the MI355X (gprx_pcafit_*): parity with the reference's own fit (tests/golden/
pca_fit_ref_golden.npz) and with the numpy restatement (tests/pca_fit_numpy.py) under the bounds of DESIGN.md section 3.12;
determinism; the pickle round trip of a device fit."""

import os
import sys

import numpy as np
import pytest

from gpras_amd.preprocess import PreProcessor
from pca_fit_numpy import assert_fit_close, fit_reference

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_pca_fit_ref import THRESHOLD, pca_fit_ref_cases  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(GOLDEN, "pca_fit_ref_golden.npz"))
CASES = pca_fit_ref_cases()
ATTRS = ("wetness_classes", "input_mean", "weights", "eofs", "eigenvalues", "spatial_mode_count", "n_samples_fit", "x_mean", "x_std")


def device_fit(c, k=None):
    pre = PreProcessor(wet_threshold=THRESHOLD, hydraulic_parameter=c["mode"])
    pre.fit(c["x"], c["elevations"], c["weights"], c["k"] if k is None else k)
    return pre


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_equals_reference(name):
    c = CASES[name]
    pre = device_fit(c)
    got = {a: getattr(pre, a) for a in ATTRS}
    assert_fit_close(got, {a: FIX[f"{name}/{a}"] for a in ATTRS})
    assert np.array_equal(pre.dry_indices, FIX[f"{name}/wetness_classes"] == "AD")
    z = pre.transform(c["x"])
    want = FIX[f"{name}/transform"]
    assert z.shape == want.shape
    if z.shape[1]:
        assert np.max(np.abs(z - want)) <= 1e-9
        assert np.max(np.abs(z.mean(axis=0))) <= 1e-9
        assert np.allclose(z.std(axis=0), 1.0, rtol=0, atol=1e-9)


def test_zero_modes_like_reference():
    c = CASES["wse_u_zero"]
    pre = device_fit(c)
    assert pre.spatial_mode_count == 0
    assert pre.eofs.shape == (0, FIX["wse_u_zero/input_mean"].size)
    assert pre.x_mean.shape == (0,) and pre.x_std.shape == (0,)
    assert pre.transform(c["x"]).shape == (c["x"].shape[0], 0)


@pytest.mark.parametrize(
    "n_s, cells, mode, weighted, seed",
    [(16, 1000, "wse", True, 1), (64, 4099, "depth", False, 2), (65, 20000, "velocity", True, 3), (128, 12345, "wse", False, 4),
     (200, 100000, "depth", True, 5)],
)
def test_random_shapes_equal_restatement(n_s, cells, mode, weighted, seed):
    rng = np.random.default_rng(seed)
    r = 6
    scales = 3.0 * 0.6 ** np.arange(r)
    elev = 10.0 + 2.0 * rng.random(cells)
    elev[rng.random(cells) < 0.1] += 50.0
    x = 11.0 + 0.5 * (rng.standard_normal((n_s, r)) * scales) @ rng.standard_normal((r, cells)) + 0.01 * rng.standard_normal((n_s, cells))
    w = 0.5 + rng.random(cells) if weighted else None
    k = 5
    want = fit_reference(x, elev, w, k, mode, THRESHOLD)
    pre = PreProcessor(wet_threshold=THRESHOLD, hydraulic_parameter=mode)
    pre.fit(x, elev, w, k)
    assert_fit_close({a: getattr(pre, a) for a in ATTRS}, want)


def test_two_fits_identical_bits():
    c = CASES["depth_w_north"]
    a, b = device_fit(c), device_fit(c)
    for key in ATTRS:
        assert np.array_equal(np.asarray(getattr(a, key)), np.asarray(getattr(b, key))), key


def test_pickle_of_device_fit_reloads_and_projects_identically(tmp_path):
    c = CASES["wse_w_north"]
    pre = device_fit(c)
    path = tmp_path / "pre.pkl"
    pre.to_file(path)
    back = PreProcessor.from_file(path)
    z, z2 = pre.transform(c["x"]), back.transform(c["x"])
    assert np.array_equal(z, z2)
    f1, v1 = pre.reverse_transform(z, np.abs(z) * 0.1)
    f2, v2 = back.reverse_transform(z, np.abs(z) * 0.1)
    assert np.array_equal(f1, f2) and np.array_equal(v1, v2)
    d = back.wse_2_depth(c["x"])
    assert np.array_equal(d, np.maximum(c["x"] - c["elevations"], 0.0))


def test_unweighted_fit_keeps_empty_weights_and_projects_unweighted():
    c = CASES["velocity_u_k"]
    pre = device_fit(c)
    assert pre.weights.shape == (0,)
    assert np.max(np.abs(pre.transform(c["x"]) - FIX["velocity_u_k/transform"])) <= 1e-9


def test_fewer_wet_cells_than_samples_is_a_value_error():
    rng = np.random.default_rng(0)
    elev = np.full(40, 10.0)
    elev[5:] += 100.0  # 5 wet cells, 8 samples
    x = 11.0 + rng.random((8, 40))
    with pytest.raises(ValueError):
        PreProcessor(hydraulic_parameter="wse").fit(x, elev)
