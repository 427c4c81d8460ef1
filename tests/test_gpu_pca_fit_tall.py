"""The covariance route of PreProcessor.fit on the MI355X (``sample_route = "auto"``, gprx_pcafit_create_auto / _cov / _components_cov;
csrc/pca_fit_tall.h): parity with the reference's own fit on more samples than wet cells (tests/golden/pca_fit_tall_ref_golden.npz) and
with the numpy restatement (tests/pca_fit_tall_numpy.py) under the bounds of DESIGN.md section 3.12b; ``input_mean`` against live
numpy across the 8192-row piece; the row-split kernels against the one-thread-per-cell kernels bit for bit; determinism; the Gram
route through "auto"; the device eigensolver; the pickle round trip; the wrong-route calls of the C ABI."""

import ctypes as C
import os
import sys

import numpy as np
import pytest

from gpras_amd import _lib
from gpras_amd._lib import ptr
from gpras_amd.preprocess import PreProcessor
from pca_fit_tall_numpy import assert_tall_fit_close, fit_reference_tall

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_pca_fit_ref import THRESHOLD, pca_fit_ref_cases  # noqa: E402
from make_golden_pca_fit_tall_ref import pca_fit_tall_ref_cases  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(GOLDEN, "pca_fit_tall_ref_golden.npz"))
CASES = pca_fit_tall_ref_cases()
ATTRS = ("wetness_classes", "input_mean", "weights", "eofs", "eigenvalues", "spatial_mode_count", "n_samples_fit", "x_mean", "x_std")
GPRX_ESTATE = 5


def auto_fit(x, elev, w, k, mode, eigensolver="host"):
    pre = PreProcessor(wet_threshold=THRESHOLD, hydraulic_parameter=mode)
    pre.sample_route = "auto"
    pre.eigensolver = eigensolver
    pre.fit(x, elev, w, k)
    return pre


def case_fit(c, **kw):
    return auto_fit(c["x"], c["elevations"], c["weights"], c["k"], c["mode"], **kw)


def attrs_of(pre, x=None):
    got = {a: getattr(pre, a) for a in ATTRS}
    if x is not None and pre.spatial_mode_count:
        got["transform"] = pre.transform(x)
    return got


def assert_same_bits(a, b):
    for key in ATTRS:
        assert np.array_equal(np.asarray(getattr(a, key)), np.asarray(getattr(b, key))), key


def random_case(n_s, cells, mode, weighted, seed):
    """Low-rank signal plus noise, a tenth of the cells always dry (wse / depth), from two cells on."""
    rng = np.random.default_rng(seed)
    r = min(4, cells)
    scales = 3.0 * 0.6 ** np.arange(r)
    elev = 9.5 + 1.5 * rng.random(cells)
    if cells > 8:
        elev[rng.random(cells) < 0.1] += 50.0
    x = 11.0 + 0.5 * (rng.standard_normal((n_s, r)) * scales) @ rng.standard_normal((r, cells)) + 0.01 * rng.standard_normal((n_s, cells))
    w = 0.5 + rng.random(cells) if weighted else None
    return x, elev, w


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_equals_reference(name):
    c = CASES[name]
    pre = case_fit(c)
    assert pre.last_route == "covariance" and "covariance" in pre.last_timings_ms
    want = {a: FIX[f"{name}/{a}"] for a in ATTRS}
    if f"{name}/transform" in FIX.files:
        want["transform"] = FIX[f"{name}/transform"]
    fig = {}
    try:
        assert_tall_fit_close(attrs_of(pre, c["x"]), want, report=fig)
    finally:
        print(name, fig)
    assert np.array_equal(pre.dry_indices, FIX[f"{name}/wetness_classes"] == "AD")
    assert pre.pca_.components_.shape == (pre.spatial_mode_count, c["n_wet"]) and pre.pca_.n_samples_seen_ == c["x"].shape[0]


SHAPES = [(129, 40, "wse", True), (1031, 97, "depth", False), (300, 5, "velocity", True), (700, 257, "wse", False), (8193, 17, "depth", True),
          (16385, 24, "wse", False), (20001, 300, "velocity", False)]


@pytest.mark.parametrize("n_s, cells, mode, weighted", SHAPES)
def test_shapes_equal_restatement(n_s, cells, mode, weighted):
    x, elev, w = random_case(n_s, cells, mode, weighted, seed=n_s + cells)
    k = 3
    want = fit_reference_tall(x, elev, w, k, mode, THRESHOLD)
    pre = auto_fit(x, elev, w, k, mode)
    assert pre.last_route == "covariance"
    fig = {}
    try:
        assert_tall_fit_close(attrs_of(pre, x), want, report=fig)
    finally:
        print((n_s, cells), fig)


@pytest.mark.parametrize("n_s, cells", [(8192, 20), (8193, 17), (16385, 24), (24577, 9)])
def test_input_mean_equals_live_numpy_across_the_piece_boundary(n_s, cells):
    x, _, _ = random_case(n_s, cells, "velocity", False, seed=n_s)
    pre = auto_fit(x, None, None, 2, "velocity")
    assert pre.last_route == "covariance"
    assert np.array_equal(pre.input_mean, np.asfortranarray(x).mean(axis=0))


@pytest.mark.parametrize("n_s, cells, mode, weighted", [(8193, 17, "depth", True), (1031, 97, "wse", False), (60, 57, "wse", True)])
def test_rowsplit_kernels_equal_the_cell_kernels_bit_for_bit(n_s, cells, mode, weighted):
    # (60, 57): n_samples <= n_cells with fewer wet cells than samples, the shape where "auto" has tried the Gram route first
    x, elev, w = random_case(n_s, cells, mode, weighted, seed=7 * n_s + cells)
    if cells == 57:
        elev[40:] += 50.0
    lib = _lib.load()
    fits = {}
    try:
        for v in (0, 1):
            _lib.check(lib.gprx_set_tuning(b"pcafit_rowsplit", v))
            fits[v] = auto_fit(x, elev, w, None, mode)
    finally:
        _lib.check(lib.gprx_set_tuning(b"pcafit_rowsplit", 1))
    assert fits[0].last_route == fits[1].last_route == "covariance"
    assert_same_bits(fits[0], fits[1])


def test_two_fits_identical_bits():
    c = CASES["depth_w_north_manybatch"]
    assert_same_bits(case_fit(c), case_fit(c))


def test_auto_takes_the_gram_route_with_the_default_bits():
    c = pca_fit_ref_cases()["depth_w_north"]
    default = PreProcessor(wet_threshold=THRESHOLD, hydraulic_parameter=c["mode"])
    default.fit(c["x"], c["elevations"], c["weights"], c["k"])
    auto = case_fit(c)
    assert default.last_route == auto.last_route == "gram" and "covariance" not in auto.last_timings_ms
    assert_same_bits(default, auto)


def test_default_route_still_refuses_tall_input():
    c = CASES["velocity_u_north_plus1"]
    with pytest.raises(ValueError):
        PreProcessor(wet_threshold=THRESHOLD, hydraulic_parameter=c["mode"]).fit(c["x"], c["elevations"], c["weights"], c["k"])


def test_device_eigensolver_on_the_covariance_route():
    name = "wse_w_north_onebatch"
    c = CASES[name]
    pre = case_fit(c, eigensolver="device")
    assert pre.last_route == "covariance" and pre.last_eig_sweeps >= 1 and "eigensolver" in pre.last_timings_ms
    want = {a: FIX[f"{name}/{a}"] for a in ATTRS}
    want["transform"] = FIX[f"{name}/transform"]
    assert_tall_fit_close(attrs_of(pre, c["x"]), want)


def test_more_modes_than_wet_cells_is_a_value_error():
    x, elev, w = random_case(50, 12, "wse", False, seed=3)
    elev[:] = 9.0
    elev[9:] += 50.0  # 9 wet cells: k = 10 passes the check before the device (k <= n_cells) and fails once n_wet is known
    assert auto_fit(x, elev, None, 8, "wse").eofs.shape == (8, 9)
    with pytest.raises(ValueError):
        auto_fit(x, elev, None, 10, "wse")


def test_pickle_of_a_tall_fit_reloads_and_projects_identically(tmp_path):
    c = CASES["wse_u_k_manybatch"]
    pre = case_fit(c)
    path = tmp_path / "pre.pkl"
    pre.to_file(path)
    back = PreProcessor.from_file(path)
    assert sorted(back.to_dict()) == sorted(pre.to_dict())
    z, z2 = pre.transform(c["x"]), back.transform(c["x"])
    assert np.array_equal(z, z2)
    f1, v1 = pre.reverse_transform(z, np.abs(z) * 0.1)
    f2, v2 = back.reverse_transform(z, np.abs(z) * 0.1)
    assert np.array_equal(f1, f2) and np.array_equal(v1, v2)


def test_wrong_route_calls_return_estate():
    lib = _lib.load()
    tall, short = CASES["velocity_w_k_plus1"], pca_fit_ref_cases()["velocity_u_k"]
    for c, route_name, wrong in ((tall, "covariance", ("gprx_pcafit_gram", "gprx_pcafit_components")),
                                 (short, "Gram", ("gprx_pcafit_cov", "gprx_pcafit_components_cov"))):
        x = np.ascontiguousarray(c["x"])
        n_s, cells = x.shape
        w = None if c["weights"] is None else ptr(c["weights"])
        h, route = C.c_void_p(), C.c_int(-1)
        _lib.check(lib.gprx_pcafit_create_auto(0, ptr(x), n_s, cells, None, w, 2, THRESHOLD, C.byref(route), C.byref(h)))
        try:
            assert _lib.PCAFIT_ROUTES[route.value] == route_name.lower()
            codes, mean, g, n_wet = np.empty(cells, dtype=np.uint8), np.empty(cells), np.empty((max(n_s, cells),) * 2), C.c_int64()
            assert getattr(lib, wrong[0])(h, ptr(codes), ptr(mean), ptr(g), C.byref(n_wet)) == GPRX_ESTATE
            assert route_name in lib.gprx_pcafit_last_error(h).decode()
            u, lam, eofs, z = np.zeros((max(n_s, cells), 1)), np.ones(1), np.empty((1, cells)), np.empty((n_s, 1))
            if wrong[1] == "gprx_pcafit_components":
                rc = lib.gprx_pcafit_components(h, 1, ptr(u), ptr(lam), ptr(eofs), ptr(z))
            else:
                rc = lib.gprx_pcafit_components_cov(h, 1, ptr(u), ptr(eofs), ptr(z))
            assert rc == GPRX_ESTATE and route_name in lib.gprx_pcafit_last_error(h).decode()
        finally:
            lib.gprx_pcafit_destroy(h)
