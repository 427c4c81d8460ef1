"""HmsPreProcessor on the MI355X (gprx_hms_*, gprx_api): parity with the reference's own fit (tests/golden/hms_ref_golden.npz)
and with the numpy restatement (tests/hms_numpy.py) under the bounds of DESIGN.md section 3.13; the API against np.convolve;
determinism; causality of transform; pickle round trips."""

import os
import pickle
import sys

import numpy as np
import pytest

from gpras_amd.preprocess import HmsPreProcessor
from hms_numpy import api, api_fast, assert_close, assert_fit_close, fit_reference, transform_reference

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_hms_ref import api_case, hms_ref_cases  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(GOLDEN, "hms_ref_golden.npz"))
CASES = hms_ref_cases()
ATTRS = ("input_mean", "eofs", "eigenvalues", "precip_spatial_mode_count", "n_samples_fit", "x_mean", "x_std")


def device_fit(c, x=None):
    pre = HmsPreProcessor()
    pre.fit(c["x"] if x is None else x, c["bc_mask"], c["precip_mask"], c["k"])
    return pre


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("order", ["C", "F"])
def test_fit_and_transform_equal_reference(name, order):
    c = CASES[name]
    x = np.asarray(c["x"], order=order)
    pre = device_fit(c, x)
    assert_fit_close({a: getattr(pre, a) for a in ATTRS}, {a: FIX[f"{name}/{a}"] for a in ATTRS}, c["x"])
    assert isinstance(pre.n_samples_fit, np.integer)
    assert pre.bc_mask is c["bc_mask"] and pre.precip_mask is c["precip_mask"]
    assert_close(pre.transform(x), FIX[f"{name}/transform"], 1e-10, "transform")


def test_api_equals_reference_fixture():
    a, k, window = api_case()
    pre = HmsPreProcessor()
    out = pre.calc_antecedent_precipitation_index(a, k=k, window=window)
    want = FIX["api/window"]
    assert out.shape == want.shape == (len(a), 1)
    assert np.max(np.abs(out - want)) <= 1e-12 * np.max(np.abs(want))
    assert_close(pre.calc_antecedent_precipitation_index(a), FIX["api/default"], 1e-12, "api default")


@pytest.mark.parametrize("n, k, window", [(100_000, 0.85, None), (100_000, 1, None), (30_000, 0.9, 700), (257, 1, 1), (1000, 0.85, 5000),
                                          (5, 0.85, None)])
def test_api_against_convolve(n, k, window):
    rng = np.random.default_rng(n + int(100 * k))
    a = rng.standard_normal(n) * (rng.random(n) < 0.4)
    out = HmsPreProcessor().calc_antecedent_precipitation_index(a, k=k, window=window)
    W = n if window is None else window
    if W <= 5000:
        want = api(a, k, window)
        w = np.abs(np.array([k**i for i in range(W)]))
        bound = np.convolve(np.abs(a), w, mode="full")[:n]
    else:  # the O(T W) convolution with the zero tail cut (k < 1) or an extended-precision running sum (k = 1)
        want = api_fast(a, k)
        bound = api_fast(np.abs(a), k)[:, 0]
    assert out.shape == (n, 1)
    assert np.all(np.abs(out[:, 0] - want[:, 0]) <= 1e-12 * bound + 1e-300)


def test_api_nonfinite_input_keeps_the_zero_tail():
    a = np.zeros(6000)
    a[10] = np.inf
    out = HmsPreProcessor().calc_antecedent_precipitation_index(a)
    want = api(a)
    assert np.array_equal(np.isnan(out), np.isnan(want)) and np.array_equal(np.isinf(out), np.isinf(want))
    assert np.isnan(out[5000, 0])  # 0.85**4990 == 0, and 0 * inf is NaN in np.convolve too


def test_large_fit_equals_restatement():
    rng = np.random.default_rng(5)
    T, p, n_bc = 200_000, 400, 4
    r = 8
    scales = 3.0 * 0.6 ** np.arange(r)
    amp = rng.standard_normal((T, r)) * scales
    pat = rng.standard_normal((r, p))
    x = np.empty((T, n_bc + p))
    x[:, n_bc:] = 2.0 + 0.3 * amp @ pat + 0.02 * rng.random((T, p))
    x[:, :n_bc] = 40.0 + 5.0 * rng.standard_normal((T, n_bc))
    pm = np.zeros(n_bc + p, dtype=bool)
    pm[n_bc:] = True
    x = np.asfortranarray(x)
    want = fit_reference(x, ~pm, pm, None, fast_api=True)
    pre = HmsPreProcessor()
    pre.fit(x, ~pm, pm)
    assert pre.precip_spatial_mode_count == want["precip_spatial_mode_count"] > 0
    assert_fit_close({a: getattr(pre, a) for a in ATTRS}, want, x)
    state = dict(want, bc_mask=~pm, precip_mask=pm)
    rows = slice(0, 20_000)
    assert_close(pre.transform(x[rows])[:, : n_bc + pre.eofs.shape[0] + 1], transform_reference(state, x[rows], True)[:, : n_bc + pre.eofs.shape[0] + 1],
                 1e-10, "transform")


def test_two_fits_identical_bits_and_transform_is_causal():
    c = CASES["t_gt_5p_north"]
    a, b = device_fit(c), device_fit(c)
    for key in ATTRS:
        assert np.array_equal(np.asarray(getattr(a, key)), np.asarray(getattr(b, key))), key
    rng = np.random.default_rng(3)
    x = np.repeat(c["x"], 20, axis=0) + 0.01 * rng.standard_normal((20 * c["x"].shape[0], c["x"].shape[1]))
    full = a.transform(x)
    for n in (1, 255, 256, 257, 3000, x.shape[0] - 1):
        assert np.array_equal(a.transform(x[:n]), full[:n]), n


def test_k_beyond_the_component_count():
    c = CASES["t_mid"]  # T > p: every component exists, a larger k keeps the reference's slice
    p = int(FIX["t_mid/eofs"].shape[1])
    pre = HmsPreProcessor()
    pre.fit(c["x"], c["bc_mask"], c["precip_mask"], p + 3)
    assert pre.precip_spatial_mode_count == p + 3 and pre.eofs.shape == (p, p)
    assert pre.x_mean.shape == (int(np.sum(c["bc_mask"])) + p + 3,)
    c = CASES["t_lt_p"]  # T < p: the Gram route divides by sqrt(lambda); no direction beyond the rank
    with pytest.raises(ValueError):
        HmsPreProcessor().fit(c["x"], c["bc_mask"], c["precip_mask"], c["x"].shape[0])


def _raw_hms(rows, n_bc, n_precip, n_other=0, with_mean=False):
    """A gprx_hms handle over random x: columns [bc | precip | unused], created with or without input_mean."""
    import ctypes as C

    from gpras_amd import _lib
    from gpras_amd._lib import ptr

    lib = _lib.load()
    n_f = n_bc + n_precip + n_other
    x = np.random.default_rng(100 * rows + n_f).standard_normal((rows, n_f))
    bc, pc = np.arange(n_bc, dtype=np.int64), np.arange(n_bc, n_bc + n_precip, dtype=np.int64)
    mean = x.mean(axis=0)
    h = C.c_void_p()
    _lib.check(lib.gprx_hms_create(0, ptr(x), rows, n_f, n_f, 0, ptr(bc) if n_bc else None, n_bc, ptr(pc), n_precip, ptr(mean) if with_mean else None,
                                   C.byref(h)))
    return lib, h, n_f


def test_call_order_of_the_handle_is_enforced():
    """gprx_hms_cov runs once and only on a handle created without input_mean; gprx_hms_features needs input_mean from either;
    gprx_hms_components belongs to the Gram route alone."""
    import ctypes as C

    from gpras_amd import _lib
    from gpras_amd._lib import ptr

    lib, h, n_f = _raw_hms(8, 1, 4, n_other=1)
    try:
        mean, cov, route = np.empty(n_f), np.empty((4, 4)), C.c_int(-1)
        x_mean, x_std = np.empty(4), np.empty(4)  # n_bc + 0 components + 3
        assert lib.gprx_hms_features(h, 0, None, None, 0, None, 0, ptr(x_mean), ptr(x_std), 1, None) == _lib.GPRX_ESTATE
        assert lib.gprx_hms_cov(h, ptr(mean), ptr(cov), C.byref(route)) == _lib.GPRX_OK
        assert route.value == 0  # HMS_COV: rows >= precip columns
        assert lib.gprx_hms_cov(h, ptr(mean), ptr(cov), C.byref(route)) == _lib.GPRX_ESTATE
        u, lam, eofs = np.eye(8)[:, :2].copy(), np.ones(2), np.empty((2, 4))
        assert lib.gprx_hms_components(h, 2, ptr(u), ptr(lam), ptr(eofs)) == _lib.GPRX_ESTATE
    finally:
        lib.gprx_hms_destroy(h)
    lib, h, n_f = _raw_hms(8, 1, 4, n_other=1, with_mean=True)
    try:
        assert lib.gprx_hms_cov(h, ptr(mean), ptr(cov), C.byref(route)) == _lib.GPRX_ESTATE
    finally:
        lib.gprx_hms_destroy(h)


def test_components_step_checks_k_and_the_retained_eigenvalues():
    """The same two checks in gprx_hms_components (Gram route) and gprx_pcafit_components: k < rows, eigenvalues positive."""
    import ctypes as C

    from gpras_amd import _lib
    from gpras_amd._lib import ptr

    u4, u2, lam4, bad = np.eye(4), np.eye(4)[:, :2].copy(), np.ones(4), np.array([1.0, 0.0])
    eofs, z = np.empty((4, 40)), np.empty((4, 4))
    lib, h, n_f = _raw_hms(4, 0, 40)
    try:
        mean, cov, route = np.empty(n_f), np.empty((4, 4)), C.c_int(-1)
        assert lib.gprx_hms_cov(h, ptr(mean), ptr(cov), C.byref(route)) == _lib.GPRX_OK and route.value == 1  # HMS_GRAM
        assert lib.gprx_hms_components(h, 4, ptr(u4), ptr(lam4), ptr(eofs)) == _lib.GPRX_EINVAL
        assert lib.gprx_hms_components(h, 2, ptr(u2), ptr(bad), ptr(eofs)) == _lib.GPRX_EINVAL
        assert b"positive" in lib.gprx_hms_last_error(h)
    finally:
        lib.gprx_hms_destroy(h)
    x = np.random.default_rng(7).standard_normal((4, 40))
    h = C.c_void_p()
    _lib.check(lib.gprx_pcafit_create(0, ptr(x), 4, 40, None, None, 2, 0.0, C.byref(h)))  # velocity: every cell is wet
    try:
        assert lib.gprx_pcafit_components(h, 4, ptr(u4), ptr(lam4), ptr(eofs), ptr(z)) == _lib.GPRX_EINVAL
        assert lib.gprx_pcafit_components(h, 2, ptr(u2), ptr(bad), ptr(eofs), ptr(z)) == _lib.GPRX_EINVAL
        assert b"positive" in lib.gprx_pcafit_last_error(h)
    finally:
        lib.gprx_pcafit_destroy(h)


def test_pickle_round_trips_both_ways(tmp_path):
    c = CASES["dry_cells"]
    pre = device_fit(c)
    path = tmp_path / "hms.pkl"
    pre.to_file(path)
    with open(path, "rb") as f:
        d = pickle.load(f)
    assert type(d) is dict and b"gpras_amd" not in path.read_bytes()
    back = HmsPreProcessor.from_file(path)
    assert np.array_equal(pre.transform(c["x"]), back.transform(c["x"]))
    # a dict in the reference's format, made from the reference's own fit, transforms like the reference
    rec = {a: FIX[f"dry_cells/{a}"] for a in ATTRS}
    ref = dict(rec, bc_mask=c["bc_mask"], precip_mask=c["precip_mask"], precip_spatial_mode_count=int(rec["precip_spatial_mode_count"]),
               n_samples_fit=np.int64(rec["n_samples_fit"]))
    path2 = tmp_path / "ref.pkl"
    with open(path2, "wb") as f:
        pickle.dump(ref, f)
    assert_close(HmsPreProcessor.from_file(path2).transform(c["x"]), FIX["dry_cells/transform"], 1e-10, "transform")
