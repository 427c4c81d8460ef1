"""``PreProcessor.fit`` with the eigendecomposition on the device (``eigensolver = "device"``: gprx_pcafit_eig and
gprx_pcafit_components_dev, DESIGN.md sections 3.12 and 3.16): parity with the reference's own fit and the numpy restatement
under the bounds of the host route, exact agreement of both routes on everything that is not floating-point linear algebra,
determinism, and no download of the Gram matrix."""

import os
import sys

import numpy as np
import pytest

from gpras_amd import _lib
from gpras_amd.preprocess import PreProcessor
from pca_fit_numpy import assert_fit_close, fit_reference

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_pca_fit_ref import THRESHOLD, pca_fit_ref_cases  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(GOLDEN, "pca_fit_ref_golden.npz"))
CASES = pca_fit_ref_cases()
ATTRS = ("wetness_classes", "input_mean", "weights", "eofs", "eigenvalues", "spatial_mode_count", "n_samples_fit", "x_mean", "x_std")
SHAPES = [(16, 1000, "wse", True, 1), (65, 20000, "velocity", True, 3), (200, 100000, "depth", True, 5), (300, 5000, "wse", False, 6)]


class DevicePreProcessor(PreProcessor):
    eigensolver = "device"


def fit(cls, c, k=None):
    pre = cls(wet_threshold=THRESHOLD, hydraulic_parameter=c["mode"])
    pre.fit(c["x"], c["elevations"], c["weights"], c["k"] if k is None else k)
    return pre


def random_case(n_s, cells, mode, weighted, seed):
    """The generator of test_random_shapes_equal_restatement (tests/test_gpu_pca_fit.py)."""
    rng = np.random.default_rng(seed)
    r = 6
    scales = 3.0 * 0.6 ** np.arange(r)
    elev = 10.0 + 2.0 * rng.random(cells)
    elev[rng.random(cells) < 0.1] += 50.0
    x = 11.0 + 0.5 * (rng.standard_normal((n_s, r)) * scales) @ rng.standard_normal((r, cells)) + 0.01 * rng.standard_normal((n_s, cells))
    return dict(x=x, elevations=elev, weights=0.5 + rng.random(cells) if weighted else None, mode=mode, k=5)


@pytest.fixture(scope="module")
def random_fits():
    """(case, device-route fit, host-route fit) per shape, computed once."""
    out = {}
    for shape in SHAPES:
        c = random_case(*shape)
        out[shape] = (c, fit(DevicePreProcessor, c), fit(PreProcessor, c))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_route_equals_reference(name):
    c = CASES[name]
    pre = fit(DevicePreProcessor, c)
    got = {a: getattr(pre, a) for a in ATTRS}
    assert_fit_close(got, {a: FIX[f"{name}/{a}"] for a in ATTRS})
    assert "eigensolver" in pre.last_timings_ms and pre.last_eig_sweeps >= 1
    assert "eigensolver" not in pre.to_dict()


@pytest.mark.parametrize("shape", SHAPES)
def test_device_route_equals_restatement(random_fits, shape):
    c, dev, _ = random_fits[shape]
    want = fit_reference(c["x"], c["elevations"], c["weights"], c["k"], c["mode"], THRESHOLD)
    assert_fit_close({a: getattr(dev, a) for a in ATTRS}, want)


@pytest.mark.parametrize("shape", SHAPES)
def test_both_routes_agree_exactly_where_no_eigensolver_is_involved(random_fits, shape):
    c, dev, host = random_fits[shape]
    for key in ("wetness_classes", "input_mean", "weights"):
        assert np.array_equal(np.asarray(getattr(dev, key)), np.asarray(getattr(host, key))), key
    # the mode count North's rule picks from either route's eigenvalues
    a = DevicePreProcessor(wet_threshold=THRESHOLD, hydraulic_parameter=c["mode"])
    b = PreProcessor(wet_threshold=THRESHOLD, hydraulic_parameter=c["mode"])
    a.fit(c["x"], c["elevations"], c["weights"], None)
    b.fit(c["x"], c["elevations"], c["weights"], None)
    assert a.spatial_mode_count == b.spatial_mode_count
    assert np.array_equal(a.wetness_classes, b.wetness_classes) and np.array_equal(a.input_mean, b.input_mean)


def test_two_device_route_fits_identical_bits():
    c = CASES["depth_w_north"]
    a, b = fit(DevicePreProcessor, c), fit(DevicePreProcessor, c)
    for key in ATTRS:
        assert np.array_equal(np.asarray(getattr(a, key)), np.asarray(getattr(b, key))), key


class _Recorder:
    """Stands in for the loaded library and records the names of the entry points a fit calls."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._lib, name)


def test_device_route_downloads_no_gram_matrix(monkeypatch):
    rec = _Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    c = CASES["wse_w_north"]
    fit(DevicePreProcessor, c)
    assert "gprx_pcafit_eig" in rec.calls and "gprx_pcafit_components_dev" in rec.calls
    assert "gprx_pcafit_gram" not in rec.calls and "gprx_pcafit_components" not in rec.calls
    rec.calls.clear()
    fit(PreProcessor, c)
    assert "gprx_pcafit_gram" in rec.calls and "gprx_pcafit_eig" not in rec.calls


def test_instance_attribute_selects_the_route_too():
    c = CASES["wse_w_north"]
    pre = PreProcessor(wet_threshold=THRESHOLD, hydraulic_parameter=c["mode"])
    pre.eigensolver = "device"
    pre.fit(c["x"], c["elevations"], c["weights"], c["k"])
    assert "eigensolver" in pre.last_timings_ms


def _raw_handle(c):
    import ctypes as C

    from gpras_amd._lib import as_f64, ptr
    from gpras_amd.preprocess import MODES

    lib = _lib.load()
    x, elev, w = as_f64(c["x"]), as_f64(c["elevations"]), as_f64(c["weights"])
    h = C.c_void_p()
    _lib.check(lib.gprx_pcafit_create(0, ptr(x), x.shape[0], x.shape[1], ptr(elev), ptr(w), MODES.index(c["mode"]), THRESHOLD, C.byref(h)))
    return lib, h, x.shape


def test_the_gram_matrix_cannot_come_down_once_the_device_route_has_run():
    """create downloads nothing of size n_s^2; G comes down only through gprx_pcafit_gram, and after gprx_pcafit_eig (which
    overwrites G on the device) that call is GPRX_ESTATE: a fit that took the device route has never had G on the host."""
    import ctypes as C

    from gpras_amd._lib import ptr

    c = CASES["wse_w_north"]
    lib, h, (n_s, cells) = _raw_handle(c)
    try:
        codes, mean, lam, gram = np.empty(cells, dtype=np.uint8), np.empty(cells), np.empty(n_s), np.full((n_s, n_s), -1.0)
        n_wet, sweeps = C.c_int64(), C.c_int()
        assert lib.gprx_pcafit_eig(h, ptr(codes), ptr(mean), ptr(lam), C.byref(n_wet), C.byref(sweeps)) == _lib.GPRX_OK
        assert lib.gprx_pcafit_gram(h, ptr(codes), ptr(mean), ptr(gram), C.byref(n_wet)) == _lib.GPRX_ESTATE
        assert np.all(gram == -1.0)
        assert lib.gprx_pcafit_eig(h, ptr(codes), ptr(mean), ptr(lam), C.byref(n_wet), C.byref(sweeps)) == _lib.GPRX_ESTATE
    finally:
        lib.gprx_pcafit_destroy(h)


def test_call_order_gram_first_then_eig_agree_and_eig_after_components_is_refused():
    import ctypes as C

    from gpras_amd._lib import ptr

    c = CASES["wse_w_north"]
    lib, h, (n_s, cells) = _raw_handle(c)
    try:
        codes, mean, lam, gram = np.empty(cells, dtype=np.uint8), np.empty(cells), np.empty(n_s), np.empty((n_s, n_s))
        n_wet, sweeps = C.c_int64(), C.c_int()
        assert lib.gprx_pcafit_gram(h, ptr(codes), ptr(mean), ptr(gram), C.byref(n_wet)) == _lib.GPRX_OK
        assert lib.gprx_pcafit_eig(h, ptr(codes), ptr(mean), ptr(lam), C.byref(n_wet), C.byref(sweeps)) == _lib.GPRX_OK
        want = np.linalg.eigvalsh(gram)[::-1]
        assert np.max(np.abs(lam - want)) <= 1e-12 * want[0]
        gram2 = np.empty_like(gram)  # the host copy made by the first call is still served
        assert lib.gprx_pcafit_gram(h, ptr(codes), ptr(mean), ptr(gram2), C.byref(n_wet)) == _lib.GPRX_OK
        assert np.array_equal(gram, gram2)
    finally:
        lib.gprx_pcafit_destroy(h)
    lib, h, _ = _raw_handle(c)
    try:
        assert lib.gprx_pcafit_gram(h, ptr(codes), ptr(mean), ptr(gram), C.byref(n_wet)) == _lib.GPRX_OK
        lam_h, u = np.linalg.eigh(gram)
        u_k, lam_k = np.ascontiguousarray(u[:, ::-1][:, :2]), np.ascontiguousarray(lam_h[::-1][:2])
        eofs, z = np.empty((2, n_wet.value)), np.empty((n_s, 2))
        assert lib.gprx_pcafit_components(h, 2, ptr(u_k), ptr(lam_k), ptr(eofs), ptr(z)) == _lib.GPRX_OK
        assert lib.gprx_pcafit_eig(h, ptr(codes), ptr(mean), ptr(lam), C.byref(n_wet), C.byref(sweeps)) == _lib.GPRX_ESTATE
    finally:
        lib.gprx_pcafit_destroy(h)
