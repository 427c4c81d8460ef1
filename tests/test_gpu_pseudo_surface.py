"""The pseudo-surface low-fidelity model on the device (gpras_amd/csrc/pseudo.h, gpras_amd/pseudo_surface.py) against the reference's
own outputs (tests/golden/pseudo_ref_golden.npz) and the numpy restatement (tests/pseudo_numpy.py).

Bounds.  Bit for bit: the centerline fit (a median selects; (a + b) / 2 is one rounding), interpolate_centerline, interpolate_surface
and the two floors when fed the reference's own boundary elevations -- the same IEEE operations in the same order.  Spline
evaluation: 4 x eps_spline relative to the reference, eps_spline being the recorded difference between the restatement and
FITPACK (the fixture in the tree records 0: the restatement follows fpbspl / splev operation by operation, and so does the kernel).
From flows: 4 x eps_spline x max(|us_wse|, |ds_wse|) x (max|1 - w| + max|w|) per element, every later step being 1-Lipschitz in the
boundary elevations up to the weights.  lf_features against the host chain of existing entries: bit for bit, the row slabs agreeing.
"""

import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pseudo_numpy
from gpras_amd._lib import GPRX_EINVAL, GPRX_ESTATE, GPRX_OK, DeviceBuffer, ptr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_pseudo_ref import N_CELLS, N_CENTERLINE, pseudo_ref_cases  # noqa: E402

FIX = np.load(os.path.join(GOLDEN, "pseudo_ref_golden.npz"))
CASES = pseudo_ref_cases()
EPS = float(FIX["eps_spline"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64)[~np.isnan(b)], b.view(np.int64)[~np.isnan(b)]) and np.array_equal(np.isnan(a), np.isnan(b))


def curves():
    from gpras_amd.pseudo_surface import RatingCurve

    return [RatingCurve.from_arrays(FIX[f"curve/{n}/knots"], FIX[f"curve/{n}/coefficients"]) for n in ("us", "ds")]


def estimator(name="a", w=True):
    from gpras_amd.pseudo_surface import PseudoSurface

    c = CASES["surfaces"][name]
    us, ds = curves()
    return PseudoSurface(c["elev"], c["idx"], us, ds, FIX[f"fit/{c['fit']}/cl_interpolater"] if w else None, n_centerline=N_CENTERLINE)


def flow_bound(us_wse, ds_wse, w):
    return 4.0 * EPS * np.maximum(np.abs(us_wse), np.abs(ds_wse)).reshape(-1, 1) * (np.max(np.abs(1.0 - w)) + np.max(np.abs(w)))


# ---- rating curves -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["us", "ds"])
def test_spline_eval_against_the_reference(lib, name):
    knots, coef = FIX[f"curve/{name}/knots"], FIX[f"curve/{name}/coefficients"]
    queries = dict(CASES["curves"][name]["queries"], knots=knots)
    worst = 0.0
    for qn, qv in queries.items():
        want = FIX[f"curve/{name}/predict/{qn}"]
        x = np.ascontiguousarray(qv, dtype=np.float64)
        got = np.empty_like(x)
        assert lib.gprx_spline_eval(0, ptr(knots), len(knots), ptr(coef), ptr(x), x.size, ptr(got)) == GPRX_OK
        err = float(np.max(np.abs(got - want) / np.abs(want)))
        print(f"spline {name}/{qn}: max relative difference {err:.3e} (bound {4 * EPS:.3e})")
        worst = max(worst, err)
        assert same_bits(got, pseudo_numpy.spline_eval(knots, coef, x)), qn  # the restatement, operation by operation
    assert worst <= 4.0 * EPS


def test_rating_curve_predict_shapes_nan_and_fit_stats(lib):
    from gpras_amd.pseudo_surface import RatingCurve

    c = CASES["curves"]["us"]
    rc = RatingCurve(c["q"], c["wse"])
    col = c["queries"]["column"]
    got = rc.predict(col)
    assert got.shape == col.shape == (57, 1)
    assert np.max(np.abs(got - FIX["curve/us/predict/column"]) / np.abs(FIX["curve/us/predict/column"])) <= max(4.0 * EPS, 1e-12)
    x = np.array([[np.nan, 100.0, -np.inf], [1e3, np.nan, 5.0]])
    out = rc.predict(x)
    assert np.array_equal(np.isnan(out), [[True, False, True], [False, True, False]])
    stats = rc.fit_stats
    np.testing.assert_allclose([stats["rmse"], stats["mae"]], FIX["curve/us/fit_stats"], rtol=1e-9)
    big = np.linspace(5.0, 4e4, 100_003)  # more arguments than one pass of the grid
    assert same_bits(rc.predict(big), pseudo_numpy.spline_eval(rc.knots, rc.coefficients, big))


def test_spline_and_handle_argument_errors(lib):
    knots, coef = FIX["curve/us/knots"], FIX["curve/us/coefficients"]
    x = np.ones(3)
    out = np.empty(3)
    assert lib.gprx_spline_eval(0, ptr(knots), 7, ptr(coef), ptr(x), 3, ptr(out)) == GPRX_EINVAL
    bad = knots.copy()
    bad[5] = bad[7]
    bad[6] = bad[4]
    assert lib.gprx_spline_eval(0, ptr(bad), len(bad), ptr(coef), ptr(x), 3, ptr(out)) == GPRX_EINVAL
    assert b"non-decreasing" in lib.gprx_ps_last_error(None)
    c = CASES["surfaces"]["a"]
    idx = np.ascontiguousarray(c["idx"], dtype=np.int32)
    idx[7] = N_CENTERLINE
    h = C.c_void_p()
    assert lib.gprx_ps_create(0, N_CELLS, ptr(c["elev"]), ptr(idx), N_CENTERLINE, None, None, 0, None, None, 0, None, C.byref(h)) == GPRX_EINVAL
    idx[7] = 0
    assert lib.gprx_ps_create(0, N_CELLS, ptr(c["elev"]), ptr(idx), N_CENTERLINE, None, None, 0, None, None, 0, None, C.byref(h)) == GPRX_OK
    try:
        out = np.empty((2, N_CELLS))
        assert lib.gprx_ps_surface(h, None, ptr(out)) == GPRX_ESTATE  # no boundary series
        us = np.ones(2)
        assert lib.gprx_ps_rating(h, ptr(us), ptr(us), 2, None, None) == GPRX_ESTATE  # no curves
        assert lib.gprx_ps_set_boundaries(h, ptr(us), ptr(us), 2) == GPRX_OK
        buf = DeviceBuffer(out.nbytes)
        assert lib.gprx_ps_surface_dev(h, 0, 2, None, N_CELLS, buf.ptr, N_CELLS) == GPRX_ESTATE  # no weights
        w = np.zeros(N_CENTERLINE)
        assert lib.gprx_ps_set_weights(h, ptr(w)) == GPRX_OK
        assert lib.gprx_ps_surface_dev(h, 1, 2, None, N_CELLS, buf.ptr, N_CELLS) == GPRX_EINVAL  # rows beyond the series
        assert lib.gprx_ps_surface_dev(h, 0, 2, None, N_CELLS, buf.ptr, N_CELLS - 1) == GPRX_EINVAL
        assert lib.gprx_ps_surface_dev(h, 0, 2, buf.ptr, N_CELLS + 1, buf.ptr, N_CELLS) == GPRX_EINVAL  # in place, unequal pitch
        zq, block = np.zeros(2), np.ones((2, N_CENTERLINE))
        assert lib.gprx_ps_fit_centerline(h, ptr(us), ptr(us), ptr(zq), ptr(zq), ptr(block), 2, ptr(w)) == GPRX_EINVAL
        buf.free()
    finally:
        lib.gprx_ps_destroy(h)


# ---- centerline fit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "even", "nan_column", "ties"])
def test_fit_centerline_equals_the_reference_bit_for_bit(lib, name):
    c = CASES["fits"][name]
    ps = estimator(w=False)
    got = ps.fit_centerline(c["us_wse"], c["ds_wse"], c["us_q"], c["ds_q"], c["wse"])
    want = FIX[f"fit/{name}/cl_interpolater"]
    assert same_bits(got, want), np.flatnonzero(got != want)
    assert same_bits(ps.fit_centerline(c["us_wse"][:, None], c["ds_wse"], c["us_q"], c["ds_q"], c["wse"]), got)  # twice: the same bits
    ps.close()


@pytest.mark.parametrize("rows,cols,seed", [(4001, 70, 1), (4000, 9, 2), (1, 8, 3), (2, 5, 4), (33, 1, 5)])
def test_fit_centerline_equals_numpy_median_on_larger_blocks(lib, rows, cols, seed):
    """Many rows per thread, ties (values rounded to a coarse grid in some columns), infinities, exact zeros, masked rows."""
    from gpras_amd.pseudo_surface import PseudoSurface

    rng = np.random.default_rng(seed)
    us = 100.0 + rng.random(rows)
    ds = us - 1.0 - rng.random(rows)
    wse = us[:, None] - (us - ds)[:, None] * rng.standard_normal((rows, cols))
    wse[:, ::3] = np.round(wse[:, ::3], 1)  # ties
    if rows > 10:
        ds[5] = us[5]  # +-inf
        wse[7, :] = us[7]  # zeros
    us_q = np.where(rng.random(rows) < 0.2, 0.0, 5.0)
    ds_q = np.where(rng.random(rows) < 0.5, -1.0, 2.0)
    us_q[0] = 1.0
    keep = (us_q > 0) | (ds_q > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.median((us[keep, None] - wse[keep]) / (us[keep] - ds[keep])[:, None], axis=0)
    ps = PseudoSurface(np.zeros(3), np.zeros(3, dtype=np.int64), None, None, n_centerline=cols)
    got = ps.fit_centerline(us, ds, us_q, ds_q, wse)
    ps.close()
    assert np.array_equal(got, want, equal_nan=True), np.flatnonzero(got != want)
    assert same_bits(got, pseudo_numpy.fit_centerline(us, ds, us_q, ds_q, wse))


# ---- surfaces ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b"])
def test_surfaces_from_the_reference_boundaries_bit_for_bit(lib, name):
    c = CASES["surfaces"][name]
    ps = estimator(name)
    us, ds = FIX[f"surface/{name}/us_wse"], FIX[f"surface/{name}/ds_wse"]  # (T, 1), as the reference passes them
    cl = ps.interpolate_centerline(us, ds)
    assert same_bits(cl, FIX[f"surface/{name}/centerline"])
    assert same_bits(ps.interpolate_surface(cl), FIX[f"surface/{name}/gathered"])
    full = ps.surface_from_wse(us, ds, c["fluvial"])
    assert same_bits(full, FIX[f"surface/{name}/lf_plan_data"])
    assert same_bits(ps.surface_from_wse(us, ds, c["fluvial"]), full)  # twice: the same bits
    n = 5
    assert same_bits(ps.surface_from_wse(us[:n], ds[:n], c["fluvial"][:n]), full[:n])  # the first rows alone
    w = FIX[f"fit/{c['fit']}/cl_interpolater"]
    assert same_bits(ps.surface_from_wse(us, ds), pseudo_numpy.surface(us, ds, w, c["idx"], c["elev"]))  # no fluvial floor
    dev = DeviceBuffer.from_array(c["fluvial"])
    assert same_bits(ps.surface_from_wse(us, ds, dev), full)
    dev.free()
    ps.close()


@pytest.mark.parametrize("name", ["a", "b"])
def test_lf_plan_data_from_flows_within_the_derived_bound(lib, name):
    c = CASES["surfaces"][name]
    ps = estimator(name)
    w = FIX[f"fit/{c['fit']}/cl_interpolater"]
    want = FIX[f"surface/{name}/lf_plan_data"]
    got = ps.lf_plan_data(c["us_q"][:, None], c["ds_q"][:, None], c["fluvial"])
    bound = flow_bound(FIX[f"surface/{name}/us_wse"], FIX[f"surface/{name}/ds_wse"], w)
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok)
    diff = np.where(ok, np.abs(got - np.where(ok, want, 0.0)), 0.0)
    print(f"lf_plan_data {name}: max |difference| {diff.max():.3e}, bound {bound.max():.3e}")
    assert np.all(diff <= bound)
    ps.close()


@pytest.mark.parametrize("ld_out,ld_fl,cells", [(112, 101, 101), (102, 102, 102), (103, 101, 101), (20016, 20001, 20001)])
def test_surface_dev_pitches_padding_and_in_place(lib, ld_out, ld_fl, cells):
    """Every vector / scalar combination of the loads and stores, the zeroed padding, more centerline cells than LDS holds."""
    from gpras_amd.pseudo_surface import PseudoSurface

    rng = np.random.default_rng(cells + ld_out)
    n_cl = 9000 if cells > 1000 else 37
    T = 19
    elev, idx, w = 100.0 + rng.random(cells), rng.integers(0, n_cl, cells), rng.random(n_cl)
    us = 102.0 + rng.random(T)
    ds = us - rng.random(T)
    fl = 100.0 + 3.0 * rng.random((T, ld_fl))
    fl[2, 1] = np.nan
    ps = PseudoSurface(elev, idx, None, None, w)
    ps._set_boundaries(us, ds)
    want = pseudo_numpy.surface(us, ds, w, idx, elev, fl[:, :cells])
    fdev = DeviceBuffer.from_array(fl)
    odev = DeviceBuffer.from_array(np.full((T, ld_out), np.nan))
    try:
        assert lib.gprx_ps_surface_dev(ps.handle, 0, T, fdev.ptr, ld_fl, odev.ptr, ld_out) == GPRX_OK
        assert lib.gprx_ps_synchronize(ps.handle) == GPRX_OK
        got = odev.to_array((T, ld_out))
        assert same_bits(got[:, :cells], want)
        assert np.all(got[:, cells:] == 0.0)
        assert lib.gprx_ps_surface_dev(ps.handle, 3, T - 3, fdev.at(3 * ld_fl), ld_fl, fdev.at(3 * ld_fl), ld_fl) == GPRX_OK  # in place
        assert lib.gprx_ps_synchronize(ps.handle) == GPRX_OK
        inplace = fdev.to_array((T, ld_fl))
        assert same_bits(inplace[3:, :cells], want[3:]) and same_bits(inplace[:3], fl[:3])
        assert np.all(inplace[3:, cells:] == 0.0)
    finally:
        fdev.free()
        odev.free()
        ps.close()


def test_surface_kernel_indexes_past_two_to_the_31(lib):
    """T x n_cells = 2 200 x 1 000 002 > 2^31 elements, no fluvial operand: one 17.6 GB output; rows on both sides of element 2^31."""
    from gpras_amd.pseudo_surface import PseudoSurface

    T, cells, n_cl = 2200, 1_000_002, 1000
    assert T * cells > 2**31
    rng = np.random.default_rng(31)
    elev, idx, w = 100.0 + 4.0 * rng.random(cells), rng.integers(0, n_cl, cells), rng.random(n_cl)
    us = 103.0 + rng.random(T)
    ds = us - 2.0 * rng.random(T)
    ps = PseudoSurface(elev, idx, None, None, w)
    ps._set_boundaries(us, ds)
    out = DeviceBuffer(8 * T * cells)
    try:
        assert lib.gprx_ps_surface_dev(ps.handle, 0, T, None, cells, out.ptr, cells) == GPRX_OK
        assert lib.gprx_ps_synchronize(ps.handle) == GPRX_OK
        first_past = 2**31 // cells  # the row that holds element 2^31
        for t in (0, 1, 1100, first_past - 1, first_past, first_past + 1, T - 2, T - 1):
            row = np.empty(cells)
            assert lib.gprx_memcpy_d2h(0, ptr(row), out.at(t * cells), row.nbytes) == GPRX_OK
            assert same_bits(row, pseudo_numpy.surface(us[t : t + 1], ds[t : t + 1], w, idx, elev)[0]), t
    finally:
        out.free()
        ps.close()


# ---- flows to features ---------------------------------------------------------------------------------------------------------------
def _feature_setup(T, seed=5, n=96, d=3, kf=4, k=6):
    from gpras_amd.gpr import GPRAS
    from gpras_amd.preprocess import EOFProjector

    rng = np.random.default_rng(seed)
    c = CASES["surfaces"]["b"]
    cells = N_CELLS
    x = rng.normal(size=(n, d))
    y = np.stack([np.sin(x @ rng.normal(size=d)) + 0.05 * rng.normal(size=n) for _ in range(kf)], axis=1)
    gpr = GPRAS("Matern32")
    gpr.fit(x, y, 16, "grid", "adam", max_iter=6)

    def projector(modes, level, spread):
        dry = np.zeros(cells, dtype=bool)
        dry[[3, 17, 100]] = True
        n_wet = cells - 3
        return EOFProjector(dry, c["elev"], level + rng.normal(size=n_wet), rng.uniform(0.5, 1.5, size=n_wet),
                            spread * rng.normal(size=(modes, n_wet)) / np.sqrt(modes), rng.normal(size=modes), rng.uniform(0.5, 2, size=modes), "wse")

    fluvial_proj = projector(kf, 116.0, 6.0)  # a fluvial field that wins in places
    hf_proj = projector(k, 115.0, 1.0)
    us_q = 10.0 ** rng.uniform(0.8, 4.6, T)
    ds_q = us_q * rng.uniform(0.8, 1.3, T)
    return gpr, fluvial_proj, hf_proj, rng.normal(size=(T, d)), us_q, ds_q


def _check_features(T):
    from gpras_amd.pipeline import DevicePipeline

    gpr, fluvial_proj, hf_proj, fx, us_q, ds_q = _feature_setup(T)
    ps = estimator("b")
    # the fluvial leg alone: the device field equals the host chain of existing entries
    fluvial_host = fluvial_proj.reverse_transform(gpr.predict(fx)[0])
    dev, ns = DevicePipeline(gpr, fluvial_proj).predict_mean_field_dev(fx)
    assert ns == T and same_bits(dev.to_array((T, N_CELLS)), fluvial_host)
    lf = ps.lf_plan_data(us_q, ds_q, fluvial_host)
    assert same_bits(ps.lf_plan_data(us_q, ds_q, dev), lf)
    dev.free()
    assert np.mean(lf == fluvial_host) > 0.02 and np.mean(lf > fluvial_host) > 0.02  # the fluvial floor acts, and not everywhere
    want = hf_proj.transform(lf)
    got = ps.lf_features(us_q, ds_q, hf_proj, fluvial_x=fx, fluvial_gpr=gpr, fluvial_projector=fluvial_proj)
    assert got.shape == (T, hf_proj.spatial_mode_count) and same_bits(got, want), float(np.max(np.abs(got - want)))
    assert same_bits(ps.lf_features(us_q, ds_q, hf_proj, fluvial_x=fx, fluvial_gpr=gpr, fluvial_projector=fluvial_proj), got)
    assert same_bits(ps.lf_features(us_q, ds_q, hf_proj), hf_proj.transform(ps.lf_plan_data(us_q, ds_q)))  # without the fluvial floor
    with pytest.raises(ValueError):
        ps.lf_features(us_q, ds_q, hf_proj, fluvial_x=fx)
    ps.close()
    return got


def test_lf_features_equal_the_host_chain_inside_one_slab(lib):
    _check_features(37)


def test_lf_features_equal_the_host_chain_over_three_slabs(lib):
    """GPRX_PCA_CHUNK_DOUBLES = 64 x 112 in a child process: slabs of 64 rows, T = 150 = 64 + 64 + 22."""
    code = "import sys; sys.path.insert(0, 'tests'); import test_gpu_pseudo_surface as t; z = t._check_features(150); print('slabs ok', z.shape)"
    env = dict(os.environ, GPRX_PCA_CHUNK_DOUBLES=str(64 * 112))
    res = subprocess.run([sys.executable, "-c", code], env=env, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0 and "slabs ok (150, 6)" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    slab = json.loads(subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, 'tests'); import test_gpu_pseudo_surface as t; t.print_slab()"],
                                     env=env, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), capture_output=True, text=True,
                                     timeout=600).stdout.strip().splitlines()[-1])
    assert slab == 64


def print_slab():
    from gpras_amd._lib import load

    _, _, hf_proj, _, _, _ = _feature_setup(3)
    rows = C.c_int64()
    assert load().gprx_pca_slab_rows(hf_proj.handle, C.byref(rows)) == GPRX_OK
    print(rows.value)
