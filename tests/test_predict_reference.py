"""The longdouble prediction of the route tests (predict_reference.py) against mpmath at 50 digits and against the float64 oracle, and
the recorded bounds against their script and against the 1e-8 of BASELINE.  CPU only."""

import importlib.util
import os

import mpmath
import numpy as np
import pytest

import predict_reference as pr
from oracle import exact as oex

HERE = os.path.dirname(os.path.abspath(__file__))
EPS_LD = float(np.finfo(pr.LD).eps)


def _mpf(v):
    """A longdouble (or double) as an exact mpmath number: it splits into two doubles."""
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(pr.LD(v) - pr.LD(hi)))


def _g_mp(kernel, r2):
    if kernel == "RBF":
        return mpmath.exp(-r2 / 2)
    r = mpmath.sqrt(max(r2, mpmath.mpf("1e-36")))
    if kernel == "Matern12":
        return mpmath.exp(-r)
    if kernel == "Matern32":
        return (1 + mpmath.sqrt(3) * r) * mpmath.exp(-mpmath.sqrt(3) * r)
    if kernel == "Matern52":
        return (1 + mpmath.sqrt(5) * r + mpmath.mpf(5) / 3 * r * r) * mpmath.exp(-mpmath.sqrt(5) * r)
    return mpmath.exp(-r / 2)  # Exponential


def _kmat_mp(kernel, a, b, variance, ls):
    out = mpmath.matrix(a.shape[0], b.shape[0])
    for i in range(a.shape[0]):
        for j in range(b.shape[0]):
            r2 = sum(((mpmath.mpf(float(a[i, k])) - mpmath.mpf(float(b[j, k]))) / mpmath.mpf(float(ls[k]))) ** 2 for k in range(a.shape[1]))
            out[i, j] = mpmath.mpf(variance) * _g_mp(kernel, r2)
    return out


@pytest.mark.parametrize("kernel", list(pr.KERNEL_IDS))
def test_longdouble_kernel_and_prediction_against_mpmath(kernel):
    n, ns, d = 12, 3, 2
    rng = np.random.default_rng(5)
    x, xs, y = rng.standard_normal((n, d)), rng.standard_normal((ns, d)), rng.standard_normal(n)
    variance, ls, noise = 1.3, np.array([0.7, 1.4]), 0.07
    k_ld = pr.kmat_ld(kernel, x, x, variance, ls)
    mean_ld, var_ld = pr.predict_ld(kernel, x, y, variance, ls, noise, xs, True)
    _, varf_ld = pr.predict_ld(kernel, x, y, variance, ls, noise, xs, False)
    with mpmath.workdps(50):
        k_mp = _kmat_mp(kernel, x, x, variance, ls)
        # an entry of K: d differences, quotients, squares and sums, one sqrt, the polynomial, one exp whose argument (at most
        # sqrt(5) r ~ 10 here) multiplies the relative error it carries, the scaling -- 64 eps_ld covers it with room
        k_rel = max(abs(_mpf(k_ld[i, j]) - k_mp[i, j]) / k_mp[i, j] for i in range(n) for j in range(n))
        assert float(k_rel) < 64 * EPS_LD
        for i in range(n):
            k_mp[i, i] += mpmath.mpf(noise)
        ks_mp = _kmat_mp(kernel, x, xs, variance, ls)
        low = mpmath.cholesky(k_mp)
        alpha = mpmath.lu_solve(k_mp, mpmath.matrix([mpmath.mpf(float(v)) for v in y]))
        cond = float(np.linalg.cond(np.array([[float(k_mp[i, j]) for j in range(n)] for i in range(n)])))
        # K alpha = y by Cholesky: backward error c n eps_ld |K| (c a small constant) plus the 64 eps_ld of the entries themselves,
        # forward error cond(K) times that; the mean carries it through |ks_j| |alpha|, the variance through ks_j^T K^-1 ks_j <= v
        budget = (8 * n + 64) * cond * EPS_LD
        alpha_norm = mpmath.sqrt(sum(alpha[i] ** 2 for i in range(n)))
        for j in range(ns):
            ks_norm = mpmath.sqrt(sum(ks_mp[i, j] ** 2 for i in range(n)))
            mean = sum(ks_mp[i, j] * alpha[i] for i in range(n))
            assert float(abs(_mpf(mean_ld[j]) - mean)) <= budget * float(ks_norm * alpha_norm)
            col = mpmath.matrix([ks_mp[i, j] for i in range(n)])
            v = mpmath.lu_solve(low, col)  # (L v = ks_j; low is triangular, any solver at 50 digits will do)
            var_f = mpmath.mpf(variance) - sum(v[i] ** 2 for i in range(n))
            assert float(abs(_mpf(varf_ld[j]) - var_f)) <= 2 * budget * variance
            assert float(abs(_mpf(var_ld[j]) - (var_f + mpmath.mpf(noise)))) <= 2 * budget * (variance + noise)


@pytest.mark.parametrize("cid", ["S2", "S3", "S5"])
def test_longdouble_prediction_agrees_with_the_float64_oracle(cid):
    c = pr.CASES[cid]
    x, y, xs = pr.data(cid)
    v, ls, s = pr.hyper(cid)
    mean, var = pr.reference(cid)
    om, ov = oex.predict(c.kernel, x, y[:, 0], v, ls if c.ard else float(ls[0]), s, xs, True)
    assert pr.mean_err(om, mean) <= 1e-10 and pr.var_err(ov, var) <= 1e-10


def test_spelled_out_exp_and_log1p_against_mpmath():
    """exp_ld and log1p_ld use no libm; they are good to a few longdouble ulp over the ranges the kernels and softplus use."""
    xs = np.concatenate([np.linspace(-60.0, 3.0, 253), [-0.0, 1e-18, -1e-18, 0.34657359, -0.34657359]])
    zs = np.concatenate([np.linspace(0.0, 1.0, 101), [1e-30, 1e-12, 3e-5]])
    got_exp, got_log = pr.exp_ld(xs), pr.log1p_ld(zs)
    with mpmath.workdps(50):
        assert max(float(abs(_mpf(g) / mpmath.exp(mpmath.mpf(float(x))) - 1)) for g, x in zip(got_exp, xs)) < 8 * EPS_LD
        assert max(float(abs(_mpf(g) / mpmath.log1p(mpmath.mpf(float(z))) - 1)) for g, z in zip(got_log, zs) if z > 0) < 8 * EPS_LD
    assert got_log[0] == 0


def test_hyperparameters_are_the_stated_ones_on_the_theta_grid():
    """theta is the inverse softplus of what the case states, on a grid of 2^-30; softplus' slope is below 1, so what it gives back
    is the stated value to 2^-31.  The data are on their grid of 2^-20."""
    for cid, c in pr.CASES.items():
        for cell, (v, ls, s) in enumerate(c.hypers):
            gv, gls, gs = pr.hyper(cid, cell)
            assert abs(gv - v) <= 2.0 ** -30 and abs(gs - s) <= 2.0 ** -30 * s and np.all(np.abs(gls - np.atleast_1d(ls)) <= 2.0 ** -30)
            assert gls.size == (c.d if c.ard else 1)
            assert np.array_equal(pr.thetas(cid)[cell] * pr.THETA_GRID, np.rint(pr.thetas(cid)[cell] * pr.THETA_GRID))
        assert all(np.array_equal(a * pr.DATA_GRID, np.rint(a * pr.DATA_GRID)) for a in pr.data(cid))


def test_recorded_bounds_are_what_the_script_writes():
    spec = importlib.util.spec_from_file_location("make_predict_bounds", os.path.join(HERE, "golden", "make_predict_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(pr.BOUNDS_PATH) as fh:
        assert fh.read() == mod.render()


def test_every_allowed_error_stays_inside_the_baseline_tolerance():
    """8 x the recorded ratio is at most 1e-8 for every case, cell, route and quantity: the new tests ask no less than the old ones.
    A case that needs more is a badly chosen case."""
    b = pr.bounds()
    assert b and all(pr.U <= r and pr.MARGIN * r <= pr.BASELINE_TOL for r in b.values()), max(b, key=b.get)
    expected = {f"{cid}/c{cell}/{route}/{q}" for cid, c in pr.CASES.items() for cell in range(len(c.units)) for route in c.routes for q in ("mean", "var")}
    assert set(b) == expected


def test_no_reference_variance_is_a_cancelled_number():
    """min(ref var_y) >= noise in every cell, so the relative measure of the variance never divides by the remainder of a cancellation."""
    for cid, c in pr.CASES.items():
        for cell in range(len(c.units)):
            assert float(np.min(pr.reference(cid, cell)[1])) >= pr.hyper(cid, cell)[2], (cid, cell)
