"""CPU pins of the peak ensemble's numpy mirror (ensemble_numpy.py) and of the host-side argument checks of gpras_amd.ensemble: the joint
covariance against the terms of ``oracle/sgpr.py``, the exact fused multiply-add against rational arithmetic, the chain against
``sweep_numpy``'s restatement of the reference, the statistics against numpy's own reductions, ``joint_applies`` and every argument check."""

from fractions import Fraction

import numpy as np
import pytest
from scipy.linalg import solve_triangular

import ensemble_numpy as en
import sweep_numpy as sn
from gpras_amd import ensemble as ge
from gpras_amd.synth import make_regression
from oracle import kernels as okn
from oracle import sgpr as osg


@pytest.mark.parametrize("kernel", ["RBF", "Matern32"])
@pytest.mark.parametrize("include_noise", [True, False])
def test_joint_covariance_against_the_oracle_terms(kernel, include_noise):
    n, d, m, ns = 120, 3, 15, 23
    x, y, xs = make_regression(n, d, n_outputs=1, n_test=ns, config=4)
    z = np.ascontiguousarray(x[:m] + 1e-3)
    variance, ls, noise = 1.1, 0.9, 0.07
    mean, cov = en.joint_covariance(kernel, x, y[:, 0], z, variance, ls, noise, xs, include_noise)
    t = osg.common_terms(kernel, x, y[:, 0], z, variance, ls, noise)
    kus = okn.kmat(kernel, z, xs, variance, ls)
    tmp1 = solve_triangular(t["L"], kus, lower=True)
    tmp2 = solve_triangular(t["LB"], tmp1, lower=True)
    want = okn.kmat(kernel, xs, xs, variance, ls) - tmp1.T @ tmp1 + tmp2.T @ tmp2
    want = want + (noise if include_noise else osg.JITTER * variance) * np.eye(ns)
    assert np.array_equal(cov, want)
    ref_mean, ref_var = osg.predict(kernel, x, y[:, 0], z, variance, ls, noise, xs, include_noise)
    assert np.array_equal(mean, ref_mean)
    extra = 0.0 if include_noise else osg.JITTER * variance
    np.testing.assert_allclose(np.diag(cov), ref_var + extra, rtol=1e-12)
    # the padded factor: the leading block factors C, the padding is the identity
    lc = en.padded_cholesky(cov, 64)
    np.testing.assert_allclose(lc[:ns, :ns] @ lc[:ns, :ns].T, cov, rtol=0, atol=1e-13 * (variance + noise))
    assert np.array_equal(lc[ns:, ns:], np.eye(64 - ns)) and not np.any(lc[ns:, :ns]) and not np.any(lc[:ns, ns:])


def test_pack_scores():
    rng = np.random.default_rng(0)
    k, s, rows, tp = 2, 3, 5, 64
    mean, zn = rng.normal(size=(k, rows)), rng.normal(size=(k, s, tp))
    lc = np.stack([en.padded_cholesky(np.eye(rows) + 0.5, tp) for _ in range(k)])
    got = en.pack_scores(mean, lc, zn, rows)
    assert got.shape == (s, rows, k)
    for kk in range(k):
        np.testing.assert_allclose(got[:, :, kk], mean[kk][None, :] + zn[kk, :, :rows] @ lc[kk, :rows, :rows].T, rtol=1e-14)
    assert np.array_equal(en.pack_scores(mean, lc, np.zeros_like(zn), rows), np.broadcast_to(mean.T[None], (s, rows, k)))


def _exact_fma(a, b, c):
    """round(a b + c) from rational arithmetic: the nearest double, ties to even (``float(Fraction)`` rounds correctly)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def test_fma_is_exact():
    rng = np.random.default_rng(1)
    a, b = rng.normal(size=400), rng.normal(size=400)
    c = rng.normal(size=400)
    c[:100] = -(a[:100] * b[:100])  # cancellation: the result is the product's rounding error
    c[100:200] *= 1e-17  # the addend below the product's last bit
    c[200:250] = 0.0
    a[250:260] = 0.0
    # halfway cases: 1 + 2^-53 (1 + tiny) must round up, 1 + 2^-53 (1 - tiny) down
    a[300:302], b[300:302], c[300:302] = 2.0**-53, [1.0 + 2.0**-30, 1.0 - 2.0**-30], 1.0
    got = en.fma(a, b, c)
    want = np.array([_exact_fma(*t) for t in zip(a.tolist(), b.tolist(), c.tolist())])
    assert np.array_equal(got, want)
    assert got[300] == 1.0 + 2.0**-52 and got[301] == 1.0


@pytest.mark.parametrize("hp", ["wse", "depth", "velocity"])
def test_member_chain_against_the_reference_restatement(hp):
    """The device's operation order (fma chain, divide, add) against numpy's ``dot`` chain of ``sweep_numpy``: equal to rounding, the dry
    cells and the clamp exactly."""
    k, rows, members = 7, 9, 3
    state, *_ = sn.make_case(40, k, [rows], hp, weighted=True, dry=(3, 17), seed=5)
    scores = np.random.default_rng(2).normal(size=(members, rows, k))
    y = en.member_fields(state, scores)
    for s in range(members):
        _, want, _ = sn.metric_fields(state, k, scores[s], None, np.zeros((rows, 40)))
        np.testing.assert_allclose(y[s], want, rtol=1e-12, atol=1e-13)
        if hp != "velocity":
            assert np.all(y[s] >= 0.0)
    peak = en.member_peaks(state, scores)
    assert np.array_equal(peak, y.max(axis=1))
    assert np.array_equal(peak[:, 3], np.zeros(members) if hp != "velocity" else np.full(members, state["elevations"][3]))


def test_statistics_against_numpy():
    members, cells = 17, 30
    rng = np.random.default_rng(3)
    peak = rng.uniform(0.0, 1.0, size=(members, cells))
    peak[:, 0] = 0.5
    peak[::2, 1] = 0.5
    peak[:, 2] = np.repeat(rng.uniform(size=6), 3)[:members]
    quantiles = (0.0, 0.25, 0.5, 1.0)  # q (S - 1) = 0, 4, 8, 16 exactly
    ranks = en.quantile_ranks(quantiles, members)
    assert ranks.tolist() == [0, 4, 8, 16] and np.array_equal(ranks, ge.quantile_ranks(quantiles, members))
    areas = rng.uniform(1.0, 5.0, size=cells)
    st = en.member_stats(peak, (0.5, 0.25), ranks, areas)
    assert np.array_equal(st["order"], np.sort(peak, axis=0)[ranks])
    assert np.array_equal(st["order"], np.quantile(peak, quantiles, axis=0, method="lower"))
    assert np.array_equal(st["exceed"][0], (peak > 0.5).sum(axis=0)) and st["exceed"][0, 0] == 0 and st["exceed"].dtype == np.int32
    np.testing.assert_allclose(st["mean"], np.mean(peak, axis=0), rtol=1e-14)
    np.testing.assert_allclose(st["std"], np.std(peak, axis=0), rtol=1e-13)
    assert st["std"][0] == 0.0
    np.testing.assert_allclose(st["wet_area"][:, 1], ((peak > 0.25) * areas).sum(axis=1), rtol=1e-14)
    assert np.array_equal(en.member_stats(peak, (0.5,), ranks)["wet_area"][:, 0], (peak > 0.5).sum(axis=1).astype(np.float64))


def test_joint_applies():
    assert ge.joint_applies(50, 8, 100) is None and ge.joint_applies(320, 64, 1024) is None
    assert "exact model" in ge.joint_applies(None, 8, 100)
    assert "320" in ge.joint_applies(321, 8, 100)
    assert "64" in ge.joint_applies(50, 65, 100)
    assert "1024" in ge.joint_applies(50, 8, 1025)
    assert ge.joint_applies(50, 8, 0)


def test_argument_checks():
    assert ge.padded_rows(1) == 64 and ge.padded_rows(64) == 64 and ge.padded_rows(65) == 128
    thr, rk = ge.check_stats_args(17, (0.5, 1.0), [0, 16])
    assert thr.dtype == np.float64 and rk.dtype == np.int32 and rk.tolist() == [0, 16]
    for members, thresholds, ranks in ((0, (), ()), (4097, (), ()), (4, np.arange(9.0), ()), (4, (), np.arange(9) % 4), (4, (), [4]), (4, (), [-1]),
                                       (4, [np.nan], ()), (4, (), [0.5])):
        with pytest.raises(ValueError):
            ge.check_stats_args(members, thresholds, ranks)
    for q in ([-0.1], [1.1], [np.nan]):
        with pytest.raises(ValueError):
            ge.quantile_ranks(q, 8)
    lo, hi = ge.check_event_ranges([(0, 3), (3, 7), (8, 10)], 10)
    assert lo.tolist() == [0, 3, 8] and hi.tolist() == [3, 7, 10]
    for bad in ([(3, 7), (0, 3)], [(0, 5), (4, 8)], [(0, 0)], [(0, 11)], [(-1, 2)], []):
        with pytest.raises(ValueError):
            ge.check_event_ranges(bad, 10)
    with pytest.raises(ValueError):
        ge.PeakEnsemble(object(), object())  # not a fitted model
