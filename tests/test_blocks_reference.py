"""The longdouble references of the block tests (blocks_reference.py) against mpmath at 50 digits, and the recorded bounds against
their script.  CPU only."""

import importlib.util
import os

import mpmath
import numpy as np

import blocks_reference as br

HERE = os.path.dirname(os.path.abspath(__file__))


def _mp(a):
    return mpmath.matrix([[mpmath.mpf(float(v)) for v in row] for row in np.atleast_2d(a)])


def _worst(ref_ld, ref_mp, scale_mp):
    """max |longdouble reference - mpmath| / scale, elementwise, evaluated in mpmath (a longdouble splits exactly into two doubles)."""
    worst = mpmath.mpf(0)
    for i in range(ref_ld.shape[0]):
        for j in range(ref_ld.shape[1]):
            hi = float(ref_ld[i, j])
            lo = float(ref_ld[i, j] - br.LD(hi))
            worst = max(worst, abs(mpmath.mpf(hi) + mpmath.mpf(lo) - ref_mp[i, j]) / scale_mp[i, j])
    return float(worst)


def test_longdouble_references_against_mpmath():
    assert np.finfo(br.LD).eps < 1.1e-19
    rng = np.random.default_rng(3)
    with mpmath.workdps(50):
        # one 64 x 48 x 32 product, with the update term
        a, b, c0 = rng.standard_normal((64, 32)), rng.standard_normal((48, 32)), rng.standard_normal((64, 48))
        ref, mag = br.gemm_ref(0, 1, 0.7, a, b, -1.3, c0)
        exact = mpmath.mpf(0.7) * (_mp(a) * _mp(b).T) + mpmath.mpf(-1.3) * _mp(c0)
        # K + 2 longdouble operations per element: (K + 2) eps_ld |.| is the textbook bound, ~1e-5 of the bound the kernels are held to
        assert _worst(ref, exact, _mp(mag.astype(np.float64))) < 34 * np.finfo(br.LD).eps
        # one 128 x 128 triangular solve (the factor the solve tests use), both orientations
        low, _ = br.solve_inputs(128, br.NOISES[1])
        rhs = br.rhs(128, 4, 0)
        for transpose in (False, True):
            x = br.solve_lower_ld(low, rhs, transpose)
            lo_mp = _mp(low).T if transpose else _mp(low)
            x_mp = _mp(rhs)
            for i in (range(127, -1, -1) if transpose else range(128)):  # substitution at 50 digits
                others = range(i + 1, 128) if transpose else range(i)
                for j in range(4):
                    x_mp[i, j] = (x_mp[i, j] - mpmath.fsum(lo_mp[i, m] * x_mp[m, j] for m in others)) / lo_mp[i, i]
            # forward error of substitution: cond(L) n eps_ld at worst; cond(L) <= sqrt(n (1 + noise) / noise) = 1.2e4 for this factor
            scale = mpmath.matrix(128, 4)
            top = max(abs(x_mp[i, j]) for i in range(128) for j in range(4))
            for i in range(128):
                for j in range(4):
                    scale[i, j] = top
            assert _worst(x, x_mp, scale) < 1.2e4 * 128 * np.finfo(br.LD).eps
        # the longdouble Cholesky factor: L L^T reproduces the matrix
        k = rng.standard_normal((24, 30))
        spd = k @ k.T + np.eye(24)
        lo = br.chol_ld(spd)
        back = (lo @ lo.T).astype(np.float64)
        assert np.max(np.abs(back - spd)) <= 2 * np.finfo(np.float64).eps * np.max(np.abs(spd))


def test_spelled_out_log_against_mpmath():
    """log_ld uses no libm (the recorded log-determinant ratios must not depend on the host's): a few longdouble ulp of the value,
    absolutely below 1e-3 of it near x = 1."""
    x = np.concatenate([np.random.default_rng(0).uniform(1e-3, 5.0, 300), [1.0, 0.5, 2.0, 0.70710678, 1.41421356]])
    got = br.log_ld(x)
    assert got[300] == 0
    with mpmath.workdps(50):
        for g, v in zip(got, x):
            hi = float(g)
            exact = mpmath.log(mpmath.mpf(float(v)))
            assert abs(mpmath.mpf(hi) + mpmath.mpf(float(g - br.LD(hi))) - exact) <= 4 * float(np.finfo(br.LD).eps) * max(abs(exact), mpmath.mpf("1e-3"))


def test_recorded_bounds_are_what_the_script_writes():
    spec = importlib.util.spec_from_file_location("make_blocks_bounds", os.path.join(HERE, "golden", "make_blocks_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(br.BOUNDS_PATH) as fh:
        assert fh.read() == mod.render()


def test_recorded_factor_limits_stay_within_highams_constant():
    """What the GPU tests allow a factor, 8 x the recorded ratio, never exceeds n + 2: |A - L L^T| <= gamma_{n+1} |L| |L|^T holds for
    the Cholesky factor under ANY order of its sums (Higham, theorem 10.3), so a limit above it would allow more than rounding."""
    keys = [k for k in br.bounds() if k.startswith("potrf/")]
    assert len(keys) == len(br.SIZES) * len(br.NOISES) * len(br.SEEDS)
    for k in keys:
        n = int(k.split("/")[1][1:])
        assert 8.0 * br.bounds()[k] <= n + 2, (k, br.bounds()[k])
    # products with the explicit inverses (potrf_cell/ keys, the cell kernel's form) have no such bound: recorded, and from two block
    # columns on 8 x the ratio is beyond n + 2 on every noise-1e-6 matrix, which is why the GPU test caps that limit at n + 2
    cell = {k: v for k, v in br.bounds().items() if k.startswith("potrf_cell/")}
    assert len(cell) == len(keys) and all(v >= br.bounds()[k.replace("potrf_cell/", "potrf/")] for k, v in cell.items())
    assert all(8.0 * v > int(k.split("/")[1][1:]) + 2 for k, v in cell.items() if "/n64/" not in k and br.tag(br.NOISES[1]) in k)


def test_emulated_factorisation_against_the_longdouble_factor():
    """emu_potrf (float64, blocked) against chol_ld and the longdouble solves: the well-conditioned matrices to 1e-11, the others by
    their residuals alone (Higham's constant for the factor; the solves and inverses within the n u of their ratios)."""
    for noise in br.NOISES:
        for n in (64, 192, 320):
            a, rows = br.potrf_input(n, noise, 1), br.potrf_rhs(n, 1)[:3]
            low, inv, beta = br.emu_potrf(a, rows)
            assert np.all(np.triu(low, 1) == 0.0)
            assert br.factor_ratio(a, low) <= n + 2
            assert br.solve_ratio(low, beta.T, rows.T) <= 1.0
            assert max(br.inverse_ratio(low[i:i + 64, i:i + 64], inv[i // 64]) for i in range(0, n, 64)) <= 1.0
            if noise == br.NOISES[0]:
                ref, ref_inv = br.solve_inputs(n, noise, 1)
                assert br.rel_err(low, ref) < 1e-11 and br.rel_err(inv, ref_inv) < 1e-11
                assert br.rel_err(beta.T, br.solve_lower_ld(ref, rows.T)) < 1e-11
    # a factor with one wrong element is seen: the ratio counts roundings, and 1e-9 relative is millions of them
    low = br.emu_potrf(br.potrf_input(128, br.NOISES[0], 0))[0]
    low[100, 37] *= 1.0 + 1e-9
    assert br.factor_ratio(br.potrf_input(128, br.NOISES[0], 0), low) > 1e4


def test_exact_factor_is_reproduced_without_rounding():
    """exact_factor's matrix under two schedules with different sums -- LAPACK's and the blocked float64 emulation with explicit
    inverses: L0, the inverses of its diagonal blocks and Z come back bit for bit."""
    from scipy.linalg import cholesky, solve_triangular

    for n in (64, 192, 320, 1088):
        a, low0, inv0, y, z = br.exact_factor(n, 2)
        assert np.array_equal(np.tril(low0), low0) and np.max(np.abs(a)) < 2.0 ** 20 and np.max(np.abs(inv0)) <= 4.0
        assert set(np.unique(np.log2(np.diag(low0)))) <= {-1.0, 0.0, 1.0, 2.0}
        assert np.array_equal(a * 4.0, np.rint(a * 4.0)) and np.array_equal(y * 2.0, np.rint(y * 2.0))
        for i in range(0, n, 64):
            assert np.array_equal(inv0[i // 64] @ low0[i:i + 64, i:i + 64], np.eye(64))
        got = cholesky(a, lower=True)
        assert np.array_equal(got, low0)
        assert np.array_equal(solve_triangular(got, y.T, lower=True).T, z)
        low, inv, beta = br.emu_potrf(a, y)
        assert np.array_equal(low, low0) and np.array_equal(inv, inv0) and np.array_equal(beta, z)
    a1, a2 = br.exact_factor(128, 0)[0], br.exact_factor(128, 1)[0]
    assert not np.array_equal(a1, a2)  # (one matrix per cell)


def test_canary_is_a_nan_with_its_own_bits():
    c = br.canary((3, 2))
    assert np.all(np.isnan(c)) and np.all(br.is_canary(c))
    assert not np.any(br.is_canary(np.array([np.nan, 0.0, np.inf])))
