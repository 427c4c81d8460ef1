"""The longdouble joint prediction of the route tests (joint_reference.py) against loeo_reference.sgpr_predict_ld on the same blocks,
against mpmath at 50 digits and against the float64 mirror ensemble_numpy.joint_covariance; the case table against the branches it is
there for; the recorded bounds against their script and against the cap -- no new bound looser than the absolute 1e-8 (variance + noise)
it replaces --; and the sharpness of the measures: a result that the absolute bound accepts and these reject.  CPU only."""

import importlib.util
import os

import mpmath
import numpy as np
import pytest
from scipy.linalg import solve_triangular

import ensemble_numpy as en
import joint_reference as jr
import loeo_reference as lr
from oracle import kernels as okn
from oracle import sgpr as osg
from test_sparse_objective_reference import _g_mp, _mpf

HERE = os.path.dirname(os.path.abspath(__file__))
LD = jr.LD
EPS_LD = float(np.finfo(LD).eps)
ROWS_PER_CHUNK, DIAG_BLOCK, SPLIT_PANEL_FROM, JOINT_MAX_NS, MAX_D, MAX_MP = 256, 256, 24, 1024, 64, 320  # gp_joint.h, potrf.h, kfun.h


def _oracle_form(form):
    return "direct" if form == "difference" else "expanded"


# ---- the definition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["F-m1-ns65", "F-m65-ns130", "B-RBF-ard", "B-Matern32-iso", "B-RBF-expanded"])
def test_mean_and_diagonal_are_the_marginal_prediction(cid):
    """joint_ld's mean and the diagonal of C are loeo_reference.sgpr_predict_ld's mean and variance on the same kernel blocks -- the same
    formulas, another order of the sums: 64 longdouble ulps of the natural scale (max |mean|; S_ii)."""
    c = jr.CASES[cid]
    x, y, zs, xs = jr.data(cid)
    for cell in (0, c.cells - 1):
        v, ls, s = jr.hyper(cid, cell)
        z = zs[cell]
        kuu = jr.kmat_form_ld(c.kernel, z, z, v, ls, c.form) + LD(jr.JITTER) * np.eye(c.m, dtype=LD)
        kuf, kus = jr.kmat_form_ld(c.kernel, z, x, v, ls, c.form), jr.kmat_form_ld(c.kernel, z, xs, v, ls, c.form)
        kss_diag = np.diag(jr.kmat_form_ld(c.kernel, xs, xs, v, ls, c.form))
        for include_noise in (True, False):
            mean, var = lr.sgpr_predict_ld(kuu, kuf, y[:, jr.units(cid)[cell]], kus, v, s, include_noise)
            var = var + (kss_diag - LD(v)) + (LD(0) if include_noise else LD(jr.JITTER) * LD(v))  # (k(x, x) itself; the jitter term of the joint form)
            ref_mean, cov, _, scale = jr.joint_ld(cid, cell, include_noise)
            assert float(np.max(np.abs(mean - ref_mean))) <= 64 * EPS_LD * float(np.max(np.abs(ref_mean)))
            assert float(np.max(np.abs(var - np.diag(cov)) / np.diag(scale))) <= 64 * EPS_LD


@pytest.mark.parametrize("kernel,ard,form", [("Matern52", True, "difference"), ("RBF", False, "expanded"), ("Matern12", False, "difference")])
def test_longdouble_joint_prediction_against_mpmath(kernel, ard, form):
    """One tiny case (n = 12, m = 4, ns = 5) in mpmath at 50 digits, from the definition.  The budget: a kernel entry good to 16 eps_ld,
    two Cholesky solves with backward error 2 (n + m) eps_ld carried forward by cond(Kuu + jitter I) and cond(B) -- on the natural scale
    for the mean and for C, and carried once more by cond(C) into the factor."""
    n, m, d, ns = 12, 4, 2, 5
    rng = np.random.default_rng(17)
    x, y, xs = rng.standard_normal((n, d)), rng.standard_normal(n), rng.standard_normal((ns, d))
    z = x[[1, 4, 7, 10]] + 0.1 * rng.standard_normal((m, d))
    v, ls, s = jr.constrain(jr.theta_of(1.3, (0.7, 1.4) if ard else 0.9, 0.3))
    ls = np.broadcast_to(ls, (d,))
    parts = jr.joint_parts_ld(kernel, x, y, z, xs, v, ls, s, form)
    t = osg.common_terms(kernel, x, y, z, v, ls if ard else float(ls[0]), s, form=_oracle_form(form))
    budget = (2 * (n + m) + 16) * float(np.linalg.cond(t["Kuu"]) + np.linalg.cond(t["B"])) * EPS_LD
    assert budget < 2.0 ** -53
    with mpmath.workdps(50):
        mp = lambda a: mpmath.matrix([[mpmath.mpf(float(q)) for q in row] for row in np.atleast_2d(a)])
        lsm = [mpmath.mpf(float(q)) for q in ls]

        def r2(a, b):
            if form == "difference":
                return sum(((a[q] - b[q]) / lsm[q]) ** 2 for q in range(d))
            sa, sb = [a[q] / lsm[q] for q in range(d)], [b[q] / lsm[q] for q in range(d)]
            return (sum(q * q for q in sa) + sum(q * q for q in sb)) - 2 * sum(p * q for p, q in zip(sa, sb))

        def kmat(a, b):
            am, bm = mp(a), mp(b)
            out = mpmath.matrix(am.rows, bm.rows)
            for i in range(am.rows):
                for j in range(bm.rows):
                    out[i, j] = mpmath.mpf(v) * _g_mp(kernel, r2([am[i, q] for q in range(d)], [bm[j, q] for q in range(d)]))
            return out

        kuu = kmat(z, z) + mpmath.mpf("1e-6") * mpmath.eye(m)
        low = mpmath.cholesky(kuu)
        linv = mpmath.inverse(low)
        a = linv * kmat(z, x)
        lb = mpmath.cholesky(mpmath.eye(m) + a * a.T / mpmath.mpf(s))
        lbinv = mpmath.inverse(lb)
        cvec = lbinv * (a * mp(y).T) / mpmath.mpf(s)
        t1 = linv * kmat(z, xs)
        t2 = lbinv * t1
        mean_mp = t2.T * cvec
        base = kmat(xs, xs) - t1.T * t1 + t2.T * t2
        for include_noise in (True, False):
            mean, cov, lref, scale = jr.joint_from_parts(parts, v, s, include_noise)
            cov_mp = base + (mpmath.mpf(s) if include_noise else mpmath.mpf("1e-6") * mpmath.mpf(v)) * mpmath.eye(ns)
            lref_mp = mpmath.cholesky(cov_mp)
            cond_c = float(np.linalg.cond(cov.astype(np.float64)))
            em = max(float(abs(_mpf(mean[i]) - mean_mp[i])) for i in range(ns)) / float(np.max(np.abs(mean)))
            ec = max(float(abs(_mpf(cov[i, j]) - cov_mp[i, j])) / float(scale[i, j]) for i in range(ns) for j in range(ns))
            ef = max(float(abs(_mpf(lref[i, j]) - lref_mp[i, j])) / float(np.sqrt(cov[i, i])) for i in range(ns) for j in range(i + 1))
            print(f"{kernel} noise={include_noise}: mean {em / EPS_LD:.1f}, cov {ec / EPS_LD:.1f}, factor {ef / EPS_LD:.1f} eps_ld; budget "
                  f"{budget / EPS_LD:.0f}, cond(C) {cond_c:.1e}")
            assert em <= budget and ec <= budget and ef <= budget * cond_c


@pytest.mark.parametrize("cid,cell", [("F-m65-ns65", 1), ("B-Matern32-ard", 2), ("B-RBF-expanded", 0), ("R-RBF-ns257", 0), ("C24", 13)])
def test_longdouble_joint_prediction_against_the_float64_mirror(cid, cell):
    """ensemble_numpy.joint_covariance (LAPACK, BLAS, libm: the reference of test_gpu_ensemble.py) on one case of each group: every entry of
    C within 1e-10 of its natural scale, the mean within 1e-10 of its largest entry."""
    c = jr.CASES[cid]
    x, y, zs, xs = jr.data(cid)
    v, ls, s = jr.hyper(cid, cell)
    for include_noise in (True, False):
        mean, cov = en.joint_covariance(c.kernel, x, y[:, jr.units(cid)[cell]], zs[cell], v, ls if c.ard else float(ls[0]), s, xs, include_noise,
                                        form=_oracle_form(c.form))
        ref_mean, ref_cov, _, scale = jr.joint_ld(cid, cell, include_noise)
        assert jr.mean_err(mean, ref_mean) <= 1e-10
        assert float(np.max(np.abs(cov.astype(LD) - ref_cov) / scale)) <= 1e-10
        assert np.all(np.abs(ref_cov) <= scale)  # (the triangle inequality)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def test_cases_are_on_their_grids_and_reach_what_they_claim():
    for cid, c in jr.CASES.items():
        x, y, zs, xs = jr.data(cid)
        assert x.shape == (jr.N_TRAIN, c.d) and y.shape == (jr.N_TRAIN, jr.N_UNITS) and zs.shape == (c.cells, c.m, c.d) and xs.shape == (c.ns, c.d)
        assert all(np.array_equal(a * jr.DATA_GRID, np.rint(a * jr.DATA_GRID)) for a in (x, y, zs, xs))
        th = jr.thetas(cid)
        assert th.shape == (c.cells, c.nlen + 2) and np.array_equal(th * jr.pr.THETA_GRID, np.rint(th * jr.pr.THETA_GRID))
        assert len({tuple(t) for t in th}) == c.cells
        for cell in range(c.cells):
            assert len({tuple(r) for r in zs[cell]}) == c.m and not np.all(zs[cell][:, None, :] == x[None, :, :], axis=2).any()
        assert c.d <= MAX_D and c.mp <= MAX_MP and 1 <= c.ns <= JOINT_MAX_NS
    factors, build, rows = ([jr.CASES[i] for i in jr.GROUPS[g]] for g in ("factors", "build", "rows"))
    assert {c.m for c in factors} == {1, 50, 64, 65, 192, 300, 320} and {c.ns for c in factors} == {65, 130}
    assert {c.mp for c in factors} == {64, 128, 192, 320} and {-(-c.mp // ROWS_PER_CHUNK) for c in factors} == {1, 2}
    assert all((c.kernel, c.d, c.cells) == ("Matern52", 3, 3) for c in factors)
    assert {(c.kernel, c.cls) for c in build if c.d == 3} == {(k, cls) for k in jr.KERNELS for cls in jr.CLASSES}
    assert all((c.m, c.ns) == (50, 65) for c in build if c.d == 3)
    assert {(c.d, c.ard, c.form, c.ns) for c in build if c.d > 3} == {(17, True, "difference", 257), (64, True, "difference", 130), (64, False, "expanded", 130)}
    assert {(c.kernel, c.ns) for c in rows} == {(k, ns) for k in ("RBF", "Matern32") for ns in (1, 64, 65, 256, 257, 300, 1024)}
    assert all(c.cells == (2 if c.ns == JOINT_MAX_NS else 3) and c.m == 50 for c in rows)
    assert {c.ns <= DIAG_BLOCK for c in rows} == {False, True} and max(c.tp for c in rows) == JOINT_MAX_NS
    c24 = jr.CASES["C24"]
    assert c24.cells == SPLIT_PANEL_FROM and c24.tp == 320 and len({tuple(t) for t in jr.thetas("C24")}) == 24
    assert len(set(zip(jr.units("C24").tolist(), (np.arange(24) // 3).tolist()))) == 24
    assert all(jr.CASES[i].m <= 64 for i in jr.UNFUSED) and [jr.CASES[i].tp for i in jr.ROUTE_CASES] == [320, 1024]


# ---- the recorded bounds --------------------------------------------------------------------------------------------------------------
def _generator():
    spec = importlib.util.spec_from_file_location("make_joint_bounds", os.path.join(HERE, "golden", "make_joint_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_case_cell_and_quantity_has_a_recorded_bound():
    b = jr.bounds()
    assert set(b) == jr.expected_keys()
    assert all(jr.U <= r < 1e-6 for r in b.values()), max(b, key=b.get)
    assert os.path.getsize(jr.BOUNDS_PATH) < 2 ** 20
    with open(jr.BOUNDS_PATH) as fh:
        assert fh.read() == _generator().render(b)  # (the script's layout)


@pytest.mark.parametrize("cid", ["F-m1-ns65", "B-RBF-iso"])
def test_recomputing_a_case_reproduces_the_recorded_numbers(cid):
    got = jr.case_ratios(cid)
    assert got == {k: jr.bounds()[k] for k in got}


def _scale64_max(cid, cell, include_noise):
    """max_ij S_ij in float64 (LAPACK, BLAS, the oracle's kernels): a sum of magnitudes, good to 1e-9 of itself."""
    c = jr.CASES[cid]
    x, y, zs, xs = jr.data(cid)
    v, ls, s = jr.hyper(cid, cell)
    ls_arg, form = (ls if c.ard else float(ls[0])), _oracle_form(c.form)
    t = osg.common_terms(c.kernel, x, y[:, jr.units(cid)[cell]], zs[cell], v, ls_arg, s, form=form)
    t1 = np.abs(solve_triangular(t["L"], okn.kmat(c.kernel, zs[cell], xs, v, ls_arg, form), lower=True))
    t2 = np.abs(solve_triangular(t["LB"], solve_triangular(t["L"], okn.kmat(c.kernel, zs[cell], xs, v, ls_arg, form), lower=True), lower=True))
    scale = np.abs(okn.kmat(c.kernel, xs, xs, v, ls_arg, form)) + t1.T @ t1 + t2.T @ t2
    return float(np.max(scale + (s if include_noise else jr.JITTER * v) * np.eye(c.ns)))


def test_no_recorded_bound_is_looser_than_the_absolute_bound_it_replaces():
    """The cap of make_joint_bounds.py on the file as committed: 8 x recorded cov ratio x S_ij <= 1e-8 (variance + noise) for every
    element of every case, cell and include_noise (S in float64 here, checked against the longdouble one on a case)."""
    assert _scale64_max("F-m50-ns65", 1, True) == pytest.approx(float(np.max(jr.joint_ld("F-m50-ns65", 1, True)[3])), rel=1e-9)
    worst = (0.0, None)
    for cid, c in jr.CASES.items():
        for cell in range(c.cells):
            v, _, s = jr.hyper(cid, cell)
            for nz in (0, 1):
                used = jr.MARGIN * jr.recorded(cid, cell, nz, "cov") * _scale64_max(cid, cell, nz) * (1 + 1e-9) / (jr.BASELINE_TOL * (v + s))
                worst = max(worst, (used, jr.key(cid, cell, nz, "cov")))
    print(f"the loosest new bound is {worst[0]:.3e} of 1e-8 (variance + noise), at {worst[1]}")
    assert worst[0] <= 1.0, worst


# ---- sharpness ------------------------------------------------------------------------------------------------------------------------
def test_the_measures_reject_what_the_absolute_bound_accepts():
    """Three wrong results built from the restatement's own, each accepted by max |Lc Lc^T - C| <= 1e-8 (variance + noise) against the
    float64 mirror and rejected here: a relative error of 1e-9 in one covariance entry (carried by a rescaled row of the factor), one
    small entry of Lc off by 1e-9 of its row's norm, and a mean off by 1e-10 of its largest entry."""
    cid, cell = "F-m50-ns65", 0
    c = jr.CASES[cid]
    x, y, zs, xs = jr.data(cid)
    v, ls, s = jr.hyper(cid, cell)
    _, mirror = en.joint_covariance(c.kernel, x, y[:, 0], zs[cell], v, float(ls[0]), s, xs, True)
    old_accepts = lambda lc: np.max(np.abs(lc @ lc.T - mirror)) <= 1e-8 * (v + s)

    def new_accepts(mean, lc):
        return all(val <= jr.MARGIN * jr.recorded(cid, cell, 1, q) for q, val in jr.errors(mean, lc, cid, cell, 1).items())

    mean, lc = jr.emu_joint(cid, cell, 1)
    assert old_accepts(lc) and new_accepts(mean, lc)
    row = lc.copy()
    row[40] *= 1.0 + 1e-9
    entry = lc.copy()
    i, j = 50, int(np.argmin(np.abs(lc[50, :50])))
    entry[i, j] += 1e-9 * np.linalg.norm(lc[i])
    for wrong in (row, entry):
        assert old_accepts(wrong) and not new_accepts(mean, wrong)
    assert not new_accepts(mean + 1e-10 * np.max(np.abs(mean)), lc)
