"""The longdouble sparse objective of the route tests (sparse_objective_reference.py) against mpmath at 50 digits, against central
differences of its own loss and against a float64 evaluation with the oracle's kernels; the recorded bounds against their script and
against the float64 oracle; the case table against the branches it is there for; and the sharpness of the measure: results that the
block-maximum measure of the other sparse suites accepts and this one rejects.  CPU only."""

import importlib.util
import os

import mpmath
import numpy as np
import pytest

import sparse_objective_reference as sr
from oracle import kernels as okn
from oracle import sgpr as osg

HERE = os.path.dirname(os.path.abspath(__file__))
LD = sr.LD
EPS_LD = float(np.finfo(LD).eps)
NB, B_FINISH_MP, SPLITK_CHUNK, KM_DC, DZ_DC, MAX_D, SPLIT_PANEL_FROM = 64, 128, 256, 8, 16, 64, 24  # gp_sparse.h, kmat.h, grad.h, kfun.h, potrf.h
WELL_CONDITIONED = 1e6  # cond(Kuu + jitter I) up to which the other sparse suites hold a case to 1e-7 of the block maximum


def _mpf(v):
    """A longdouble (or double) as an exact mpmath number: it splits into two doubles."""
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(LD(v) - LD(hi)))


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


def _ln_logpdf_mp(u):
    return -mpmath.log(u) - mpmath.log(2 * mpmath.pi) / 2 - mpmath.log(u) ** 2 / 2


def _oracle_form(form):
    return "direct" if form == "difference" else "expanded"


def _bound_mp(kernel, x, y, m, ard, form):
    """(variance, lengthscales..., noise, z_00, z_01, ...) -> ELBO + log prior of the hyperparameters, in mpmath, from the DEFINITION of
    the bound: log N(y | 0, Qff + s I) - (n v - tr Qff) / (2 s) with Qff = Kuf^T (Kuu + jitter I)^-1 Kuf -- an n x n Cholesky
    factorisation and none of the M x M algebra the reference and the device share."""
    n, d = x.shape
    nlen = d if ard else 1
    xm = [[mpmath.mpf(float(v)) for v in row] for row in x]
    ym = mpmath.matrix([mpmath.mpf(float(v)) for v in y])

    def r2(a, b, ls):
        if form == "difference":
            return sum(((a[q] - b[q]) / ls[q]) ** 2 for q in range(d))
        sa, sb = [a[q] / ls[q] for q in range(d)], [b[q] / ls[q] for q in range(d)]
        return (sum(t * t for t in sa) + sum(t * t for t in sb)) - 2 * sum(p * q for p, q in zip(sa, sb))

    def f(*u):
        v, ls, s = u[0], [u[1 + (k if ard else 0)] for k in range(d)], u[1 + nlen]
        z = [[u[2 + nlen + i * d + q] for q in range(d)] for i in range(m)]
        kuu, kuf = mpmath.matrix(m, m), mpmath.matrix(m, n)
        for i in range(m):
            for j in range(m):
                kuu[i, j] = v * _g_mp(kernel, r2(z[i], z[j], ls))
            kuu[i, i] += mpmath.mpf("1e-6")
            for j in range(n):
                kuf[i, j] = v * _g_mp(kernel, r2(z[i], xm[j], ls))
        qff = kuf.T * mpmath.inverse(kuu) * kuf
        cov = qff + s * mpmath.eye(n)
        lc = mpmath.cholesky(cov)
        beta = mpmath.lu_solve(lc, ym)
        bound = (-sum(b * b for b in beta) / 2 - sum(mpmath.log(lc[i, i]) for i in range(n)) - mpmath.mpf(n) / 2 * mpmath.log(2 * mpmath.pi)
                 - (n * v - sum(qff[i, i] for i in range(n))) / (2 * s))
        return bound + sum(_ln_logpdf_mp(u[q]) for q in range(2 + nlen))

    return f


MP_CASES = [(k, ard, "difference") for k in sr.KERNELS for ard in (False, True)] + [("Matern52", True, "expanded")]


@pytest.mark.parametrize("kernel,ard,form", MP_CASES)
def test_longdouble_objective_against_mpmath(kernel, ard, form):
    """Loss and every gradient component of sparse_objective_ld -- the entries of Z included -- against mpmath: the loss from the
    definition of the bound, the gradient as mpmath's own numerical derivative of that loss (no derivative formula is restated) times
    the sigmoid.  The budget: a kernel entry good to 16 eps_ld, two Cholesky solves with backward error 2 (n + m) eps_ld, the first
    carried forward by cond(Kuu + jitter I), the second by cond(B); the two add up, they do not multiply: the bound depends on A' through
    A'^T (I + A' A'^T / s)^-1 A' and log det(I + A' A'^T / s) alone, whose sensitivity to a relative change of A' is at most 2."""
    n, m, d = 12, 4, 2
    rng = np.random.default_rng(11)
    x, y = rng.standard_normal((n, d)), rng.standard_normal(n)
    z = x[[1, 4, 7, 10]] + 0.1 * rng.standard_normal((m, d))
    theta = sr.theta_of(1.3, (0.7, 1.4) if ard else 0.9, 0.3)
    loss, grad, gz, loss_scale, grad_scale, gz_scale = sr.sparse_objective_ld(kernel, x, y, z, theta, sr.ALL, ard, form)
    u = sr.orf.constrained(theta)
    v, ls, s = sr.constrain(theta)
    ls_arg = ls if ard else float(ls[0])
    kuu = okn.kmat(kernel, z, z, v, ls_arg, _oracle_form(form)) + sr.JITTER * np.eye(m)
    t = osg.common_terms(kernel, x, y, z, v, ls_arg, s, form=_oracle_form(form))
    budget = (2 * (n + m) + 16) * float(np.linalg.cond(kuu) + np.linalg.cond(t["B"])) * EPS_LD
    assert budget < 2.0 ** -53
    with mpmath.workdps(50):
        f = _bound_mp(kernel, x, y, m, ard, form)
        um = [mpmath.mpf(float(q)) for q in u] + [mpmath.mpf(float(q)) for q in z.ravel()]
        print(f"loss {float(abs(_mpf(loss) + f(*um))) / float(loss_scale) / EPS_LD:.1f} eps_ld, budget {budget / EPS_LD:.0f}")
        assert float(abs(_mpf(loss) + f(*um))) <= budget * float(loss_scale)
        for k in range(len(um)):
            dk = mpmath.diff(f, tuple(um), tuple(int(q == k) for q in range(len(um))))
            if k < len(u):
                ref, got, scale = -dk / (1 + mpmath.exp(-mpmath.mpf(float(theta[k])))), grad[k], grad_scale[k]
            else:
                ref, got, scale = -dk, gz.ravel()[k - len(u)], gz_scale.ravel()[k - len(u)]
            print(f"component {k}: {float(abs(_mpf(got) - ref)) / float(scale) / EPS_LD:.1f} eps_ld")
            assert float(abs(_mpf(got) - ref)) <= budget * float(scale), (k, float(got), float(ref))


CD_CASES = ("F-RBF-iso", "Z-Matern32", "F-Matern52-ard")
CD_ENTRIES = 40


@pytest.mark.parametrize("cid", CD_CASES)
def test_longdouble_gradient_against_central_differences_of_its_own_loss(cid):
    """On cases of the GPU tests (coincident inducing points and ARD among them): central differences of the longdouble loss in every
    unconstrained hyperparameter and in 40 entries of Z (evenly spread, the one of the smallest natural scale among them), step
    t = 1e-6, the constrained values NOT rounded to double in between.  Truncation t^2 / 6 |f'''| with |f'''| taken as 64 x (natural scale
    of the component + that of the loss); cancellation 2 x 256 eps_ld x the loss's scale / (2 t), the loss being a sum of a few hundred
    terms."""
    c = sr.CASES[cid]
    x, y, z = sr.model(cid, 0)
    theta = sr.thetas(cid)[0].astype(LD)
    _, grad, gz, loss_scale, grad_scale, gz_scale = sr.reference(cid)

    def loss_at(th, zz):
        u = sr.pr.softplus_ld(th)
        u[-1] = LD(sr.pr.NOISE_LOWER) + u[-1]
        raw = sr.raw_ld(c.kernel, x, y, zz, u[0], np.broadcast_to(u[1:-1], (c.d,)), u[-1], c.ard, c.form)
        return sr.finish(raw, th, sr.ALL, u=u)[0]

    t = LD(1e-6)
    tol = lambda scale: float(t * t) / 6 * 64 * float(scale + loss_scale) + 256 * EPS_LD * float(loss_scale) / float(t)
    zl = z.astype(LD)
    for k in range(theta.size):
        e = np.zeros(theta.size, LD)
        e[k] = t
        cd = (loss_at(theta + e, zl) - loss_at(theta - e, zl)) / (2 * t)
        assert float(abs(cd - grad[k])) <= tol(grad_scale[k]), (k, float(cd), float(grad[k]), tol(grad_scale[k]))
    flat = sorted(set(np.linspace(0, z.size - 1, CD_ENTRIES - 1).astype(int).tolist()) | {int(np.argmin(gz_scale))})
    for idx in flat:
        i, k = divmod(idx, c.d)
        e = np.zeros(z.shape, LD)
        e[i, k] = t
        cd = (loss_at(theta, zl + e) - loss_at(theta, zl - e)) / (2 * t)
        assert float(abs(cd - gz[i, k])) <= tol(gz_scale[i, k]), (i, k, float(cd), float(gz[i, k]), tol(gz_scale[i, k]))


def _scales64(cid, cell=0):
    """The natural scales of the module's docstring in float64: numpy's BLAS and sums, the oracle's kernels, g and h."""
    c = sr.CASES[cid]
    x, y, z = sr.model(cid, cell)
    v, ls, s = sr.hyper(cid, cell)
    form = _oracle_form(c.form)
    n, m = x.shape[0], c.m
    t = osg.common_terms(c.kernel, x, y, z, v, ls, s, form=form)
    p, q, low, a, lb, cvec = t["Kuf"], t["Kuu"], t["L"], t["A"], t["LB"], t["c"]
    linv = np.linalg.inv(low)
    qinv = linv.T @ linv
    r = np.linalg.inv(lb) @ linv
    sinv = r.T @ r
    mvec = linv.T @ np.linalg.solve(lb.T, cvec)
    g_q = 0.5 * (qinv - sinv) - (qinv @ p) @ (qinv @ p).T / (2 * s) - 0.5 * np.outer(mvec, mvec)
    g_p = ((qinv - sinv - np.outer(mvec, mvec)) @ p + np.outer(mvec, y)) / s
    r2p, r2q = okn.scaled_sqdist(z, x, ls, form), okn.scaled_sqdist(z, z, ls, form)
    ghp, ghq = np.abs(g_p * v * okn.h_of_r2(c.kernel, r2p)), g_q * v * okn.h_of_r2(c.kernel, r2q)
    ghqs, ghq = np.abs(ghq + ghq.T), np.abs(ghq)
    resid = y - p.T @ mvec
    loss_scale = (0.5 * n * np.log(2 * np.pi) + np.sum(np.abs(np.log(np.diag(lb)))) + 0.5 * n * abs(np.log(s)) + 0.5 * (n * v / s + np.sum(a * a))
                  + 0.5 * (y @ y / s + cvec @ cvec))
    s_var = n / (2 * s) + np.sum(np.abs(g_p * p)) / v + np.sum(np.abs(g_q * (q - sr.JITTER * np.eye(m)))) / v
    s_noise = (abs(s * (m - np.sum(np.linalg.inv(lb) ** 2))) + s * np.sum(a * a) + resid @ resid + n * v) / (2 * s * s) + n / (2 * s)
    s_ls, s_z = np.zeros(c.d), np.zeros((m, c.d))
    for k in range(c.d):
        dp, dq = z[:, k][:, None] - x[:, k][None, :], z[:, k][:, None] - z[:, k][None, :]
        s_ls[k] = (np.sum(ghp * dp * dp) + np.sum(ghq * dq * dq)) / ls[k] ** 3
        s_z[:, k] = (np.sum(ghp * np.abs(dp), axis=1) + np.sum(ghqs * np.abs(dq), axis=1)) / ls[k] ** 2
    return loss_scale, np.concatenate([[s_var], s_ls if c.ard else [s_ls.sum()], [s_noise]]), s_z


@pytest.mark.parametrize("cid", ["F-Matern12-iso", "F-RBF-expanded", "G-Matern52-ard", "H-fused"])
def test_natural_scales_against_the_oracle_kernels(cid):
    """The denominators of every comparison from oracle/kernels.py's g and h in float64 and numpy's sums (N < M, the expanded form,
    M > 64, held-out rows); and |value| <= its scale (the triangle inequality)."""
    cell = sr.CASES[cid].cells - 1
    raw = sr.reference_raw(cid, cell)
    loss, grad, gz, loss_scale, grad_scale, gz_scale = sr.reference(cid, cell)
    assert abs(loss) <= loss_scale and np.all(np.abs(grad) <= grad_scale) and np.all(np.abs(gz) <= gz_scale)
    want_loss, want_u, want_z = _scales64(cid, cell)
    np.testing.assert_allclose(raw.du_scale.astype(np.float64), want_u, rtol=1e-9)
    np.testing.assert_allclose(gz_scale.astype(np.float64), want_z, rtol=1e-9)
    theta = sr.thetas(cid)[cell]
    u = sr.orf.constrained(theta)
    np.testing.assert_allclose(float(loss_scale), want_loss + np.sum(np.abs(sr.orf.ln_logpdf_ld(u).astype(np.float64))), rtol=1e-12)
    np.testing.assert_allclose(grad_scale.astype(np.float64), (want_u + np.abs((1.0 + np.log(u)) / u)) / (1.0 + np.exp(-theta)), rtol=1e-9)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _mp(m):
    return NB * ((m + NB - 1) // NB)


def test_cases_are_on_their_grids_and_hold_what_they_claim():
    for cid, c in sr.CASES.items():
        x, y, zs = sr.data(cid)
        assert x.shape == (c.n, c.d) and y.shape == (c.n, sr.N_UNITS) and zs.shape == (c.cells, c.m, c.d)
        assert all(np.array_equal(a * sr.DATA_GRID, np.rint(a * sr.DATA_GRID)) for a in (x, y, zs))
        th = sr.thetas(cid)
        assert th.shape == (c.cells, c.nlen + 2) and np.array_equal(th * sr.pr.THETA_GRID, np.rint(th * sr.pr.THETA_GRID))
        assert len({tuple(t) for t in th}) == c.cells and (c.cells == 1 or len(set(sr.units(cid).tolist())) > 1)
        on_rows = np.all(zs[:, :, None, :] == x[None, None, :, :], axis=3).any(axis=2)  # (cells, m): the point IS a training row
        assert np.array_equal(on_rows, np.broadcast_to(np.arange(c.m) % 2 == 0, on_rows.shape) if c.coincident else np.zeros_like(on_rows)), cid
        for cell in range(c.cells):
            assert len({tuple(r) for r in zs[cell]}) == c.m  # (no two inducing points of a cell coincide)
        assert len(c.holds) in (0, c.cells)
    # a middle range across the 256-column chunk edge, a prefix, a suffix, a single row, nothing
    assert sr.HOLDS[0][0] == 0 and sr.HOLDS[1][1] == 600 and sr.HOLDS[2][0] < SPLITK_CHUNK < sr.HOLDS[2][1]
    assert sr.HOLDS[3][1] - sr.HOLDS[3][0] == 1 and sr.HOLDS[4][0] == sr.HOLDS[4][1]
    assert sr.kept("H-fused", 2).size == 500 and sr.kept("H-fused", 4).size == 600


def test_case_table_reaches_every_axis_value_and_route():
    """Every axis value the routes are there for.  Fused: 15 (kernel, class) pairs, NP in {6, 8, 0} against every kernel and every class,
    the listed d, M and N.  General: 15 pairs, both sides of B_FINISH_MP, mp above 256, N = 70 < M = 100, split-K, both sides of KM_DC and
    of the 16-dimension chunks of the Z-gradient kernel.  Then the ill-conditioned pair, 24 cells, d = 70, the masks, the held rows and
    the coincident points.  It fails when a case is removed."""
    fused, general = [sr.CASES[i] for i in sr.FUSED], [sr.CASES[i] for i in sr.GENERAL]
    pairs = {(k, cls) for k in sr.KERNELS for cls in sr.CLASSES}
    for group in (fused, general):
        assert len(group) == 15 and {(c.kernel, c.cls) for c in group} == pairs
        assert {(c.kernel, c.ard) for c in group if c.form == "expanded"} == {(k, k not in sr.EXPANDED_ISO) for k in sr.KERNELS}
    assert {(c.kernel, sr.np_of(c.d)) for c in fused} == {(k, p) for k in sr.KERNELS for p in (6, 8, 0)}
    assert {(c.cls, sr.np_of(c.d)) for c in fused} == {(cls, p) for cls in sr.CLASSES for p in (6, 8, 0)}
    assert {c.d for c in fused} == {1, 5, 12, 13, 16, 17, 33, 64}
    assert {c.m for c in fused} == {1, 17, 50, 63, 64}
    assert {c.n for c in fused} == {40, 255, 257, 513} and all(c.m == 50 for c in fused if c.n == 40)
    assert all(c.cells == 3 for c in fused)
    assert {c.m for c in general} == {65, 100, 128, 129, 192, 300, 320}
    assert {_mp(c.m) for c in general} == {128, 192, 320} and {_mp(c.m) <= B_FINISH_MP for c in general} == {False, True}
    assert {c.n for c in general} == {70, 257, 961, 1025} and all(c.m == 100 for c in general if c.n == 70)
    assert {_mp(c.n) >= 4 * SPLITK_CHUNK for c in general} == {False, True} and _mp(1025) > _mp(961) == 4 * SPLITK_CHUNK
    assert {c.d for c in general} == {1, 8, 9, 16, 17, 64}
    assert {c.d > KM_DC for c in general} == {False, True} and {(c.d + DZ_DC - 1) // DZ_DC for c in general} == {1, 2, 4}
    assert all(c.cells >= 2 for c in general)
    ill = [sr.CASES[i] for i in sr.ILL]
    assert [(c.kernel, c.d, c.m) for c in ill] == [("RBF", 3, 64), ("Matern52", 3, 130)]
    assert all(1e7 <= sr.condition(c.id) <= 1e8 for c in ill)
    c24, wide = sr.CASES["C24"], sr.CASES["D70"]
    assert c24.cells == SPLIT_PANEL_FROM and (c24.m, c24.n) == (65, 257)
    assert wide.d == 70 > MAX_D and wide.ard and wide.cells == 3
    assert set(sr.MASKS) == {15, 8, 7, 1, 2, 4}
    assert [sr.CASES[i].group for i in sr.MASK_CASES] == ["fused", "general"] and all(sr.CASES[i].masks == sr.MASKS for i in sr.MASK_CASES)
    held = [sr.CASES[i] for i in sr.ROUTES["held"]]
    assert [c.m <= NB for c in held] == [True, False] and all(c.holds == sr.HOLDS and c.d <= MAX_D for c in held)
    assert [sr.CASES[i].kernel for i in sr.COINCIDENT] == list(sr.KERNELS)
    assert all(sr.CASES[i].form == "difference" and sr.CASES[i].coincident and sr.CASES[i].m <= NB for i in sr.COINCIDENT)
    assert len(sr.UNFUSED) == 3 and set(sr.UNFUSED) <= set(sr.FUSED)
    # the routes of the GPU file: every one is there, and together they evaluate every case
    assert set(sr.ROUTES) == {"fused_lone", "fused_batch", "sequence_small", "sequence_general", "cells24", "wide", "masks", "held", "coincident"}
    assert {cid for cases in sr.ROUTES.values() for cid in cases} == set(sr.CASES)


# ---- the recorded bounds --------------------------------------------------------------------------------------------------------------
def test_recorded_bounds_are_what_the_script_writes():
    spec = importlib.util.spec_from_file_location("make_sparse_objective_bounds", os.path.join(HERE, "golden", "make_sparse_objective_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(sr.BOUNDS_PATH) as fh:
        assert fh.read() == mod.render()
    assert os.path.getsize(sr.BOUNDS_PATH) < 2 ** 20


def test_every_case_cell_mask_and_quantity_has_a_recorded_bound():
    """The file holds exactly the expected keys -- and with them everything test_gpu_sparse_objective_routes.py asks for: every route's
    cases, every cell, the case's masks, the loss, each trained hyperparameter component and gz."""
    b = sr.bounds()
    assert set(b) == sr.expected_keys()
    for cases in sr.ROUTES.values():
        for cid in cases:
            c = sr.CASES[cid]
            for cell in range(c.cells):
                for mask in c.masks:
                    assert all(sr.recorded(cid, cell, mask, q) >= sr.U for q in sr.quantities(cid, mask))
    assert all(sr.U <= r < 1e-5 for r in b.values()), max(b, key=b.get)


def _oracle(cid, cell, mask=sr.ALL):
    """(loss, grad, gz) of oracle.sgpr.loss_and_grad -- the reference of the other sparse suites."""
    c = sr.CASES[cid]
    x, y, z = sr.model(cid, cell)
    th = sr.thetas(cid)[cell]
    flags = tuple(bool(mask & b) for b in (1, 2, 4, 8))
    loss, g = osg.loss_and_grad(c.kernel, x, y, z, float(th[0]), th[1:-1] if c.ard else float(th[1]), float(th[-1]), flags, form=_oracle_form(c.form))
    return loss, np.concatenate([[g["variance"]], np.atleast_1d(g["lengthscales"]), [g["noise"]]]), np.asarray(g["Z"])


@pytest.mark.parametrize("cid", sr.FUSED + sr.GENERAL + ("C24", "D70", "H-fused", "H-general"))
def test_float64_oracle_lands_within_the_recorded_bounds(cid):
    """oracle/sgpr.py's loss_and_grad (LAPACK's and BLAS's summation orders, libm's exp and log: it gets what the device gets, MARGIN) on
    every cell of the well-conditioned cases, quantity by quantity, Z entry by entry."""
    c = sr.CASES[cid]
    for cell in range(c.cells):
        if sr.condition(cid, cell) > WELL_CONDITIONED:
            continue
        got = sr.ratios(*_oracle(cid, cell), cid, cell, sr.ALL)
        used = {q: val / sr.recorded(cid, cell, sr.ALL, q) for q, val in got.items()}
        worst = max(used, key=used.get)
        print(f"{cid}/c{cell}: worst {worst} at {used[worst]:.2f} x recorded")
        assert used[worst] <= sr.MARGIN, (cell, worst, got[worst], sr.recorded(cid, cell, sr.ALL, worst))


def test_well_conditioned_covers_the_table():
    """(what the test above skips: the ill-conditioned pair by design, and no more than a few cells of the table besides)"""
    cells = [(cid, cell) for cid in sr.FUSED + sr.GENERAL for cell in range(sr.CASES[cid].cells)]
    over = [k for k in cells if sr.condition(*k) > WELL_CONDITIONED]
    assert len(over) <= 3, over


def test_recorded_ratio_follows_the_condition_of_kuu():
    """Across the cells of the smooth kernels (RBF, Matern32, Matern52) the recorded ratios grow with cond(Kuu + jitter I): the median of
    gz and of the worst hyperparameter component over the cells with cond >= 1e4 is more than five times that over the cells with
    cond < 1e3, and each cell of the ill-conditioned pair (cond 1e7 .. 1e8) lies above EVERY cell with cond < 1e3."""
    cells = [(cid, cell) for cid in sr.FUSED + sr.GENERAL + sr.ILL for cell in range(sr.CASES[cid].cells)
             if sr.CASES[cid].kernel in ("RBF", "Matern32", "Matern52") and sr.CASES[cid].m > 1]
    cond = np.array([sr.condition(*k) for k in cells])
    worst_g = lambda cid, cell: max(sr.recorded(cid, cell, sr.ALL, q) for q in sr.quantities(cid, sr.ALL) if q not in ("loss", "gz"))
    for name, rec in (("gz", lambda cid, cell: sr.recorded(cid, cell, sr.ALL, "gz")), ("g", worst_g)):
        val = np.array([rec(*k) for k in cells])
        easy, hard = val[cond < 1e3], val[cond >= 1e4]
        print(f"{name}: {easy.size} cells below 1e3, median {np.median(easy):.2e}; {hard.size} cells from 1e4, median {np.median(hard):.2e}")
        assert easy.size >= 10 and hard.size >= 5
        assert np.median(hard) > 5 * np.median(easy), name
        for cid in sr.ILL:
            assert rec(cid, 0) > np.max(easy), (name, cid)


# ---- sharpness ------------------------------------------------------------------------------------------------------------------------
def _old_measure_accepts(loss, grad, gz, ref):
    """The measure of test_gpu_sparse_variants.py / test_gpu_sparse_general.py against the float64 oracle: the loss within 1e-9, each
    gradient block within 1e-7 of the block's largest entry."""
    ref_loss, ref_grad, ref_gz = ref
    return (abs(loss - ref_loss) <= 1e-9 * abs(ref_loss) and np.max(np.abs(grad - ref_grad)) <= 1e-7 * np.max(np.abs(ref_grad))
            and np.max(np.abs(gz - ref_gz)) <= 1e-7 * np.max(np.abs(ref_gz)))


def _new_measure_accepts(loss, grad, gz, cid, cell):
    got = sr.ratios(loss, grad, gz, cid, cell, sr.ALL)
    return all(val <= sr.MARGIN * sr.recorded(cid, cell, sr.ALL, q) for q, val in got.items())


SLOPPY_EXP = 1e-11   # relative error of every Kuf entry
SMALL_ENTRY = 1e-6   # relative error of the one Z entry of the smallest natural scale: wrong in its sixth digit


@pytest.mark.parametrize("cid", ["F-Matern52-ard", "G-RBF-ard"])  # an ARD fused shape, an M > 64 shape
def test_the_own_scale_measure_rejects_what_the_block_maximum_measure_accepts(cid, monkeypatch):
    """Two wrong results built from the float64 oracle's own: (a) every entry of Kuf carries a relative error of 1e-11 -- an exponential a
    few terms short --, (b) the one Z entry of the smallest natural scale is off by 1e-6 of itself.  The old measure (loss 1e-9, blocks
    1e-7 of the block maximum, against the oracle) accepts both, as it accepts the honest result; the new one accepts the honest result
    and rejects both.  Both sides are asserted here, so the two sizes are no tolerances anyone has to trust."""
    cell = 0
    honest = _oracle(cid, cell)
    assert _old_measure_accepts(*honest, honest) and _new_measure_accepts(*honest, cid, cell)
    # (a) a sloppy exponential in Kuf
    kmat, n = okn.kmat, sr.CASES[cid].n
    rng = np.random.default_rng(5)

    def sloppy(kernel, a, b, *args, **kw):
        k = kmat(kernel, a, b, *args, **kw)
        return k * (1.0 + SLOPPY_EXP * rng.uniform(-1.0, 1.0, k.shape)) if k.shape[1] == n else k

    monkeypatch.setattr(osg.kn, "kmat", sloppy)
    wrong = _oracle(cid, cell)
    monkeypatch.undo()
    assert not np.array_equal(wrong[2], honest[2])
    assert _old_measure_accepts(*wrong, honest)
    assert not _new_measure_accepts(*wrong, cid, cell)
    # (b) one small Z entry wrong in its sixth digit
    _, _, ref_gz, _, _, gz_scale = sr.reference(cid, cell)
    idx = np.unravel_index(np.argmin(gz_scale), gz_scale.shape)
    gz = honest[2].copy()
    gz[idx] *= 1.0 + SMALL_ENTRY
    assert _old_measure_accepts(honest[0], honest[1], gz, honest)
    assert not _new_measure_accepts(honest[0], honest[1], gz, cid, cell)
