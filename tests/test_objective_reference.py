"""The longdouble objective of the route tests (objective_reference.py) against mpmath at 50 digits, against central differences of its
own loss and against the float64 oracle, and the recorded bounds against their script.  CPU only."""

import importlib.util
import os

import mpmath
import numpy as np
import pytest

import objective_reference as orf
from oracle import exact as oex
from oracle import kernels as okn

HERE = os.path.dirname(os.path.abspath(__file__))
LD = orf.LD
EPS_LD = float(np.finfo(LD).eps)
ORACLE_FACTOR = orf.MARGIN  # the oracle gets what the device gets: LAPACK's and BLAS's summation orders, libm's exp and log


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


def _objective_mp(kernel, x, y, mask, ard):
    """u = (variance, lengthscales..., noise) -> LML + log prior of the trained parameters, in mpmath: K entry by entry from the
    definition (max(r2, 1e-36) included, which is what stops the gradient at coincident inputs), Cholesky, log det, the quadratic form."""
    n, d = x.shape
    nlen = d if ard else 1
    on = orf.trained(mask, nlen)
    xm = [[mpmath.mpf(float(v)) for v in row] for row in x]
    ym = mpmath.matrix([mpmath.mpf(float(v)) for v in y])

    def f(*u):
        v, ls, s = u[0], [u[1 + (k if ard else 0)] for k in range(d)], u[-1]
        k = mpmath.matrix(n, n)
        for i in range(n):
            for j in range(n):
                k[i, j] = v * _g_mp(kernel, sum(((xm[i][q] - xm[j][q]) / ls[q]) ** 2 for q in range(d)))
            k[i, i] += s
        low = mpmath.cholesky(k)
        beta = mpmath.lu_solve(low, ym)  # (L beta = y; low is triangular, any solver at this precision will do)
        lml = -sum(b * b for b in beta) / 2 - sum(mpmath.log(low[i, i]) for i in range(n)) - mpmath.mpf(n) / 2 * mpmath.log(2 * mpmath.pi)
        return lml + sum(_ln_logpdf_mp(u[q]) for q in np.flatnonzero(on))

    return f


MP_CASES = [(k, ard, False) for k in orf.KERNEL_IDS for ard in (False, True)] + [("Matern12", False, True), ("Matern32", True, True)]


@pytest.mark.parametrize("kernel,ard,coincident", MP_CASES)
def test_longdouble_objective_against_mpmath(kernel, ard, coincident):
    """Loss and every gradient component of objective_ld against mpmath: the loss from the definition, the gradient as mpmath's own
    numerical derivative of that loss in the constrained parameters (no derivative formula is restated) times the sigmoid.  The budget:
    an entry of K good to 16 eps_ld (two differences, quotients, squares, a sum, one sqrt, the polynomial, an exp whose argument of at
    most 5 multiplies the error it carries), a Cholesky solve with backward error 2 n eps_ld, both carried forward by cond(K) (about 25
    here) -- 1e-16 on the natural scale of each number, below the unit roundoff of the results this reference will judge."""
    n, d = 12, 2
    rng = np.random.default_rng(7)
    x, y = rng.standard_normal((n, d)), rng.standard_normal(n)
    if coincident:
        x[5] = x[2]
    theta = orf.theta_of(1.3, (0.7, 1.4) if ard else 0.9, 0.3)
    mask = orf.ALL
    loss, grad, loss_scale, grad_scale = orf.objective_ld(kernel, x, y, theta, mask, ard)
    u = orf.constrained(theta)
    v, ls, s = orf.constrain(theta)
    kmat = okn.kmat(kernel, x, x, v, ls if ard else float(ls[0])) + s * np.eye(n)
    budget = (2 * n + 16) * float(np.linalg.cond(kmat)) * EPS_LD
    assert budget < 2.0 ** -53
    with mpmath.workdps(50):
        f = _objective_mp(kernel, x, y, mask, ard)
        um = [mpmath.mpf(float(q)) for q in u]
        print(f"loss {float(abs(_mpf(loss) + f(*um))) / float(loss_scale) / EPS_LD:.1f} eps_ld, budget {budget / EPS_LD:.0f}")
        assert float(abs(_mpf(loss) + f(*um))) <= budget * float(loss_scale)
        for k in range(len(um)):
            dk = mpmath.diff(f, tuple(um), tuple(int(q == k) for q in range(len(um))))
            w = mpmath.mpf(float(theta[k]))
            ref = -dk / (1 + mpmath.exp(-w))
            print(f"g{k} {float(abs(_mpf(grad[k]) - ref)) / float(grad_scale[k]) / EPS_LD:.1f} eps_ld")
            assert float(abs(_mpf(grad[k]) - ref)) <= budget * float(grad_scale[k]), (k, float(grad[k]), float(ref))


@pytest.mark.parametrize("cid", ["K-Matern52", "N40", "C-Matern12", "C-Matern32", "X-Matern52"])
def test_longdouble_gradient_against_central_differences_of_its_own_loss(cid):
    """On cases of the GPU tests (coincident inputs and the expanded form among them): central differences of the longdouble loss in each
    unconstrained parameter, step t = 1e-7, the constrained values NOT rounded to double in between.  Truncation t^2 / 6 |f'''| with
    |f'''| taken as 64 x (natural scale of the component + that of the loss); cancellation 2 x 256 eps_ld x the loss's scale / (2 t),
    the loss being a sum of a few hundred terms."""
    c = orf.CASES[cid]
    x, y = orf.data(cid)
    theta = orf.thetas(cid)[0].astype(LD)
    _, grad, loss_scale, grad_scale = orf.reference(cid)

    def loss_at(th):
        u = orf.softplus_ld(th)
        u[-1] = LD(orf.NOISE_LOWER) + u[-1]
        raw = orf.raw_ld(c.kernel, x, y[:, 0], u[0], np.broadcast_to(u[1:-1], (c.d,)), u[-1], c.ard, c.form)
        return orf.finish(raw, th, orf.ALL, u=u)[0]

    t = LD(1e-7)
    for k in range(theta.size):
        e = np.zeros(theta.size, LD)
        e[k] = t
        cd = (loss_at(theta + e) - loss_at(theta - e)) / (2 * t)
        tol = float(t * t) / 6 * 64 * float(grad_scale[k] + loss_scale) + 256 * EPS_LD * float(loss_scale) / float(t)
        assert float(abs(cd - grad[k])) <= tol, (k, float(cd), float(grad[k]), tol)


@pytest.mark.parametrize("cid", ["K-Matern12", "A9", "X-RBF"])
def test_natural_scales_against_the_oracle_kernels(cid):
    """S_k -- the denominator of every gradient comparison -- from oracle/kernels.py's g and h in float64 and numpy's sums; and
    |g_k| <= S_k, |loss| <= its scale (the triangle inequality)."""
    c = orf.CASES[cid]
    x, y = orf.data(cid)
    v, ls, s = orf.hyper(cid)
    theta = orf.thetas(cid)[0]
    raw = orf.reference_raw(cid)
    loss, grad, loss_scale, grad_scale = orf.reference(cid)
    assert abs(loss) <= loss_scale and np.all(np.abs(grad) <= grad_scale)
    low, alpha = oex.factorize(c.kernel, x, y[:, 0], v, ls, s, "direct" if c.form == "difference" else "expanded")
    linv = np.linalg.inv(low)
    aw = np.abs(np.outer(alpha, alpha) - linv.T @ linv)
    r2 = okn.scaled_sqdist(x, x, ls, "direct" if c.form == "difference" else "expanded")
    g, h = okn.g_of_r2(c.kernel, r2), okn.h_of_r2(c.kernel, r2)
    s_ls = np.array([0.5 * np.sum(aw * np.abs(v * h) * (x[:, k][:, None] - x[:, k][None, :]) ** 2) / ls[k] ** 3 for k in range(c.d)])
    su = np.concatenate([[0.5 * np.sum(aw * np.abs(g))], s_ls if c.ard else [s_ls.sum()], [0.5 * np.trace(aw)]])
    np.testing.assert_allclose(raw.du_scale.astype(np.float64), su, rtol=1e-9)
    u = orf.constrained(theta)
    sig = 1.0 / (1.0 + np.exp(-theta))
    np.testing.assert_allclose(grad_scale.astype(np.float64), (su + np.abs((1.0 + np.log(u)) / u)) * sig, rtol=1e-9)


@pytest.mark.parametrize("cid", [c.id for c in orf.SINGLE + orf.STATE])
def test_float64_oracle_lands_within_the_recorded_bounds(cid):
    """oracle/exact.py's loss_and_grad -- the reference of the rest of the suite -- on every single case, within ORACLE_FACTOR x the
    recorded ratio (the larger of the two routes) of objective_ld, component by component."""
    c = orf.CASES[cid]
    x, y = orf.data(cid)
    th = orf.thetas(cid)[0]
    loss, grad = oex.loss_and_grad(c.kernel, x, y[:, 0], th[0], th[1:-1] if c.ard else float(th[1]), th[-1],
                                   form="direct" if c.form == "difference" else "expanded")
    grad = np.concatenate([[grad["variance"]], np.atleast_1d(grad["lengthscales"]), [grad["noise"]]])
    el, eg = orf.errors(loss, grad, orf.reference(cid))
    allowed = lambda q: ORACLE_FACTOR * max(orf.recorded(cid, 0, route, orf.ALL, q) for route in orf.ROUTES)
    print(f"{cid}: loss {el / allowed('loss') * ORACLE_FACTOR:.2f} x ratio, gradient "
          + " ".join(f"{e / allowed(f'g{k}') * ORACLE_FACTOR:.2f}" for k, e in enumerate(eg)))
    assert el <= allowed("loss")
    for k, e in enumerate(eg):
        assert e <= allowed(f"g{k}"), (k, e, allowed(f"g{k}"))


def test_spelled_out_sigmoid_and_prior_against_mpmath():
    ws = np.array([-14.0, -3.0, -0.5, 0.0, 0.7, 5.0])
    us = np.array([2e-6, 0.05, 1.0, 1.3, 11.0])
    with mpmath.workdps(50):
        for w, got in zip(ws, orf.sigmoid_ld(ws)):
            assert float(abs(_mpf(got) * (1 + mpmath.exp(-mpmath.mpf(float(w)))) - 1)) < 8 * EPS_LD
        for u, lp, dlp in zip(us, orf.ln_logpdf_ld(us), orf.ln_dlogpdf_ld(us)):
            um = mpmath.mpf(float(u))
            assert float(abs(_mpf(lp) - _ln_logpdf_mp(um))) < 8 * EPS_LD * float(abs(_ln_logpdf_mp(um)) + 1)
            assert float(abs(_mpf(dlp) - mpmath.diff(_ln_logpdf_mp, um))) < 8 * EPS_LD * float((1 + abs(mpmath.log(um))) / um)


def test_cases_are_on_their_grids_and_hold_what_they_claim():
    for cid, c in orf.CASES.items():
        x, y = orf.data(cid)
        assert x.shape == (c.n, c.d) and y.shape == (c.n, c.n_units) and len(c.units) == len(c.hypers) and max(c.units) < c.n_units
        assert all(np.array_equal(a * orf.DATA_GRID, np.rint(a * orf.DATA_GRID)) for a in (x, y))
        th = orf.thetas(cid)
        assert th.shape == (len(c.units), (c.d if c.ard else 1) + 2) and np.array_equal(th * pr_grid(), np.rint(th * pr_grid()))
        for cell, (v, ls, s) in enumerate(c.hypers):
            gv, gls, gs = orf.hyper(cid, cell)
            assert abs(gv - v) <= 2.0 ** -30 and abs(gs - s) <= 2.0 ** -30 * s and np.all(np.abs(gls - np.broadcast_to(ls, (c.d,))) <= 2.0 ** -30)
    same = lambda cid: np.sum(np.all(orf.data(cid)[0][:, None, :] == orf.data(cid)[0][None, :, :], axis=2)) - orf.CASES[cid].n
    assert same("C-Matern12") == 96 and same("C-Exponential") == 96 and same("C-Matern32") == 2 and same("K-Matern12") == 0
    assert max(-(-c.n // 64) * 64 for c in orf.CASES.values()) == 448


def pr_grid():
    return orf.pr.THETA_GRID


def test_recorded_bounds_are_what_the_script_writes():
    spec = importlib.util.spec_from_file_location("make_objective_bounds", os.path.join(HERE, "golden", "make_objective_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(orf.BOUNDS_PATH) as fh:
        assert fh.read() == mod.render()


def test_every_case_route_and_component_has_a_recorded_bound():
    b = orf.bounds()
    assert set(b) == orf.expected_keys()
    assert all(orf.U <= r < 1e-6 for r in b.values()), max(b, key=b.get)


def test_recorded_ratio_follows_the_condition_of_k():
    """H-2 and H-6 differ in the noise alone (1e-2, 2e-6): the recorded ratios of the loss and of the noise component grow with 1 / s."""
    for q in ("loss", "g2"):
        lo, hi = (orf.recorded(cid, 0, "from_inverse", orf.ALL, q) for cid in ("H-2", "H-6"))
        assert hi > 100 * lo, (q, lo, hi)
