"""Plain-numpy references for the objective-route tests (test_gpu_objective_routes.py): no GPU is imported here.

The reference of one evaluation of the exact model is objective_ld: K + s I, its Cholesky factor, alpha by two solves, K^-1 from the
inverse of the factor, loss = -(LML + log prior of the trained parameters) and the gradient in the unconstrained parameters,
g_k = 1/2 sum_ij W_ij dK_ij/dtheta_k with W = alpha alpha^T - K^-1, all in np.longdouble with no BLAS and no libm in between
(blocks_reference.py: chol_ld, solve_lower_ld, inv_lower_ld, log_ld; predict_reference.py: exp_ld, log1p_ld).  The kernel derivative
is that of csrc/kfun.h, h = 2 dg/dr2 with h = 0 where r2 < 1e-36 (coincident inputs); transforms and priors are those of csrc/gp_ctx.h
and oracle/transforms.py.  test_objective_reference.py checks it against mpmath at 50 digits and against its own central differences.

Every error is measured against the NATURAL SCALE of the number it belongs to, component by component:
  loss      |loss - ref| / (1/2 y^T K^-1 y + sum |log L_ii| + n/2 log 2 pi + sum |log prior|)
  gradient  |g_k - ref_k| / S_k,  S_k = (1/2 sum_ij |W_ij| |dK_ij/du_k| + |d log prior/du_k|) |du_k/dw_k|
so a wrong small ARD component cannot hide behind a large one, and one wrongly weighted element of the trace shows at its own size.

emu_objective restates the device route (csrc/gp_exact.h, grad.h, solve.h) in float64 on 64-wide blocks: emu_chol, beta, alpha by
emu_trsv ("substitution") or as X^T beta from X = emu_trtri ("from_inverse"), K^-1 = X^T X summed in k order, the trace per 64 x 64
tile on or below the diagonal with the off-diagonal weights doubled, tile partials added in tile order; the isotropic difference form
sums wh r2 / l, every other form sums per dimension.  Kernel entries are the longdouble kernel rounded to double under the perturbations
the device's kernel build is allowed (predict_reference.kmat64).  tests/golden/make_objective_bounds.py records how far it lands from
objective_ld (the maximum over the unperturbed run and three perturbation seeds, never below u); the GPU tests allow 8 x that.

The expanded distance form (gprx_set_distance_form) changes r2 inside g and h only; the factors ds_k of the derivatives stay differences
(grad.h).  The reference evaluates the expanded r2 in longdouble, the emulation in float64 as kmat.h states it: x / l, squares rounded
and summed in k order, the dot product in k order, (na + nb) - 2 dot.
"""

from __future__ import annotations

import functools
import json
import os
from typing import NamedTuple

import numpy as np

import predict_reference as pr
from blocks_reference import LD, NB, U, chol_ld, dot64, emu_trsv, emu_trtri, inv_lower_ld, log_ld, solve_lower_ld, sum64
from gpras_amd.synth import make_regression
from predict_reference import (DATA_GRID, KERNEL_IDS, MARGIN, NOISE_LOWER, PERTURB_SEEDS, R2_FLOOR, constrain, emu_chol, exp_ld, g_ld, kmat64, r2_ld,
                               softplus_ld, theta_of)

BOUNDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "objective_bounds.json")
ROUTES = ("substitution", "from_inverse")  # how alpha is formed
TRAIN_VARIANCE, TRAIN_LENGTHSCALE, TRAIN_NOISE = 1, 2, 4
ALL = 7
PI_LD = LD("3.14159265358979323846264338327950288")
LOG_2PI_LD = log_ld(LD(2) * PI_LD)
LOG_2PI = float(LOG_2PI_LD)
canary, is_canary = pr.canary, pr.is_canary


# ---- kernel, distance forms, derivative factor -------------------------------------------------------------------------------------
def scaled_diff_ld(x, k, ls):
    col = np.asarray(x)[:, k].astype(LD) / LD(ls[k])
    return col[:, None] - col[None, :]


def r2_form_ld(x, ls, form):
    """Scaled squared distances of x against itself in the handle's distance form, longdouble."""
    if form == "difference":
        return r2_ld(x, x, ls)
    sa = np.asarray(x).astype(LD) / np.asarray(ls).astype(LD)[None, :]
    na, dot = np.zeros(sa.shape[0], LD), np.zeros((sa.shape[0],) * 2, LD)
    for k in range(sa.shape[1]):
        na = na + sa[:, k] * sa[:, k]
        dot = dot + sa[:, k][:, None] * sa[:, k][None, :]
    return (na[:, None] + na[None, :]) - LD(2) * dot


def h_ld(kernel, r2):
    """h = 2 dg/d(r2) (csrc/kfun.h corr_gh): zero where max(r2, 1e-36) stops the gradient."""
    if kernel == "RBF":
        return -exp_ld(LD(-0.5) * r2)
    live = r2 >= R2_FLOOR
    r = np.sqrt(np.maximum(r2, R2_FLOOR))
    sqrt3, sqrt5 = np.sqrt(LD(3)), np.sqrt(LD(5))
    if kernel == "Matern12":
        h = -exp_ld(-r) / r
    elif kernel == "Matern32":
        h = LD(-3) * exp_ld(-sqrt3 * r)
    elif kernel == "Matern52":
        h = -(LD(5) / LD(3)) * (LD(1) + sqrt5 * r) * exp_ld(-sqrt5 * r)
    elif kernel == "Exponential":
        h = LD(-0.5) * exp_ld(LD(-0.5) * r) / r
    else:
        raise KeyError(kernel)
    return np.where(live, h, LD(0))


# ---- transforms and priors ------------------------------------------------------------------------------------------------------------
def sigmoid_ld(w):
    w = np.asarray(w).astype(LD)
    e = exp_ld(-np.abs(w))
    return np.where(w >= 0, LD(1) / (LD(1) + e), e / (LD(1) + e))


def ln_logpdf_ld(u):
    lu = log_ld(np.asarray(u).astype(LD))
    return -lu - LD(0.5) * LOG_2PI_LD - LD(0.5) * lu * lu


def ln_dlogpdf_ld(u):
    u = np.asarray(u).astype(LD)
    return -(LD(1) + log_ld(u)) / u


def trained(mask, nlen):
    """Which of (variance, lengthscales..., noise) the mask trains."""
    return np.array([bool(mask & TRAIN_VARIANCE)] + [bool(mask & TRAIN_LENGTHSCALE)] * nlen + [bool(mask & TRAIN_NOISE)])


class Raw(NamedTuple):
    """What an evaluation gives before priors and the chain rule: the LML, its derivatives in the constrained parameters
    (variance, lengthscales..., noise), and -- the reference only -- the sums of magnitudes behind both."""
    lml: object
    du: np.ndarray
    lml_scale: object = None
    du_scale: np.ndarray = None


def constrained(theta) -> np.ndarray:
    """(variance, lengthscales..., noise) as the library works with them: the longdouble softplus rounded to double
    (predict_reference.constrain)."""
    u = softplus_ld(theta).astype(np.float64)
    u[-1] = NOISE_LOWER + u[-1]
    return u


def finish(raw: Raw, theta, mask, dtype=LD, u=None):
    """(loss, grad, loss_scale, grad_scale) in the unconstrained parameters: loss = -(LML + log prior of the trained parameters),
    grad_k = -(dLML/du_k + dlogp/du_k) sigmoid(w_k) for a trained parameter and exactly 0 otherwise.  dtype = float64 restates the host
    code of gp_ctx.h (chain_rule, log_prior) on doubles; the scales are returned for the reference only.  u: the constrained values
    `raw` was evaluated at (default: constrained(theta))."""
    theta = np.asarray(theta)
    nlen = theta.size - 2
    u = constrained(theta) if u is None else u
    on = trained(mask, nlen)
    logp, dlogp, sig = ln_logpdf_ld(u).astype(dtype), ln_dlogpdf_ld(u).astype(dtype), sigmoid_ld(theta).astype(dtype)
    lp = dtype(0)
    for k in np.flatnonzero(on):
        lp = lp + logp[k]
    loss = -(dtype(raw.lml) + lp)
    grad = np.where(on, -(np.asarray(raw.du).astype(dtype) + dlogp) * sig, dtype(0))
    if raw.lml_scale is None:
        return loss, grad, None, None
    loss_scale = raw.lml_scale + np.sum(np.abs(logp[on]))
    grad_scale = np.where(on, (raw.du_scale + np.abs(dlogp)) * sig, LD(0))
    return loss, grad, loss_scale, grad_scale


# ---- the longdouble reference -------------------------------------------------------------------------------------------------------
def raw_ld(kernel, x, y, variance, ls, noise, ard, form="difference") -> Raw:
    """LML, dLML/d(variance, lengthscales, noise) and their natural scales, longdouble.  ls: d lengthscales (all equal unless ard)."""
    x, y = np.asarray(x), np.asarray(y).astype(LD)
    n, d = x.shape
    ls = np.broadcast_to(np.asarray(ls).astype(LD), (d,))
    v = LD(variance)
    r2 = r2_form_ld(x, ls, form)
    g, h = g_ld(kernel, r2), h_ld(kernel, r2)
    k = v * g
    k[np.diag_indices(n)] += LD(noise)
    low = chol_ld(k)
    beta = solve_lower_ld(low, y)
    alpha = solve_lower_ld(low, beta, transpose=True)
    xinv = inv_lower_ld(low)
    kinv = np.zeros((n, n), LD)
    for i in range(n):  # K^-1 = X^T X, X lower triangular
        kinv += xinv[i][:, None] * xinv[i][None, :]
    w = alpha[:, None] * alpha[None, :] - kinv
    aw = np.abs(w)
    logs = log_ld(np.diag(low))
    quad = LD(0.5) * np.sum(beta * beta)
    lml = -quad - np.sum(logs) - LD(0.5) * n * LOG_2PI_LD
    lml_scale = quad + np.sum(np.abs(logs)) + LD(0.5) * n * LOG_2PI_LD
    vh = v * h
    dls, sls = np.zeros(d, LD), np.zeros(d, LD)
    for kk in range(d):
        ds = scaled_diff_ld(x, kk, ls)
        dk = -vh * ds * ds / LD(ls[kk])
        dls[kk], sls[kk] = LD(0.5) * np.sum(w * dk), LD(0.5) * np.sum(aw * np.abs(dk))
    if not ard:
        dls, sls = np.array([np.sum(dls)]), np.array([np.sum(sls)])
    du = np.concatenate([[LD(0.5) * np.sum(w * g)], dls, [LD(0.5) * np.sum(np.diag(w))]])
    su = np.concatenate([[LD(0.5) * np.sum(aw * np.abs(g))], sls, [LD(0.5) * np.sum(np.diag(aw))]])
    return Raw(lml, du, lml_scale, su)


def objective_ld(kernel, x, y, theta, mask=ALL, ard=False, form="difference"):
    """(loss, grad, loss_scale, grad_scale) of one model at the unconstrained theta = (variance, lengthscales..., noise), longdouble."""
    v, ls, s = constrain(theta)
    return finish(raw_ld(kernel, x, y, v, ls, s, ard, form), theta, mask)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    """One data set (n, d, n_units outputs, seeded through make_regression) and the cells evaluated on it."""
    id: str
    kernel: str
    ard: bool
    n: int
    d: int
    units: tuple           # unit of each cell
    hypers: tuple          # (variance, lengthscale(s), noise) of each cell, constrained
    seed: int
    n_units: int = 2
    duplicates: str = ""   # "alternate": rows 1::2 are copies of rows 0::2; "pair": one row is a copy of another
    form: str = "difference"
    masks: tuple = (ALL,)


def _single(cid, kernel, ard, n, d, variance, ls, noise, seed, **kw):
    return Case(cid, kernel, ard, n, d, (0,), ((variance, ls, noise),), seed, **kw)


def _ls(lo, hi, d):
    return tuple(np.linspace(lo, hi, d))


SINGLE = (
    *(_single(f"K-{k}", k, False, 65, 3, 1.3, 1.2, 0.05, seed=1) for k in KERNEL_IDS),
    _single("N64", "RBF", False, 64, 1, 1.0, 0.8, 0.1, seed=2),            # np = n, one panel
    _single("N40", "Matern52", False, 40, 2, 0.9, 1.1, 0.03, seed=3),      # less than one tile
    _single("A9", "Matern32", True, 130, 9, 1.2, _ls(2.0, 4.0, 9), 0.04, seed=4, masks=tuple(range(8))),  # np = 192: odd recursion, pass 2 re-staged
    _single("A17", "RBF", True, 200, 17, 1.1, _ls(3.0, 6.0, 17), 0.02, seed=5),
    _single("D70", "Matern12", False, 130, 70, 1.0, 8.0, 0.05, seed=6),    # d > 64
    _single("D66", "Exponential", True, 100, 66, 1.2, _ls(6.0, 10.0, 66), 0.05, seed=7),
    _single("N385", "RBF", False, 385, 4, 1.5, 1.6, 0.02, seed=8),         # np = 448: HEAD / TAIL at outer_block = 128, ragged last block
    # hard conditioning: the lengthscale about twice the spread of the data (unit standard deviation per coordinate, points within +-2)
    _single("H-2", "RBF", False, 192, 2, 1.0, 4.0, 1e-2, seed=9),
    _single("H-6", "RBF", False, 192, 2, 1.0, 4.0, 2e-6, seed=9),
    # coincident inputs off the diagonal
    _single("C-Matern12", "Matern12", False, 96, 2, 1.0, 0.9, 0.05, seed=10, duplicates="alternate"),
    _single("C-Exponential", "Exponential", False, 96, 2, 1.0, 0.9, 0.05, seed=10, duplicates="alternate"),
    _single("C-Matern32", "Matern32", False, 96, 2, 1.0, 0.9, 0.05, seed=10, duplicates="pair"),
    # the expanded distance form
    _single("X-RBF", "RBF", False, 130, 5, 1.2, 2.0, 0.05, seed=11, form="expanded"),
    _single("X-Matern52", "Matern52", True, 130, 5, 1.2, _ls(1.5, 3.0, 5), 0.05, seed=11, form="expanded"),
)
# the state test: D70's data under another hyperparameter vector
STATE = (_single("D70b", "Matern12", False, 130, 70, 1.4, 11.0, 0.02, seed=6),)
B26_CELLS = 26
BATCH = (
    Case("B3", "Matern52", False, 130, 3, (2, 0, 2), tuple((1.0 + 0.3 * c, 0.9 + 0.25 * c, 0.03 * (c + 1)) for c in range(3)), seed=21, n_units=3),
    Case("B26", "RBF", False, 70, 3, tuple(c % 3 for c in range(B26_CELLS)),
         tuple((1.0 + 0.02 * c, 0.9 + 0.02 * c, 0.05 + 0.002 * c) for c in range(B26_CELLS)), seed=22, n_units=3),
    Case("B5", "Matern32", True, 200, 9, (0, 1, 1, 0, 1),
         tuple((1.0 + 0.1 * c, tuple(np.linspace(2.0, 4.0, 9) * (1.0 + 0.1 * c)), 0.02 * (c + 1)) for c in range(5)), seed=23),
    Case("B4", "Matern52", True, 70, 66, (0, 1, 0, 1),
         tuple((1.0 + 0.1 * c, tuple(np.linspace(6.0, 10.0, 66) * (1.0 + 0.05 * c)), 0.03 * (c + 1)) for c in range(4)), seed=24),
)
CASES = {c.id: c for c in SINGLE + STATE + BATCH}
PAIR = (7, 70)  # duplicates = "pair": row 70 is a copy of row 7 (two different tiles)


@functools.lru_cache(maxsize=None)
def data(cid: str):
    """(x, y) of a case: x (n, d), y (n, n_units), every entry a multiple of 2^-20; read-only."""
    c = CASES[cid]
    x, y, _ = (np.rint(a * DATA_GRID) / DATA_GRID for a in make_regression(c.n, c.d, n_outputs=c.n_units, n_test=0, config=43, unit=c.seed))
    if c.duplicates == "alternate":
        x[1::2] = x[0::2]
    elif c.duplicates == "pair":
        x[PAIR[1]] = x[PAIR[0]]
    for a in (x, y):
        a.setflags(write=False)
    return x, y


def thetas(cid: str) -> np.ndarray:
    """(cells, ntheta) unconstrained hyperparameters of a case, C order."""
    return np.ascontiguousarray(np.stack([theta_of(*h) for h in CASES[cid].hypers]))


def hyper(cid: str, cell: int = 0):
    """(variance, lengthscales (d of them), noise) the library works with in this cell."""
    v, ls, s = constrain(thetas(cid)[cell])
    return v, np.broadcast_to(ls, (CASES[cid].d,)), s


@functools.lru_cache(maxsize=None)
def reference_raw(cid: str, cell: int = 0) -> Raw:
    c = CASES[cid]
    x, y = data(cid)
    v, ls, s = hyper(cid, cell)
    return raw_ld(c.kernel, x, y[:, c.units[cell]], v, ls, s, c.ard, c.form)


def reference(cid: str, cell: int = 0, mask: int = ALL):
    """(loss, grad, loss_scale, grad_scale) of one cell, longdouble."""
    return finish(reference_raw(cid, cell), thetas(cid)[cell], mask)


# ---- error measures -----------------------------------------------------------------------------------------------------------------
def errors(loss, grad, ref) -> tuple:
    """(loss ratio, ratio of every gradient component) against a reference() tuple; untrained components (scale 0) report 0 when the
    value is exactly 0 and infinity otherwise."""
    ref_loss, ref_grad, loss_scale, grad_scale = ref
    el = float(abs(LD(loss) - ref_loss) / loss_scale)
    diff = np.abs(np.asarray(grad).astype(LD) - ref_grad)
    eg = [float(dk / sk) if sk > 0 else (0.0 if dk == 0 else np.inf) for dk, sk in zip(diff, grad_scale)]
    return el, eg


# ---- float64 restatement of the device route -------------------------------------------------------------------------------------------
def _perturb(rng, width, shape, symmetric=True):
    if rng is None:
        return 1.0
    e = rng.uniform(-width * U, width * U, shape)
    if symmetric and len(shape) == 2:
        e = np.tril(e) + np.tril(e, -1).T
    return LD(1) + e.astype(LD)


def r2_64(x, ls, form, rng):
    """r2 as the device forms it, in longdouble precision of representation: the difference form under its allowed relative error
    (4u), the expanded form from float64 norms and dot products (each under 2u) -- there the cancellation decides."""
    if form == "difference":
        return r2_ld(x, x, ls) * _perturb(rng, 4, (x.shape[0],) * 2)
    sa = np.asarray(x, np.float64) / np.asarray(ls, np.float64)[None, :]
    na = (sum64(sa * sa, axis=1).astype(LD) * _perturb(rng, 2, (x.shape[0],))).astype(np.float64)
    dot = (dot64(sa, sa.T).astype(LD) * _perturb(rng, 2, (x.shape[0],) * 2)).astype(np.float64)
    return ((na[:, None] + na[None, :]) - 2.0 * dot).astype(LD)


def tile_sums(terms, npad):
    """Per 64 x 64 tile sums of an (n, n) array of terms (zero above the diagonal): down the rows of a tile, then across."""
    n = terms.shape[0]
    t = np.zeros((npad, npad))
    t[:n, :n] = terms
    nt = npad // NB
    t = t.reshape(nt, NB, nt, NB).transpose(0, 2, 1, 3)
    return sum64(sum64(t, axis=2), axis=2)


@functools.lru_cache(maxsize=4)
def _emu_factor(cid: str, cell: int, seed):
    """The padded factor, its block inverses, beta, L^-1 and K^-1 of one cell (np x np; unit diagonal below row n, zeros in y)."""
    c = CASES[cid]
    x, y = data(cid)
    v, ls, s = hyper(cid, cell)
    rng = None if seed is None else np.random.default_rng([29, seed])
    n, npad = c.n, -(-c.n // NB) * NB
    k = np.eye(npad)
    if c.form == "difference":
        k[:n, :n] = kmat64(c.kernel, x, x, v, ls, rng, symmetric=True)
        k[np.arange(n), np.arange(n)] = v + s
    else:  # (the diagonal too comes out of the cancellation)
        g = g_ld(c.kernel, r2_64(x, ls, c.form, rng)) * _perturb(rng, 2, (n, n))
        k[:n, :n] = (LD(v) * g).astype(np.float64) + s * np.eye(n)
    low, inv = emu_chol(k)
    yp = np.zeros(npad)
    yp[:n] = y[:, c.units[cell]]
    beta = emu_trsv(low, inv, yp, False)
    xinv = emu_trtri(low, inv)
    kinv = dot64(xinv.T, xinv)
    return low, inv, beta, xinv, kinv, rng


def emu_raw(cid: str, cell: int = 0, seed=None, alpha_from_inverse=True) -> Raw:
    c = CASES[cid]
    x, _ = data(cid)
    v, ls, s = hyper(cid, cell)
    n, d = c.n, c.d
    low, inv, beta, xinv, kinv, rng = _emu_factor(cid, cell, seed)
    npad = low.shape[0]
    alpha = (dot64(xinv.T, beta) if alpha_from_inverse else emu_trsv(low, inv, beta, True))[:n]
    lml = -0.5 * sum64(beta * beta) - sum64(log_ld(np.diag(low)).astype(np.float64)) - 0.5 * n * LOG_2PI
    rng2 = None if seed is None else np.random.default_rng([31, seed])
    r2 = r2_64(x, ls, c.form, rng2)
    g = (g_ld(c.kernel, r2) * _perturb(rng2, 2, (n, n))).astype(np.float64)
    h = (h_ld(c.kernel, r2) * _perturb(rng2, 2, (n, n))).astype(np.float64)
    w = alpha[:, None] * alpha[None, :] - kinv[:n, :n]
    w = 2.0 * np.tril(w, -1) + np.diag(np.diag(w))  # tiles on or below the diagonal, the off-diagonal weights doubled
    total = lambda terms, scale=1.0: sum64((tile_sums(terms, npad) * scale).ravel())  # tile partials in tile order
    wh = (w * v) * h
    if not c.ard and c.form == "difference":  # the isotropic shortcut: -sum wh r2 / l
        dls = np.array([total(wh * r2.astype(np.float64), -1.0 / ls[0])])
    else:
        dls = np.zeros(d)
        for kk in range(d):
            col = x[:, kk] * (1.0 / ls[kk]) if c.form == "difference" else x[:, kk] / ls[kk]
            ds = col[:, None] - col[None, :]
            dls[kk] = total((wh * ds) * ds, -1.0 / ls[kk])
        if not c.ard:
            dls = np.array([sum64(dls)])
    du = 0.5 * np.concatenate([[total(w * g)], dls, [total(np.diag(np.diag(w)))]])
    return Raw(lml, du)


def emu_objective(cid: str, cell: int = 0, seed=None, alpha_from_inverse=True, mask: int = ALL):
    """(loss, grad) of the float64 restatement."""
    loss, grad, _, _ = finish(emu_raw(cid, cell, seed, alpha_from_inverse), thetas(cid)[cell], mask, np.float64)
    return loss, grad


# ---- recorded bounds ----------------------------------------------------------------------------------------------------------------
def key(cid, cell, route, mask, quantity) -> str:
    return f"{cid}/c{cell}/{route}/m{mask}/{quantity}"


def expected_keys() -> set:
    """Every entry the bounds file must hold: case, cell, route, mask, and the loss plus each TRAINED gradient component."""
    out = set()
    for cid, c in CASES.items():
        nlen = c.d if c.ard else 1
        for cell in range(len(c.units)):
            for route in ROUTES:
                for mask in c.masks:
                    out.add(key(cid, cell, route, mask, "loss"))
                    out.update(key(cid, cell, route, mask, f"g{k}") for k in np.flatnonzero(trained(mask, nlen)))
    return out


def case_ratios(cid: str) -> dict:
    """The worst error of the restatement over the unperturbed run and the perturbation seeds, never reported below u (neither the
    reference rounded to double nor a result's own last rounding resolves finer)."""
    c = CASES[cid]
    out = {}
    for cell in range(len(c.units)):
        theta = thetas(cid)[cell]
        for seed in (None,) + PERTURB_SEEDS:
            for route in ROUTES:
                raw = emu_raw(cid, cell, seed, route == "from_inverse")
                for mask in c.masks:
                    loss, grad, _, _ = finish(raw, theta, mask, np.float64)
                    el, eg = errors(loss, grad, reference(cid, cell, mask))
                    k = key(cid, cell, route, mask, "loss")
                    out[k] = max(out.get(k, U), el)
                    for j in np.flatnonzero(trained(mask, theta.size - 2)):
                        k = key(cid, cell, route, mask, f"g{j}")
                        out[k] = max(out.get(k, U), eg[j])
    return out


def compute_bounds() -> dict:
    """Every recorded ratio.  Deterministic: the same file bit for bit."""
    out = {}
    for cid in CASES:
        out.update(case_ratios(cid))
    return out


@functools.lru_cache(maxsize=None)
def bounds() -> dict:
    with open(BOUNDS_PATH) as fh:
        return json.load(fh)


def recorded(cid, cell, route, mask, quantity) -> float:
    """The recorded ratio; a missing entry is a KeyError (a test failure, never a skip)."""
    return bounds()[key(cid, cell, route, mask, quantity)]
