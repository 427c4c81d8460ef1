"""Plain-numpy references for the leave-one-event-out tests (test_gpu_loeo.py): no GPU is imported here.

The reference of a leave-one-event-out prediction is its DEFINITION, loeo_ld: for every event, SGPR predict_y (oracle/sgpr.py's
formulas: L = chol(Kuu + jitter I), A' = L^-1 Kuf, B = I + A' A'^T / s, c = LB^-1 A' y / s, mean = t2^T c, var = v + colsum(t2^2) -
colsum(t1^2) + s) of the model on the data WITHOUT the event's rows, at the event's rows, all in np.longdouble with no BLAS and no libm
in between (predict_reference.py: exp_ld; blocks_reference.py: chol_ld, solve_lower_ld).  Exact models: predict_reference.predict_ld on
the reduced data.  test_loeo_reference.py pins it to oracle.sgpr / oracle.exact on the reduced data.

emu_refactor / emu_downdate restate the two routes of gpras_amd/loeo.py in float64, every sum sequential: the refactor route is the
definition itself; the downdate route (csrc/sf_loeo.h) factorises once on all rows and, per event, H = I - t2 t2^T / s, Lh = chol(H),
c' = Lh^-1 (c - t2 y / s), W = Lh^-1 t2.  Their kernel entries are the longdouble kernel rounded to double, perturbed by what the
device's kernel build is allowed (predict_reference.kmat64: r2 (1 + d1), |d1| <= 4u, g (1 + d2), |d2| <= 2u; the expanded distance
form from float64 norms and dot products, each under 2u, as objective_reference.r2_64).  tests/golden/make_loeo_bounds.py records how
far they land from loeo_ld per case, cell and route (the maximum over the unperturbed run and three perturbation seeds, never below u);
the GPU tests allow 8 x that.

Hyperparameters, data grid and the no-libm rule are predict_reference.py's: a case states constrained values, theta is their inverse
softplus on a grid of 2^-30, every reference works with the longdouble softplus of that theta rounded to double; the data are rounded
to multiples of 2^-20.
"""

from __future__ import annotations

import functools
import json
import os
from typing import NamedTuple

import numpy as np

import predict_reference as pr
from blocks_reference import LD, U, chol_ld, dot64, solve_lower_ld, sum64
from gpras_amd.synth import make_regression

JITTER = 1e-6
MARGIN = 8.0
PERTURB_SEEDS = (0, 1, 2)
BOUNDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loeo_bounds.json")
TILE = 4096  # rows of one tile of the sparse predict (csrc/gp_sparse.h SGPR_PRED_TILE)


class Case(NamedTuple):
    """One data set (n, d, one output per cell) with its events and the cells (modes) predicted on it.  m = 0: exact models."""
    id: str
    kernel: str
    ard: bool
    form: str
    n: int
    d: int
    m: int
    events: tuple         # sorted, disjoint (lo, hi)
    hypers: tuple         # (variance, lengthscale(s), noise) of each cell, constrained
    seed: int
    routes: tuple = ("downdate", "refactor")


# a lone row, both sides of the 64-column chunk edge, several chunks; rows 0-1, 133-141 and 507-699 belong to no event
BASE_EVENTS = ((2, 3), (3, 6), (6, 69), (69, 133), (142, 207), (207, 507))
BASE_HYPERS = ((1.0, 0.9, 0.1), (1.3, 1.2, 0.06), (0.8, 0.7, 0.15))
_ARD_LS = tuple((0.7 + 0.1 * c, 1.0 + 0.1 * c, 1.4 - 0.1 * c) for c in range(3))


def _base(cid, kernel, m, seed, ard=False, form="difference"):
    hypers = tuple((v, _ARD_LS[c], s) for c, (v, _, s) in enumerate(BASE_HYPERS)) if ard else BASE_HYPERS
    return Case(cid, kernel, ard, form, 700, 3, m, BASE_EVENTS, hypers, seed)


CASES = {c.id: c for c in (
    _base("M5", "RBF", 5, seed=1),
    _base("M50", "RBF", 50, seed=2),
    _base("M64", "RBF", 64, seed=3),
    _base("ARD", "RBF", 50, seed=4, ard=True),
    _base("K-diff", "Matern32", 50, seed=5),
    _base("K-exp", "Matern52", 50, seed=6, form="expanded"),
    # the third event does not fit the first tile beside the other two (span 4200 > 4096): a second tile
    Case("TILE", "RBF", False, "difference", 4200, 3, 50, ((0, 2000), (2000, 4000), (4000, 4200)), BASE_HYPERS[:2], seed=7),
    # models the downdate kernel does not take: route "auto" runs the refactor route
    Case("M70", "RBF", False, "difference", 300, 3, 70, ((0, 65), (65, 130), (140, 300)), BASE_HYPERS[:2], seed=8, routes=("refactor",)),
    Case("EXACT", "RBF", False, "difference", 200, 3, 0, ((0, 50), (60, 130), (130, 200)), BASE_HYPERS[:2], seed=9, routes=("refactor",)),
)}
DOWNDATE_CASES = tuple(cid for cid, c in CASES.items() if "downdate" in c.routes)


@functools.lru_cache(maxsize=None)
def data(cid: str):
    """(x (n, d), y (n, cells), zs (cells, m, d) or None), every entry a multiple of 2^-20; read-only.  The inducing inputs of cell c:
    m rows of x spread over the data, shifted by (c + 1) / 32 so that none coincides with a training row."""
    c = CASES[cid]
    x, y, _ = (np.rint(a * pr.DATA_GRID) / pr.DATA_GRID for a in make_regression(c.n, c.d, n_outputs=len(c.hypers), config=43, unit=c.seed))
    zs = None
    if c.m:
        rows = np.linspace(0, c.n - 1, c.m).astype(np.int64)
        zs = np.ascontiguousarray(np.stack([x[rows] + (cell + 1) / 32.0 for cell in range(len(c.hypers))]))
        zs.setflags(write=False)
    for a in (x, y):
        a.setflags(write=False)
    return x, y, zs


def thetas(cid: str) -> np.ndarray:
    return np.ascontiguousarray(np.stack([pr.theta_of(*h) for h in CASES[cid].hypers]))


def hyper(cid: str, cell: int):
    """(variance, lengthscales, noise) the library works with in this cell."""
    return pr.constrain(thetas(cid)[cell])


def kept_rows(n: int, lo: int, hi: int) -> np.ndarray:
    return np.r_[0:lo, hi:n]


# ---- longdouble definition ---------------------------------------------------------------------------------------------------------
def r2_form_ld(a, b, ls, form):
    """Scaled squared distances in the handle's distance form, longdouble."""
    if form == "difference":
        return pr.r2_ld(a, b, ls)
    lsv = np.broadcast_to(np.asarray(ls).astype(LD), (np.shape(a)[1],))
    sa, sb = np.asarray(a).astype(LD) / lsv[None, :], np.asarray(b).astype(LD) / lsv[None, :]
    na, nb, dot = np.zeros(sa.shape[0], LD), np.zeros(sb.shape[0], LD), np.zeros((sa.shape[0], sb.shape[0]), LD)
    for k in range(sa.shape[1]):
        na = na + sa[:, k] * sa[:, k]
        nb = nb + sb[:, k] * sb[:, k]
        dot = dot + sa[:, k][:, None] * sb[:, k][None, :]
    return (na[:, None] + nb[None, :]) - LD(2) * dot


def kmat_form_ld(kernel, a, b, variance, ls, form):
    return LD(variance) * pr.g_ld(kernel, r2_form_ld(a, b, ls, form))


def sgpr_predict_ld(kuu, kuf, y, kus, variance, noise, include_noise=True):
    """SGPR predict_y in longdouble from the kernel blocks: kuu (m, m) WITH the jitter, kuf (m, n), kus (m, ns)."""
    v, s = LD(variance), LD(noise)
    low = chol_ld(kuu)
    a = solve_lower_ld(low, kuf)
    lb = chol_ld(np.eye(kuu.shape[0], dtype=LD) + (a @ a.T) / s)
    c = solve_lower_ld(lb, a @ np.asarray(y).astype(LD)) / s
    t1 = solve_lower_ld(low, kus)
    t2 = solve_lower_ld(lb, t1)
    var = v + np.sum(t2 * t2, axis=0) - np.sum(t1 * t1, axis=0)
    return t2.T @ c, (var + s if include_noise else var)


@functools.lru_cache(maxsize=None)
def loeo_ld(cid: str, cell: int):
    """(mean, var_y), each (n,) longdouble: at every event's rows the prediction of the model on all other rows; NaN elsewhere.
    Read-only."""
    c = CASES[cid]
    x, y, zs = data(cid)
    v, ls, s = hyper(cid, cell)
    mean, var = np.full(c.n, np.nan, LD), np.full(c.n, np.nan, LD)
    if c.m:
        kuu = kmat_form_ld(c.kernel, zs[cell], zs[cell], v, ls, c.form) + LD(JITTER) * np.eye(c.m, dtype=LD)
        kuf = kmat_form_ld(c.kernel, zs[cell], x, v, ls, c.form)
    for lo, hi in c.events:
        keep = kept_rows(c.n, lo, hi)
        if c.m:
            mean[lo:hi], var[lo:hi] = sgpr_predict_ld(kuu, kuf[:, keep], y[keep, cell], kuf[:, lo:hi], v, s)
        else:
            mean[lo:hi], var[lo:hi] = pr.predict_ld(c.kernel, x[keep], y[keep, cell], v, ls, s, x[lo:hi], True)
    mean.setflags(write=False)
    var.setflags(write=False)
    return mean, var


# ---- error measures (over the rows of the events) ------------------------------------------------------------------------------------
def event_mask(cid: str) -> np.ndarray:
    mask = np.zeros(CASES[cid].n, dtype=bool)
    for lo, hi in CASES[cid].events:
        mask[lo:hi] = True
    return mask


def mean_err(cid, got, ref) -> float:
    """max |m - ref| / max |ref| over the rows of the events"""
    k = event_mask(cid)
    return pr.mean_err(np.asarray(got)[k], ref[k])


def var_err(cid, got, ref) -> float:
    """max (|v - ref| / ref) over the rows of the events, on the variance with the noise term"""
    k = event_mask(cid)
    return pr.var_err(np.asarray(got)[k], ref[k])


# ---- float64 restatement of the two routes ----------------------------------------------------------------------------------------------
def _perturb(rng, width, shape, symmetric=False):
    if rng is None:
        return LD(1)
    e = rng.uniform(-width * U, width * U, shape)
    if symmetric:
        e = np.tril(e) + np.tril(e, -1).T
    return LD(1) + e.astype(LD)


def kmat64_form(kernel, a, b, variance, ls, form, rng=None, symmetric=False):
    """The kernel block as the device may form it, rounded to double."""
    if form == "difference":
        return pr.kmat64(kernel, a, b, variance, ls, rng, symmetric)
    lsv = np.broadcast_to(np.asarray(ls, np.float64), (np.shape(a)[1],))
    sa, sb = np.asarray(a, np.float64) / lsv[None, :], np.asarray(b, np.float64) / lsv[None, :]
    na = (sum64(sa * sa, axis=1).astype(LD) * _perturb(rng, 2, (sa.shape[0],))).astype(np.float64)
    nb = na if symmetric else (sum64(sb * sb, axis=1).astype(LD) * _perturb(rng, 2, (sb.shape[0],))).astype(np.float64)
    dot = (dot64(sa, sb.T).astype(LD) * _perturb(rng, 2, (sa.shape[0], sb.shape[0]), symmetric)).astype(np.float64)
    r2 = ((na[:, None] + nb[None, :]) - 2.0 * dot).astype(LD)
    g = pr.g_ld(kernel, r2) * _perturb(rng, 2, r2.shape, symmetric)
    return (LD(variance) * g).astype(np.float64)


def solve64(low, b):
    """L x = b by column-oriented substitution, float64: every element takes its subtractions in k order, one rounding per product and
    per subtraction."""
    x = np.array(b, dtype=np.float64)
    flat = x.reshape(x.shape[0], -1)
    for k in range(low.shape[0]):
        flat[k] = flat[k] / low[k, k]
        flat[k + 1:] -= low[k + 1:, k, None] * flat[k][None, :]
    return x


def solve64_t(low, b):
    """L^T x = b the same way, bottom up."""
    x = np.array(b, dtype=np.float64)
    flat = x.reshape(x.shape[0], -1)
    for k in range(low.shape[0] - 1, -1, -1):
        flat[k] = flat[k] / low[k, k]
        flat[:k] -= low[k, :k, None] * flat[k][None, :]
    return x


@functools.lru_cache(maxsize=4)
def _emu_blocks(cid: str, cell: int, seed):
    """The float64 kernel blocks of one cell on ALL rows -- (kuu with jitter, kuf) of a sparse model, (K without the noise,) of an exact
    one -- under perturbation `seed` (None: the longdouble kernel rounded to double)."""
    c = CASES[cid]
    x, _, zs = data(cid)
    v, ls, _ = hyper(cid, cell)
    rng = None if seed is None else np.random.default_rng([31, seed, cell])
    if not c.m:
        return (kmat64_form(c.kernel, x, x, v, ls, c.form, rng, symmetric=True),)
    kuu = kmat64_form(c.kernel, zs[cell], zs[cell], v, ls, c.form, rng, symmetric=True)
    if c.form == "difference":
        kuu[np.diag_indices_from(kuu)] = v
    kuu = kuu + JITTER * np.eye(c.m)
    return kuu, kmat64_form(c.kernel, zs[cell], x, v, ls, c.form, rng)


def _sgpr_factor64(kuu, kuf, y, s):
    low = pr.chol64(kuu)
    a = solve64(low, kuf)
    lb = pr.chol64(np.eye(kuu.shape[0]) + dot64(a, a.T) / s)
    return low, a, lb, solve64(lb, dot64(a, y) / s)


def emu_refactor(cid, cell, seed=None):
    """The refactor route: per event the model on the remaining rows, predict_y at the event's rows.  (mean, var), NaN outside events."""
    c = CASES[cid]
    _, y, _ = data(cid)
    v, _, s = hyper(cid, cell)
    blocks = _emu_blocks(cid, cell, seed)
    mean, var = np.full(c.n, np.nan), np.full(c.n, np.nan)
    for lo, hi in c.events:
        keep = kept_rows(c.n, lo, hi)
        if c.m:
            kuu, kuf = blocks
            low, _, lb, cvec = _sgpr_factor64(kuu, kuf[:, keep], y[keep, cell], s)
            t1 = solve64(low, kuf[:, lo:hi])
            t2 = solve64(lb, t1)
            mean[lo:hi] = dot64(t2.T, cvec)
            var[lo:hi] = ((v + s) - sum64(t1 * t1, axis=0)) + sum64(t2 * t2, axis=0)
        else:
            k = blocks[0][np.ix_(keep, keep)].copy()
            k[np.diag_indices_from(k)] = v + s
            low = pr.chol64(k)
            alpha = solve64_t(low, solve64(low, y[keep, cell]))
            ks = blocks[0][np.ix_(keep, np.arange(lo, hi))]
            vmat = solve64(low, ks)
            mean[lo:hi] = dot64(ks.T, alpha)
            var[lo:hi] = (v + s) - sum64(vmat * vmat, axis=0)
    return mean, var


def emu_downdate(cid, cell, seed=None):
    """The downdate route: one factorisation on all rows, then per event H = I - t2 t2^T / s, Lh = chol(H), c' = Lh^-1 (c - t2 y / s),
    W = Lh^-1 t2, mean = W^T c', var = ((v - colsum(t1^2)) + colsum(W^2)) + s."""
    c = CASES[cid]
    _, y, _ = data(cid)
    v, _, s = hyper(cid, cell)
    kuu, kuf = _emu_blocks(cid, cell, seed)
    low, a, lb, cvec = _sgpr_factor64(kuu, kuf, y[:, cell], s)
    mean, var = np.full(c.n, np.nan), np.full(c.n, np.nan)
    for lo, hi in c.events:
        t1 = a[:, lo:hi]  # = L^-1 k(Z, X[lo:hi])
        t2 = solve64(lb, t1)
        lh = pr.chol64(np.eye(c.m) - dot64(t2, t2.T) / s)
        cp = solve64(lh, cvec - dot64(t2, y[lo:hi, cell]) / s)
        w = solve64(lh, t2)
        mean[lo:hi] = dot64(w.T, cp)
        var[lo:hi] = ((v - sum64(t1 * t1, axis=0)) + sum64(w * w, axis=0)) + s
    return mean, var


EMU = {"downdate": emu_downdate, "refactor": emu_refactor}


def case_ratios(cid: str) -> dict:
    """{"<id>/c<cell>/<route>/<mean|var>": ratio}: the worst error of a route's restatement over the unperturbed run and the perturbation
    seeds, never reported below u."""
    c = CASES[cid]
    out = {}
    for cell in range(len(c.hypers)):
        ref_mean, ref_var = loeo_ld(cid, cell)
        worst = {(r, q): U for r in c.routes for q in ("mean", "var")}
        for seed in (None,) + PERTURB_SEEDS:
            for route in c.routes:
                mean, var = EMU[route](cid, cell, seed)
                worst[route, "mean"] = max(worst[route, "mean"], mean_err(cid, mean, ref_mean))
                worst[route, "var"] = max(worst[route, "var"], var_err(cid, var, ref_var))
        for (route, q), val in worst.items():
            out[f"{cid}/c{cell}/{route}/{q}"] = val
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


def allowed(cid: str, cell: int, route: str, quantity: str) -> float:
    """What a device result may be off by: MARGIN x the recorded ratio."""
    return MARGIN * bounds()[f"{cid}/c{cell}/{route}/{quantity}"]
