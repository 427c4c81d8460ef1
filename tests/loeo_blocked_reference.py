"""Plain-numpy references for the blocked leave-one-event-out route (test_gpu_loeo_blocked.py): no GPU is imported here.

The route (gpras_amd/csrc/gp_loeo_blocked.h) is the downdate of csrc/sf_loeo.h for 64 < M <= 320: one factorisation on
all rows, then per event H = I - t2 t2^T / s (mp x mp), Lh = chol(H), P = Lh^-1 as an explicit inverse, c' = P (c - u / s) with
u = t2 y[lo:hi], W = P t2, mean = W^T c', var = ((v - colsum(t1^2)) + colsum(W^2)) + s.

The reference is the DEFINITION, loeo_ld, as in loeo_reference.py: SGPR predict_y in np.longdouble of the model on the data without the
event's rows.  emu_blocked restates the route in float64 with sequential sums, emu_refactor the refactor route (the definition on
existing calls) beside it; tests/golden/make_loeo_blocked_bounds.py records how far each lands from loeo_ld per case, cell and route
(the maximum over the unperturbed run and three perturbation seeds, never below u); the GPU tests allow 8 x that.

This module has its OWN case table (loeo_reference.CASES is parametrised over by test_gpu_loeo.py at collection time) and takes only the
case-independent helpers of loeo_reference.py, predict_reference.py and blocks_reference.py.
"""

from __future__ import annotations

import functools
import json
import os
from typing import NamedTuple

import numpy as np

import predict_reference as pr
from blocks_reference import LD, U, dot64, sum64
from gpras_amd.synth import make_regression
from loeo_reference import JITTER, MARGIN, PERTURB_SEEDS, TILE, _sgpr_factor64, kept_rows, kmat64_form, kmat_form_ld, sgpr_predict_ld, solve64

BOUNDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loeo_blocked_bounds.json")
HYPERS = ((1.0, 0.9, 0.1), (1.3, 1.2, 0.06))  # two modes: (variance, lengthscale, noise), constrained


class Case(NamedTuple):
    id: str
    kernel: str
    form: str
    n: int
    m: int
    events: tuple  # sorted, disjoint (lo, hi)
    seed: int
    routes: tuple = ("blocked", "refactor")
    d: int = 3
    hypers: tuple = HYPERS

    @property
    def mp(self) -> int:
        return 64 * ((self.m + 63) // 64)


# a lone row, a 64-row event from an odd first column, 65 rows, a long event; rows 0-1, 135-139 belong to no event
EV300 = ((2, 3), (3, 67), (70, 135), (140, 300))
# chunk edges 63 / 64 / 65, an odd first column (129), a 199-row event (four chunks); rows 0 and 194-200 belong to no event
EV400 = ((1, 2), (2, 65), (65, 129), (129, 194), (201, 400))

CASES = {c.id: c for c in (
    # one band through the blocked route, on data the one-workgroup downdate takes too
    Case("B50", "RBF", "difference", 300, 50, EV300, seed=11, routes=("blocked", "refactor", "downdate")),
    Case("B65", "RBF", "difference", 300, 65, EV300, seed=12),     # one real row in the second band, identity padding in the rest
    Case("B128", "RBF", "difference", 300, 128, EV300, seed=13),   # two full bands, 3 lower tiles
    Case("B130", "RBF", "difference", 400, 130, EV400, seed=14),   # an odd band count: the ragged pair of the triangular inverse
    Case("B320", "RBF", "difference", 400, 320, ((0, 64), (64, 193), (200, 400)), seed=15),  # five bands, 15 tiles, the largest slot
    Case("B70T", "RBF", "difference", 4200, 70, ((0, 2000), (2000, 4000), (4000, 4200)), seed=16),  # two tiles
    Case("BM32", "Matern32", "expanded", 400, 130, EV400, seed=17),  # the other distance form through the general head
)}


@functools.lru_cache(maxsize=None)
def data(cid: str):
    """(x (n, d), y (n, cells), zs (cells, m, d)), every entry a multiple of 2^-20; read-only (the rule of loeo_reference.data)."""
    c = CASES[cid]
    x, y, _ = (np.rint(a * pr.DATA_GRID) / pr.DATA_GRID for a in make_regression(c.n, c.d, n_outputs=len(c.hypers), config=43, unit=c.seed))
    rows = np.linspace(0, c.n - 1, c.m).astype(np.int64)
    zs = np.ascontiguousarray(np.stack([x[rows] + (cell + 1) / 32.0 for cell in range(len(c.hypers))]))
    for a in (x, y, zs):
        a.setflags(write=False)
    return x, y, zs


def thetas(cid: str) -> np.ndarray:
    return np.ascontiguousarray(np.stack([pr.theta_of(*h) for h in CASES[cid].hypers]))


def hyper(cid: str, cell: int):
    """(variance, lengthscales, noise) the library works with in this cell."""
    return pr.constrain(thetas(cid)[cell])


def event_mask(cid: str) -> np.ndarray:
    mask = np.zeros(CASES[cid].n, dtype=bool)
    for lo, hi in CASES[cid].events:
        mask[lo:hi] = True
    return mask


def mean_err(cid, got, ref) -> float:
    k = event_mask(cid)
    return pr.mean_err(np.asarray(got)[k], ref[k])


def var_err(cid, got, ref) -> float:
    k = event_mask(cid)
    return pr.var_err(np.asarray(got)[k], ref[k])


# ---- longdouble definition ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loeo_ld(cid: str, cell: int):
    """(mean, var_y), each (n,) longdouble: at every event's rows the prediction of the model on all other rows; NaN elsewhere."""
    c = CASES[cid]
    x, y, zs = data(cid)
    v, ls, s = hyper(cid, cell)
    mean, var = np.full(c.n, np.nan, LD), np.full(c.n, np.nan, LD)
    kuu = kmat_form_ld(c.kernel, zs[cell], zs[cell], v, ls, c.form) + LD(JITTER) * np.eye(c.m, dtype=LD)
    kuf = kmat_form_ld(c.kernel, zs[cell], x, v, ls, c.form)
    for lo, hi in c.events:
        keep = kept_rows(c.n, lo, hi)
        mean[lo:hi], var[lo:hi] = sgpr_predict_ld(kuu, kuf[:, keep], y[keep, cell], kuf[:, lo:hi], v, s)
    mean.setflags(write=False)
    var.setflags(write=False)
    return mean, var


# ---- float64 restatements -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _emu_blocks(cid: str, cell: int, seed):
    """(kuu with jitter, kuf) of one cell on ALL rows in float64 under perturbation `seed` (None: the longdouble kernel rounded)."""
    c = CASES[cid]
    x, _, zs = data(cid)
    v, ls, _ = hyper(cid, cell)
    rng = None if seed is None else np.random.default_rng([37, seed, cell])
    kuu = kmat64_form(c.kernel, zs[cell], zs[cell], v, ls, c.form, rng, symmetric=True)
    if c.form == "difference":
        kuu[np.diag_indices_from(kuu)] = v
    kuu = kuu + JITTER * np.eye(c.m)
    return kuu, kmat64_form(c.kernel, zs[cell], x, v, ls, c.form, rng)


def emu_refactor(cid, cell, seed=None):
    """The refactor route: per event the model on the remaining rows, predict_y at the event's rows."""
    c = CASES[cid]
    _, y, _ = data(cid)
    v, _, s = hyper(cid, cell)
    kuu, kuf = _emu_blocks(cid, cell, seed)
    mean, var = np.full(c.n, np.nan), np.full(c.n, np.nan)
    for lo, hi in c.events:
        keep = kept_rows(c.n, lo, hi)
        low, _, lb, cvec = _sgpr_factor64(kuu, kuf[:, keep], y[keep, cell], s)
        t1 = solve64(low, kuf[:, lo:hi])
        t2 = solve64(lb, t1)
        mean[lo:hi] = dot64(t2.T, cvec)
        var[lo:hi] = ((v + s) - sum64(t1 * t1, axis=0)) + sum64(t2 * t2, axis=0)
    return mean, var


def _emu_down(cid, cell, seed, explicit_inverse):
    c = CASES[cid]
    _, y, _ = data(cid)
    v, _, s = hyper(cid, cell)
    kuu, kuf = _emu_blocks(cid, cell, seed)
    _, a, lb, cvec = _sgpr_factor64(kuu, kuf, y[:, cell], s)
    mean, var = np.full(c.n, np.nan), np.full(c.n, np.nan)
    for lo, hi in c.events:
        t1 = a[:, lo:hi]  # = L^-1 k(Z, X[lo:hi])
        t2 = solve64(lb, t1)
        lh = pr.chol64(np.eye(c.m) - dot64(t2, t2.T) / s)
        b = cvec - dot64(t2, y[lo:hi, cell]) / s
        if explicit_inverse:
            p = solve64(lh, np.eye(c.m))
            cp, w = dot64(p, b), dot64(p, t2)
        else:
            cp, w = solve64(lh, b), solve64(lh, t2)
        mean[lo:hi] = dot64(w.T, cp)
        var[lo:hi] = ((v - sum64(t1 * t1, axis=0)) + sum64(w * w, axis=0)) + s
    return mean, var


def emu_blocked(cid, cell, seed=None):
    """The blocked route: H, chol64, P = Lh^-1 as the explicit inverse, c' = P (c - u / s), W = P t2."""
    return _emu_down(cid, cell, seed, True)


def emu_downdate(cid, cell, seed=None):
    """The one-workgroup downdate (loeo_reference.emu_downdate on this module's data): substitutions in the place of P."""
    return _emu_down(cid, cell, seed, False)


EMU = {"blocked": emu_blocked, "refactor": emu_refactor, "downdate": emu_downdate}


def case_ratios(cid: str) -> dict:
    """{"<id>/c<cell>/<route>/<mean|var>": ratio}: the worst error of a route's restatement over the unperturbed run and the perturbation
    seeds, never reported below u (the rule of loeo_reference.case_ratios)."""
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


__all__ = ["CASES", "MARGIN", "TILE", "U", "allowed", "bounds", "compute_bounds", "data", "emu_blocked", "emu_refactor", "hyper", "loeo_ld", "thetas"]
