"""Plain-numpy references for the joint-prediction route tests (test_gpu_joint_routes.py): no GPU is imported here.

The reference of a joint prediction is its DEFINITION, joint_ld: oracle/sgpr.py:187-197 with the diagonal kept joint,
  L = chol(Kuu + jitter I), A' = L^-1 Kuf, B = I + A' A'^T / s, LB = chol(B), c = LB^-1 A' y / s,
  t1 = L^-1 Kus, t2 = LB^-1 t1, mean = t2^T c, C = Kss - t1^T t1 + t2^T t2 + (s, or jitter v) I, Lref = chol(C),
all in np.longdouble with no BLAS and no libm in between (loeo_reference.kmat_form_ld; blocks_reference.chol_ld, solve_lower_ld;
predict_reference.exp_ld).  test_joint_reference.py checks it against mpmath at 50 digits, against loeo_reference.sgpr_predict_ld and
against the float64 mirror ensemble_numpy.joint_covariance.

Every covariance entry is measured against its NATURAL SCALE, the sum of the magnitudes of the terms that make it up (the convention of
sparse_objective_reference.py): S_ij = |Kss_ij| + (|t1|^T |t1|)_ij + (|t2|^T |t2|)_ij + delta_ij (the diagonal term), so a small entry
cannot hide behind a large one.  The three measures:
  mean    max |m - ref| / max |ref|                                       (predict_reference.mean_err)
  cov     max_ij |Lc Lc^T - C|_ij / S_ij, the product Lc Lc^T formed in longdouble from the float64 factor that was returned
  factor  max_{i >= j} |Lc_ij - Lref_ij| / sqrt(C_ii)                    (sqrt(C_ii) is the norm of row i of the factor)

emu_joint restates csrc/gp_joint.h's predict_joint_batch in float64: L, LB and c as sparse_objective_reference.emu_raw forms them (the
blocked factorisations with explicit inverse diagonal blocks, S = A' A'^T and u = A' y as partial sums per 256 columns, c carried as an
appended row of the factorisation of B), kernel entries through loeo_reference.kmat64_form under the perturbations the device's build
is allowed (r2 (1 + d1), |d1| <= 4u, g (1 + d2), |d2| <= 2u; the expanded form from float64 norms and dot products; every constrained
hyperparameter one ulp beside the correctly rounded softplus), Kss built symmetric, t1 = emu_trsm(L, ., Kus), t2 = emu_trsm(LB, ., t1),
the mean by blocks_reference.emu_colreduce with 256 rows per chunk, C0 = fl(Kss + the diagonal term), then C0 - t1^T t1, then + t2^T t2
(the order of the two beta = 1 GEMMs), and blocks_reference.emu_potrf on the matrix padded with the identity to Tp.
tests/golden/make_joint_bounds.py records how far it lands from joint_ld per case, cell and include_noise (the maximum over the
unperturbed run and three perturbation seeds, never below u); the GPU tests allow 8 x that.

Hyperparameters, data grid and the no-libm rule are predict_reference.py's: a case states constrained values, theta is their inverse
softplus on a grid of 2^-30, every reference works with the longdouble softplus of that theta rounded to double; data, inducing inputs
and event rows are multiples of 2^-20.
"""

from __future__ import annotations

import functools
import json
import os
from typing import NamedTuple

import numpy as np

import loeo_reference as lr
import predict_reference as pr
from blocks_reference import LD, NB, U, chol_ld, dot64, emu_colreduce, emu_potrf, emu_trsm, solve_lower_ld
from gpras_amd.synth import make_regression
from loeo_reference import kmat_form_ld
from predict_reference import DATA_GRID, KERNEL_IDS, MARGIN, PERTURB_SEEDS, constrain, theta_of
from sparse_objective_reference import CLASSES, class_flags

BOUNDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "joint_bounds.json")
JITTER = 1e-6
CHUNK = 256           # csrc/gp_sparse.h SPLITK_CHUNK (S and u of the factorisation), rows_per_chunk of the mean's column reduce
N_TRAIN, N_UNITS, MAX_NS = 300, 3, 1024
BASELINE_TOL = 1e-8   # the absolute bound of test_gpu_ensemble.py's joint tests, in units of (variance + noise): the cap of every new bound
KERNELS = tuple(KERNEL_IDS)
canary, is_canary = pr.canary, pr.is_canary
mean_err = pr.mean_err


class Case(NamedTuple):
    """One model shape (kernel, class, d, m) on the shared data set layout (300 training rows, three outputs) and one event of ns rows.
    Cell c has unit c mod 3 and hyperparameter set c div 3."""
    id: str
    group: str   # factors | build | rows | cells24
    kernel: str
    cls: str
    d: int
    m: int
    ns: int
    cells: int
    seed: int
    ls_scale: float = 1.0  # the lengthscales are multiplied by this (EXPANDED_ISO_LS)

    @property
    def ard(self):
        return class_flags(self.kernel, self.cls)[0]

    @property
    def form(self):
        return class_flags(self.kernel, self.cls)[1]

    @property
    def nlen(self):
        return self.d if self.ard else 1

    @property
    def tp(self):
        return -(-self.ns // NB) * NB

    @property
    def mp(self):
        return -(-self.m // NB) * NB


FACTOR_M = (1, 50, 64, 65, 192, 300, 320)   # fused: 1, 50, 64; mp = 128 nearly all padding: 65; mp = 320, two row chunks: 300, 320
FACTOR_NS = (65, 130)
ROWS_KERNELS = ("RBF", "Matern32")
ROWS_NS = (1, 64, 65, 256, 257, 300, 1024)
C24_SETS = 8
# Matern12 and Exponential in the expanded form: k depends on r = sqrt(r2), and on the diagonal of Kss and Kuu the float64 cancellation
# |a|^2 + |a|^2 - 2 a.a leaves a residue of a few u |a / l|^2 where the longdouble definition has 1e-19 of it -- k moves by
# v sqrt(u) |a| / l, 1e-7 of itself at l = 0.9: a property of the form (sparse_objective_reference.py), a hundred times the cap that
# make_joint_bounds.py holds every recorded bound to.  The residue falls as 1 / l, so these cases take lengthscales 256 times as long;
# Matern12 stays well conditioned there (cond(Kuu) grows like l, not like a power of it).
EXPANDED_ISO_LS = 256.0


def _table():
    out, i = [], 0

    def add(cid, group, kernel, cls, d, m, ns, cells):
        nonlocal i
        long_ls = class_flags(kernel, cls) == (False, "expanded")
        out.append(Case(cid, group, kernel, cls, d, m, ns, cells, seed=i, ls_scale=EXPANDED_ISO_LS if long_ls else 1.0))
        i += 1

    for m in FACTOR_M:
        for ns in FACTOR_NS:
            add(f"F-m{m}-ns{ns}", "factors", "Matern52", "iso", 3, m, ns, 3)
    for kernel in KERNELS:
        for cls in CLASSES:
            add(f"B-{kernel}-{cls}", "build", kernel, cls, 3, 50, 65, 3)
    add("B-d17-ard", "build", "Matern32", "ard", 17, 50, 257, 3)
    add("B-d64-ard", "build", "Matern52", "ard", 64, 50, 130, 3)
    add("B-d64-iso-expanded", "build", "Matern12", "expanded", 64, 50, 130, 3)  # (Matern12's expanded class is the isotropic one)
    for kernel in ROWS_KERNELS:
        for ns in ROWS_NS:
            add(f"R-{kernel}-ns{ns}", "rows", kernel, "iso", 3, 50, ns, 2 if ns == MAX_NS else 3)
    # 8 hyperparameter sets x 3 units at Tp = 320: the first count at which the picker of csrc/potrf.h takes the split panel
    add("C24", "cells24", "Matern32", "iso", 3, 50, 300, 3 * C24_SETS)
    return out


CASES = {c.id: c for c in _table()}
GROUPS = {g: tuple(c.id for c in CASES.values() if c.group == g) for g in ("factors", "build", "rows", "cells24")}
UNFUSED = ("F-m50-ns65", "F-m50-ns130")            # the cases also run with "sgpr_fused" = 0
ROUTE_CASES = ("R-Matern32-ns300", "R-RBF-ns1024")  # the Cholesky-route tests: Tp = 320 and Tp = 1024


def units(cid: str) -> np.ndarray:
    return np.ascontiguousarray([c % N_UNITS for c in range(CASES[cid].cells)], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def hypers(cid: str):
    """(variance, lengthscale(s), noise) of every cell as the case states them: loeo_reference.BASE_HYPERS (ARD: _ARD_LS, repeated along
    the dimensions), the lengthscales multiplied by sqrt(d / 3) (and by the case's ls_scale); set j > 0 of the 24-cell case: the first set's values moved by 5 % a step."""
    c = CASES[cid]
    scale = float(np.sqrt(c.d / 3.0)) * c.ls_scale
    out = []
    for cell in range(c.cells):
        base, j = cell % N_UNITS, cell // N_UNITS
        v, ls, s = lr.BASE_HYPERS[base]
        if c.ard:
            ls = tuple(lr._ARD_LS[base][k % 3] for k in range(c.d))
        grow = 1.0 + 0.05 * j
        ls = tuple(scale * grow * q for q in ls) if c.ard else scale * grow * ls
        out.append((v * grow, ls, s * grow))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def thetas(cid: str) -> np.ndarray:
    """(cells, ntheta) unconstrained hyperparameters on the 2^-30 grid, C order; read-only."""
    out = np.ascontiguousarray(np.stack([theta_of(*h) for h in hypers(cid)]))
    out.setflags(write=False)
    return out


def hyper(cid: str, cell: int):
    """(variance, lengthscales (d of them), noise) the library works with in this cell."""
    v, ls, s = constrain(thetas(cid)[cell])
    return v, np.broadcast_to(ls, (CASES[cid].d,)), s


@functools.lru_cache(maxsize=None)
def _points(d: int, seed: int):
    return tuple(np.rint(a * DATA_GRID) / DATA_GRID for a in make_regression(N_TRAIN, d, n_outputs=N_UNITS, n_test=MAX_NS, config=53, unit=seed))


@functools.lru_cache(maxsize=None)
def data(cid: str):
    """(x (300, d), y (300, 3), zs (cells, m, d), xs (ns, d)), every entry a multiple of 2^-20; read-only.  The inducing inputs of cell c
    are chosen as in loeo_reference.data: m rows of x spread over the data, shifted by (c + 1) / 32 so that none coincides with a
    training row; where m > 300 the rest are rows shifted by (c + 1) / 32 + 1 / 4 (sparse_objective_reference.data).  The event is the
    first ns of 1024 test rows."""
    c = CASES[cid]
    x, y, xs_all = _points(c.d, c.seed)
    rows = np.linspace(0, N_TRAIN - 1, min(c.m, N_TRAIN)).astype(np.int64)
    more = np.linspace(0, N_TRAIN - 1, max(c.m - N_TRAIN, 0)).astype(np.int64)
    zs = []
    for cell in range(c.cells):
        shift = (cell + 1) / 32.0
        zs.append(np.concatenate([x[rows] + shift, x[more] + (shift + 0.25)]))
    zs = np.ascontiguousarray(np.stack(zs))
    xs = np.ascontiguousarray(xs_all[:c.ns])
    for a in (x, y, zs, xs):
        a.setflags(write=False)
    return x, y, zs, xs


# ---- the longdouble definition ------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def joint_parts_ld(kernel, x, y, z, xs, variance, ls, noise, form):
    """(mean, Kss, t1^T t1, t2^T t2, |t1|^T |t1|, |t2|^T |t2|) in longdouble: everything the two include_noise values share."""
    m = z.shape[0]
    s = LD(noise)
    kuu = kmat_form_ld(kernel, z, z, variance, ls, form) + LD(JITTER) * np.eye(m, dtype=LD)
    low = chol_ld(kuu)
    a = solve_lower_ld(low, kmat_form_ld(kernel, z, x, variance, ls, form))
    lb = chol_ld(np.eye(m, dtype=LD) + (a @ a.T) / s)
    c = solve_lower_ld(lb, a @ np.asarray(y).astype(LD)) / s
    t1 = solve_lower_ld(low, kmat_form_ld(kernel, z, xs, variance, ls, form))
    t2 = solve_lower_ld(lb, t1)
    a1, a2 = np.abs(t1), np.abs(t2)
    return t2.T @ c, kmat_form_ld(kernel, xs, xs, variance, ls, form), t1.T @ t1, t2.T @ t2, a1.T @ a1, a2.T @ a2


def joint_from_parts(parts, variance, noise, include_noise):
    """(mean, C, Lref, S) from joint_parts_ld's tuple."""
    mean, kss, q1, q2, s1, s2 = parts
    add = LD(noise) if include_noise else LD(JITTER) * LD(variance)
    eye = np.eye(kss.shape[0], dtype=LD)
    cov = kss - q1 + q2 + add * eye
    return mean, cov, chol_ld(cov), np.abs(kss) + s1 + s2 + add * eye


@functools.lru_cache(maxsize=None)
def _parts(cid: str, cell: int):
    c = CASES[cid]
    x, y, zs, xs = data(cid)
    v, ls, s = hyper(cid, cell)
    return _frozen(*joint_parts_ld(c.kernel, x, y[:, units(cid)[cell]], zs[cell], xs, v, ls, s, c.form))


@functools.lru_cache(maxsize=None)
def joint_ld(cid: str, cell: int, include_noise):
    """(mean (ns,), C (ns, ns), Lref (ns, ns), S (ns, ns)) of one cell in longdouble; read-only."""
    v, _, s = hyper(cid, cell)
    return _frozen(*joint_from_parts(_parts(cid, cell), v, s, bool(include_noise)))


# ---- error measures -----------------------------------------------------------------------------------------------------------------
def llt_ld(lc) -> np.ndarray:
    """The lower triangle of Lc Lc^T in longdouble from the lower triangle of a float64 factor (zeros above the diagonal)."""
    low = np.tril(np.asarray(lc)).astype(LD)
    n = low.shape[0]
    out = np.zeros((n, n), LD)
    for i0 in range(0, n, NB):
        i1 = min(n, i0 + NB)
        out[i0:i1, :i1] = low[i0:i1, :i1] @ low[:i1, :i1].T
    return np.tril(out)


def cov_err(lc, cov, scale) -> float:
    """max_ij |Lc Lc^T - C|_ij / S_ij (both sides symmetric: taken over i >= j)."""
    sel = np.tril(np.ones(cov.shape, bool))
    return float(np.max(np.abs(llt_ld(lc) - cov)[sel] / scale[sel]))


def factor_err(lc, cov, lref) -> float:
    """max_{i >= j} |Lc_ij - Lref_ij| / sqrt(C_ii)"""
    diff = np.abs(np.tril(np.asarray(lc)).astype(LD) - lref)
    return float(np.max(diff / np.sqrt(np.diag(cov))[:, None]))


def errors(mean, lc, cid, cell, include_noise) -> dict:
    """{"mean", "cov", "factor"}: the three measures of one cell's result; lc: the leading (ns, ns) block of the returned factor."""
    ref_mean, cov, lref, scale = joint_ld(cid, cell, bool(include_noise))
    return {"mean": mean_err(mean, ref_mean), "cov": cov_err(lc, cov, scale), "factor": factor_err(lc, cov, lref)}


# ---- float64 restatement of predict_joint_batch ---------------------------------------------------------------------------------------
def hyper64(cid: str, cell: int, seed):
    """sparse_objective_reference.hyper64 on this module's cases: the first perturbation seed moves every constrained hyperparameter one
    ulp up, the second one ulp down, the third each its own way (csrc/px_math.h's softplus may leave a neighbour)."""
    v, ls, s = constrain(thetas(cid)[cell])
    if seed is not None:
        j = PERTURB_SEEDS.index(seed)
        step = (np.ones, lambda k: -np.ones(k))[j](ls.size + 2) if j < 2 else np.random.default_rng([41, seed, cell]).choice([-1.0, 1.0], ls.size + 2)
        u = np.concatenate([[v], ls, [s]])
        u = np.nextafter(u, np.where(step > 0, np.inf, -np.inf))
        v, ls, s = float(u[0]), u[1:-1], float(u[-1])
    return v, np.broadcast_to(ls, (CASES[cid].d,)), s


@functools.lru_cache(maxsize=2)
def _emu_parts(cid: str, cell: int, seed):
    """(mean, Kss (lower triangle valid), t1, t2, variance, noise) of the restatement: what the two include_noise values share."""
    c = CASES[cid]
    x, y, zs, xs = data(cid)
    y, z = y[:, units(cid)[cell]], zs[cell]
    v, ls, s = hyper64(cid, cell, seed)
    n, m, mp = N_TRAIN, c.m, c.mp
    rng = None if seed is None else np.random.default_rng([47, seed, cell])
    kuu = lr.kmat64_form(c.kernel, z, z, v, ls, c.form, rng, symmetric=True)
    if c.form == "difference":
        kuu[np.diag_indices(m)] = v  # (r2 = 0 exactly: g = 1; the expanded form's diagonal comes out of the cancellation)
    q = np.eye(mp)
    q[:m, :m] = kuu + JITTER * np.eye(m)
    p = np.zeros((mp, n))
    p[:m] = lr.kmat64_form(c.kernel, z, x, v, ls, c.form, rng)
    low, inv_l, _ = emu_potrf(q)
    a = emu_trsm(low, inv_l, p)
    inv_s = 1.0 / s
    ssum, usum = np.zeros((mp, mp)), np.zeros(mp)
    for c0 in range(0, n, CHUNK):
        ac = a[:, c0:c0 + CHUNK]
        ssum = ssum + dot64(ac, ac.T)
        usum = usum + dot64(ac, y[c0:c0 + CHUNK])
    b = ssum * inv_s
    b[np.diag_indices(mp)] += 1.0
    lb, inv_lb, crow = emu_potrf(b, extra_rows=(usum * inv_s)[None, :])
    kus = np.zeros((mp, c.ns))
    kus[:m] = lr.kmat64_form(c.kernel, z, xs, v, ls, c.form, rng)
    t1 = emu_trsm(low, inv_l, kus)
    t2 = emu_trsm(lb, inv_lb, t1)
    mean = emu_colreduce(t2, crow[0], CHUNK)
    kss = lr.kmat64_form(c.kernel, xs, xs, v, ls, c.form, rng, symmetric=True)
    if c.form == "difference":
        kss[np.diag_indices(c.ns)] = v
    return mean, kss, t1, t2, v, s


def emu_joint(cid: str, cell: int, include_noise, seed=None):
    """(mean (ns,), Lc (ns, ns)) of the float64 restatement (module docstring); seed None: the longdouble kernel rounded to double."""
    c = CASES[cid]
    mean, kss, t1, t2, v, s = _emu_parts(cid, cell, seed)
    cov = np.eye(c.tp)
    cov[:c.ns, :c.ns] = kss
    cov[np.arange(c.ns), np.arange(c.ns)] += s if include_noise else JITTER * v
    t1p, t2p = np.zeros((c.mp, c.tp)), np.zeros((c.mp, c.tp))
    t1p[:, :c.ns], t2p[:, :c.ns] = t1, t2
    cov = cov - dot64(t1p.T, t1p)
    cov = cov + dot64(t2p.T, t2p)
    low = emu_potrf(cov)[0]
    return mean, low[:c.ns, :c.ns]


# ---- recorded bounds ----------------------------------------------------------------------------------------------------------------
QUANTITIES = ("mean", "cov", "factor")


def key(cid, cell, include_noise, quantity) -> str:
    return f"{cid}/c{cell}/n{int(bool(include_noise))}/{quantity}"


def expected_keys() -> set:
    return {key(cid, cell, nz, q) for cid, c in CASES.items() for cell in range(c.cells) for nz in (0, 1) for q in QUANTITIES}


def case_ratios(cid: str, cells=None) -> dict:
    """The worst error of the restatement over the unperturbed run and the perturbation seeds, never reported below u (neither the
    reference rounded to double nor a result's own last rounding resolves finer)."""
    out = {}
    for cell in (range(CASES[cid].cells) if cells is None else cells):
        for seed in (None,) + PERTURB_SEEDS:
            for nz in (1, 0):
                mean, low = emu_joint(cid, cell, nz, seed)
                for q, val in errors(mean, low, cid, cell, nz).items():
                    k = key(cid, cell, nz, q)
                    out[k] = max(out.get(k, U), val)
    return out


def compute_bounds() -> dict:
    """Every recorded ratio.  Deterministic: the same file bit for bit."""
    out = {}
    for cid in CASES:
        out.update(case_ratios(cid))
        _parts.cache_clear()
        joint_ld.cache_clear()
    return out


def cap_used(cid: str, cell: int, include_noise, recorded_cov: float) -> float:
    """max_ij MARGIN x recorded cov ratio x S_ij / (1e-8 (variance + noise)): at most 1 where the new bound is no looser, element by
    element, than the absolute bound of test_gpu_ensemble.py that it replaces."""
    v, _, s = hyper(cid, cell)
    scale = joint_ld(cid, cell, bool(include_noise))[3]
    return float(MARGIN * recorded_cov * np.max(scale) / (LD(BASELINE_TOL) * (LD(v) + LD(s))))


@functools.lru_cache(maxsize=None)
def bounds() -> dict:
    with open(BOUNDS_PATH) as fh:
        return json.load(fh)


def recorded(cid, cell, include_noise, quantity) -> float:
    """The recorded ratio; a missing entry is a KeyError (a test failure, never a skip)."""
    return bounds()[key(cid, cell, include_noise, quantity)]
