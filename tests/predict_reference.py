"""Plain-numpy references for the prediction-route tests (test_gpu_predict_routes.py): no GPU is imported here.

The reference of a prediction is predict_ld: kernel matrix, Cholesky factor, the two solves for alpha, mean = Ks^T alpha and
var = v - colsum((L^-1 Ks)^2) [+ s], all in np.longdouble with no BLAS in between (blocks_reference.py: chol_ld, solve_lower_ld).
test_predict_reference.py checks it against mpmath at 50 digits.

emu_predict_inverse / emu_predict_substitution restate the two device routes of csrc/gp_predict.h in float64: a right-looking
Cholesky on 64-wide blocks with explicit inverses of the diagonal blocks, then either L^-1 by emu_trtri, Vt = Kst L^-T and row sums of
squares, or emu_trsm and column sums in chunks of 256 rows.  Their kernel entries are the longdouble kernel rounded to double (so that
no host libm decides a recorded number), perturbed by what the device's kernel build is allowed: r2 (1 + d1), |d1| <= 4u, and
g (1 + d2), |d2| <= 2u.  tests/golden/make_predict_bounds.py records how far they land from predict_ld on the cases named here
(the maximum over the unperturbed run and three perturbation seeds); the GPU tests allow 8 x that.

Hyperparameters: the C ABI takes unconstrained values and applies softplus itself.  A case states the constrained values; theta is
their inverse softplus rounded to a multiple of 2^-30, and every reference works with the longdouble softplus of THAT theta rounded to
double -- what the library computes from it, to the last bit or one beside it.

The recorded numbers must come out the same on every host, and a ratio moves in its fourth digit when the reference moves in its
last longdouble bit.  So nothing that is recorded passes through a libm: exp and log1p are spelled out here in longdouble additions,
multiplications and divisions (the x87 transcendental instructions behind expl / logl differ between CPU vendors in the last bits),
and the data of make_regression -- a float64 sine and a BLAS product -- are rounded to multiples of 2^-20 before use.
"""

from __future__ import annotations

import functools
import json
import os
from typing import NamedTuple

import numpy as np

import blocks_reference as br
from blocks_reference import LD, NB, U, chol_ld, dot64, emu_colreduce, emu_trsm, emu_trsv, emu_trtri, solve_lower_ld, sum64
from gpras_amd.synth import make_regression

KERNEL_IDS = {"RBF": 0, "Matern12": 1, "Matern32": 2, "Matern52": 3, "Exponential": 4}
R2_FLOOR = LD("1e-36")
NOISE_LOWER = 1e-6
ROWS_PER_CHUNK = 256  # predict_dev's column reduce
DATA_GRID = 2.0 ** 20
PERTURB_SEEDS = (0, 1, 2)
MARGIN = 8.0
BASELINE_TOL = 1e-8
BOUNDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_bounds.json")
ROUTES = {1: "inverse", 2: "substitution"}


# ---- longdouble kernel and prediction ----------------------------------------------------------------------------------------
def r2_ld(a, b, lengthscales):
    """Scaled squared distance in the difference form, longdouble."""
    a, b = np.asarray(a).astype(LD), np.asarray(b).astype(LD)
    ls = np.broadcast_to(np.asarray(lengthscales).astype(LD), (a.shape[1],))
    out = np.zeros((a.shape[0], b.shape[0]), LD)
    for k in range(a.shape[1]):
        diff = (a[:, k][:, None] - b[:, k][None, :]) / ls[k]
        out += diff * diff
    return out


LN2_HI = LD(0.6931471803691238)  # 33 significant bits: k LN2_HI is exact for |k| < 2^31
LN2_LO = LD("1.9082149292705878161442656807550013e-10")
EXP_TERMS, LOG1P_TERMS = 19, 24


def exp_ld(x):
    """exp in longdouble by +, -, *, / alone: x = k ln 2 + r with |r| <= 0.35, the Taylor series of exp(r) to r^19 / 19! < 1e-25 by
    Horner, scaled by 2^k.  A few longdouble ulp."""
    x = np.asarray(x, dtype=LD)
    k = np.rint(x / (LN2_HI + LN2_LO))
    r = (x - k * LN2_HI) - k * LN2_LO
    p = np.ones_like(r)
    for j in range(EXP_TERMS, 0, -1):
        p = LD(1) + r * p / LD(j)
    return np.ldexp(p, k.astype(np.int64))


def log1p_ld(z):
    """log(1 + z) for 0 <= z <= 1 the same way: 2 atanh(t) = 2 t sum t^2k / (2k + 1) with t = z / (2 + z) <= 1/3."""
    z = np.asarray(z, dtype=LD)
    t = z / (LD(2) + z)
    t2 = t * t
    s = np.zeros_like(t)
    for j in range(LOG1P_TERMS, -1, -1):
        s = LD(1) / LD(2 * j + 1) + t2 * s
    return LD(2) * t * s


def g_ld(kernel, r2):
    """The correlation as a function of the scaled squared distance (oracle/kernels.py g_of_r2), longdouble throughout."""
    if kernel == "RBF":
        return exp_ld(LD(-0.5) * r2)
    r = np.sqrt(np.maximum(r2, R2_FLOOR))
    sqrt3, sqrt5, five_thirds = np.sqrt(LD(3)), np.sqrt(LD(5)), LD(5) / LD(3)
    if kernel == "Matern12":
        return exp_ld(-r)
    if kernel == "Matern32":
        return (LD(1) + sqrt3 * r) * exp_ld(-sqrt3 * r)
    if kernel == "Matern52":
        return (LD(1) + sqrt5 * r + five_thirds * r * r) * exp_ld(-sqrt5 * r)
    if kernel == "Exponential":
        return exp_ld(LD(-0.5) * r)
    raise KeyError(kernel)


def kmat_ld(kernel, a, b, variance, lengthscales):
    return LD(variance) * g_ld(kernel, r2_ld(a, b, lengthscales))


def predict_ld(kernel, x, y, variance, lengthscales, noise, xs, include_noise=True):
    """(mean, var) of the exact model, longdouble."""
    k = kmat_ld(kernel, x, x, variance, lengthscales)
    k[np.diag_indices_from(k)] += LD(noise)
    low = chol_ld(k)
    alpha = solve_lower_ld(low, solve_lower_ld(low, np.asarray(y).astype(LD)), transpose=True)
    ks = kmat_ld(kernel, x, xs, variance, lengthscales)
    mean = np.sum(ks * alpha[:, None], axis=0)
    v = solve_lower_ld(low, ks)
    var = LD(variance) - np.sum(v * v, axis=0)
    return mean, (var + LD(noise) if include_noise else var)


# ---- hyperparameters as the C ABI sees them -------------------------------------------------------------------------------------
def softplus_ld(w):
    w = np.asarray(w).astype(LD)
    return np.maximum(w, 0) + log1p_ld(exp_ld(-np.abs(w)))


THETA_GRID = 2.0 ** 30


def theta_of(variance, lengthscales, noise) -> np.ndarray:
    """The unconstrained vector (variance, lengthscales..., noise) handed to the library: the inverse softplus on a grid of 2^-30 (the
    host's log and expm1 decide nothing but which grid point, and no value here sits within 1e-16 of the middle between two)."""
    u = np.concatenate([[variance], np.atleast_1d(lengthscales), [noise - NOISE_LOWER]]).astype(LD)
    w = u + np.log(-np.expm1(-u))
    return np.ascontiguousarray((np.rint(w * LD(THETA_GRID)) / LD(THETA_GRID)).astype(np.float64))


def constrain(theta):
    """(variance, lengthscales (array), noise) that softplus gives back from theta."""
    sp = softplus_ld(theta).astype(np.float64)
    return float(sp[0]), sp[1:-1].copy(), float(NOISE_LOWER + sp[-1])


# ---- the cases -------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    """One data set (n, d, n_units outputs, ns test points, seeded through make_regression) and the cells predicted on it."""
    id: str
    kernel: str
    ard: bool
    n: int
    d: int
    ns: int
    units: tuple          # unit of each cell
    hypers: tuple         # (variance, lengthscale(s), noise) of each cell, constrained
    seed: int
    n_units: int = 2
    duplicate_rows: bool = False
    routes: tuple = ("inverse",)
    alpha_from_inverse: bool = False  # the evaluation with a gradient forms alpha = L^-T beta as X^T beta from the explicit inverse


def _single(cid, kernel, ard, n, d, ns, variance, ls, noise, seed, **kw):
    return Case(cid, kernel, ard, n, d, ns, (0,), ((variance, ls, noise),), seed, routes=("inverse", "substitution"), **kw)


_S1 = (1.0, 0.8, 0.1)
SINGLE = (
    _single("S1", "RBF", False, 64, 1, 1, *_S1, seed=1),
    _single("S2", "Matern52", True, 65, 3, 63, 1.3, tuple(np.linspace(0.7, 1.4, 3)), 0.07, seed=2),
    _single("S3", "Matern12", False, 130, 2, 65, 0.7, 0.5, 1e-3, seed=3),
    _single("S4", "RBF", False, 256, 3, 130, 2.0, 1.5, 1e-4, seed=4),
    _single("S5", "Matern32", True, 300, 5, 200, 1.2, tuple(np.linspace(0.6, 1.2, 5)), 0.03, seed=5),
    _single("S6", "Exponential", False, 70, 65, 65, 1.0, 6.0, 0.1, seed=6),
    _single("S7", "RBF", False, 64, 1, 32768 + 65, *_S1, seed=1),
)
# the state test: S3's data under two more hyperparameter vectors (the second one reached through an evaluation with a gradient)
STATE = (
    _single("S3b", "Matern12", False, 130, 2, 65, 1.1, 0.8, 0.02, seed=3),
    _single("S3c", "Matern12", False, 130, 2, 65, 0.9, 0.65, 0.005, seed=3, alpha_from_inverse=True),
)
B4_CELLS = 33
BATCH = (
    Case("B1", "Matern52", True, 130, 3, 65, (0, 1, 1, 2, 0),
         tuple((1.0 + 0.2 * c, tuple(np.linspace(0.7, 1.4, 3) * (1.0 + 0.1 * c)), 0.04 * (c + 1)) for c in range(5)), seed=11, n_units=3,
         routes=("inverse", "substitution")),
    *(Case(f"B2-{k}", k, False, 64, 2, 1, (0, 1), ((1.0, 0.8, 0.1), (1.4, 1.1, 0.05)), seed=12) for k in KERNEL_IDS),
    Case("B3", "RBF", False, 64, 1, 8192 + 65, (0, 1), ((1.0, 0.8, 0.1), (1.5, 0.6, 0.05)), seed=13),
    Case("B4", "RBF", False, 128, 3, 65, tuple(c % 3 for c in range(B4_CELLS)),
         tuple((1.0 + 0.02 * c, 0.9 + 0.01 * c, 0.05 + 0.002 * c) for c in range(B4_CELLS)), seed=14, n_units=3),
    Case("B5", "Exponential", False, 70, 65, 65, (0, 1), ((1.0, 6.0, 0.1), (1.3, 5.0, 0.06)), seed=6),
    Case("B6", "RBF", False, 128, 3, 20, (0, 1, 0, 1), tuple((1.0 + 0.1 * c, 0.9 + 0.05 * c, 0.1 + 0.02 * c) for c in range(4)), seed=16,
         duplicate_rows=True),
)
CASES = {c.id: c for c in SINGLE + STATE + BATCH}


@functools.lru_cache(maxsize=None)
def data(cid: str):
    """(x, y, xs) of a case: x (n, d), y (n, n_units), xs (ns, d), every entry a multiple of 2^-20; read-only."""
    c = CASES[cid]
    x, y, xs = (np.rint(a * DATA_GRID) / DATA_GRID for a in make_regression(c.n, c.d, n_outputs=c.n_units, n_test=c.ns, config=41, unit=c.seed))
    if c.duplicate_rows:
        x[1::2] = x[0::2]
    for a in (x, y, xs):
        a.setflags(write=False)
    return x, y, xs


def thetas(cid: str) -> np.ndarray:
    """(cells, ntheta) unconstrained hyperparameters of a case, C order."""
    return np.ascontiguousarray(np.stack([theta_of(*h) for h in CASES[cid].hypers]))


def hyper(cid: str, cell: int = 0):
    """(variance, lengthscales, noise) the library works with in this cell."""
    return constrain(thetas(cid)[cell])


@functools.lru_cache(maxsize=None)
def reference(cid: str, cell: int = 0):
    """(mean, var_y) of one cell in longdouble; var_f = var_y - noise is not stored.  Read-only."""
    c = CASES[cid]
    x, y, xs = data(cid)
    v, ls, s = hyper(cid, cell)
    mean, var = predict_ld(c.kernel, x, y[:, c.units[cell]], v, ls, s, xs, True)
    mean.setflags(write=False)
    var.setflags(write=False)
    return mean, var


# ---- error measures ---------------------------------------------------------------------------------------------------------------
def mean_err(got, ref) -> float:
    """max |m - ref| / max |ref|"""
    return float(np.max(np.abs(np.asarray(got).astype(LD) - ref)) / np.max(np.abs(ref)))


def var_err(got, ref) -> float:
    """max (|v - ref| / ref), on the variance with the noise term"""
    return float(np.max(np.abs(np.asarray(got).astype(LD) - ref) / ref))


# ---- float64 restatement of the two routes ----------------------------------------------------------------------------------------
def kmat64(kernel, a, b, variance, lengthscales, rng=None, symmetric=False):
    """The longdouble kernel rounded to double; with rng, r2 and g carry the relative errors the device's kernel build is allowed."""
    r2 = r2_ld(a, b, lengthscales)

    def factor(width):
        e = rng.uniform(-width * U, width * U, r2.shape)
        if symmetric:
            e = np.tril(e) + np.tril(e, -1).T
        return LD(1) + e.astype(LD)

    if rng is not None:
        r2 = r2 * factor(4)
    g = g_ld(kernel, r2)
    if rng is not None:
        g = g * factor(2)
    return (LD(variance) * g).astype(np.float64)


def chol64(a):
    """Unblocked lower Cholesky factor of one diagonal block, float64, every sum sequential."""
    n = a.shape[0]
    low = np.zeros((n, n))
    for j in range(n):
        col = a[j:, j] - (sum64(low[j:, :j] * low[j, :j][None, :], axis=1) if j else 0.0)
        if not col[0] > 0.0:
            raise np.linalg.LinAlgError(f"pivot {j + 1}")
        d = np.sqrt(col[0])
        low[j, j] = d
        low[j + 1:, j] = col[1:] / d
    return low


def inv_lower64(low):
    """Inverse of one lower triangular diagonal block by substitution, float64."""
    n = low.shape[0]
    x = np.zeros((n, n))
    for i in range(n):
        row = -dot64(low[i:i + 1, :i], x[:i, :])[0] if i else np.zeros(n)
        row[i] += 1.0
        x[i, :] = row / low[i, i]
    return x


def emu_chol(a):
    """Right-looking Cholesky on 64-wide block columns, plainly written: factor the diagonal block, invert it, multiply the panel
    below by the inverse, subtract the panel's outer product from everything to its right.  Returns (L, inverses of the diagonal
    blocks) as solve.h's drivers take them."""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    nb = n // NB
    low, inv = np.zeros((n, n)), np.zeros((nb, NB, NB))
    for j in range(nb):
        cur, rest = slice(NB * j, NB * j + NB), slice(NB * j + NB, n)
        low[cur, cur] = chol64(a[cur, cur])
        inv[j] = inv_lower64(low[cur, cur])
        if j + 1 < nb:
            low[rest, cur] = dot64(a[rest, cur], inv[j].T)
            a[rest, rest] -= dot64(low[rest, cur], low[rest, cur].T)
    return low, inv


@functools.lru_cache(maxsize=8)
def _emu_model(cid: str, cell: int, seed):
    """What both routes start from: the padded factor, the block inverses, beta = L^-1 y, alpha, Ks (np, ns) and the hyperparameters.
    Padding as on the device: a unit diagonal below row n of K, zeros in y and in the rows of Ks."""
    c = CASES[cid]
    x, y, xs = data(cid)
    v, ls, s = hyper(cid, cell)
    rng = None if seed is None else np.random.default_rng([23, seed])
    n, npad = c.n, -(-c.n // NB) * NB
    k = np.eye(npad)
    k[:n, :n] = kmat64(c.kernel, x, x, v, ls, rng, symmetric=True)
    k[np.arange(n), np.arange(n)] = v + s
    low, inv = emu_chol(k)
    yp = np.zeros(npad)
    yp[:n] = y[:, c.units[cell]]
    beta = emu_trsv(low, inv, yp, False)
    alpha = emu_trsv(low, inv, beta, True)
    ks = np.zeros((npad, c.ns))
    ks[:n] = kmat64(c.kernel, x, xs, v, ls, rng)
    return low, inv, beta, alpha, ks, v, s


def emu_predict_inverse(cid, cell=0, seed=None, include_noise=True, alpha_from_inverse=False):
    """exact_predict_inverse: L^-1 by trtri_lower, mean = Kst alpha (row dots), Vt = Kst L^-T, var = base - row sums of Vt^2."""
    low, inv, beta, alpha, ks, v, s = _emu_model(cid, cell, seed)
    xinv = emu_trtri(low, inv)
    if alpha_from_inverse:
        alpha = dot64(xinv.T, beta)
    kst = np.ascontiguousarray(ks.T)
    mean = dot64(kst, alpha)
    vt = dot64(kst, xinv.T)
    base = v + (s if include_noise else 0.0)
    return mean, base - sum64(vt * vt, axis=1)


def emu_predict_substitution(cid, cell=0, seed=None, include_noise=True):
    """The substitution loop of predict_dev: column sums in chunks of 256 rows for mean = Ks^T alpha, V = L^-1 Ks by trsm_lower_left,
    var = base - the same column sums of V^2."""
    low, inv, _, alpha, ks, v, s = _emu_model(cid, cell, seed)
    mean = emu_colreduce(ks, alpha, ROWS_PER_CHUNK)
    vmat = emu_trsm(low, inv, ks)
    base = v + (s if include_noise else 0.0)
    return mean, base - emu_colreduce(vmat, None, ROWS_PER_CHUNK)


def case_ratios(cid: str) -> dict:
    """{"<id>/c<cell>/<route>/<mean|var>": ratio}: the worst error of the restatement over the unperturbed run and the perturbation
    seeds, never reported below u (neither the reference rounded to double nor a result's own last rounding resolves finer)."""
    c = CASES[cid]
    out = {}
    for cell in range(len(c.units)):
        ref_mean, ref_var = reference(cid, cell)
        worst = {(r, q): U for r in c.routes for q in ("mean", "var")}
        for seed in (None,) + PERTURB_SEEDS:
            runs = []
            if "inverse" in c.routes:
                runs.append(("inverse", emu_predict_inverse(cid, cell, seed)))
                if c.alpha_from_inverse:
                    runs.append(("inverse", emu_predict_inverse(cid, cell, seed, alpha_from_inverse=True)))
            if "substitution" in c.routes:
                runs.append(("substitution", emu_predict_substitution(cid, cell, seed)))
            for route, (mean, var) in runs:
                worst[route, "mean"] = max(worst[route, "mean"], mean_err(mean, ref_mean))
                worst[route, "var"] = max(worst[route, "var"], var_err(var, ref_var))
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


canary, is_canary = br.canary, br.is_canary
