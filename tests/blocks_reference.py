"""Plain-numpy references for the block tests (test_gpu_gemm_variants.py, test_gpu_solve_blocks.py): no GPU is imported here.

Everything that serves as a reference is computed in np.longdouble (x87 extended, eps 1.08e-19 -- asserted below); products, the
Cholesky factor, triangular solves and inverses are spelled out so that no double-precision BLAS sits between the data and the
reference.  test_blocks_reference.py checks these against mpmath at 50 digits.

The `emu_*` functions are a float64 restatement of the block algorithms of csrc/solve.h (explicit 64 x 64 inverses of the
diagonal blocks plus products) and of the blocked Cholesky of csrc/potrf.h (emu_potrf: substitution against the diagonal blocks,
whose inverses it also forms).  tests/golden/make_blocks_bounds.py runs them on the matrices named here and records how far
they land from the reference; the GPU tests allow 8 x that.
"""

from __future__ import annotations

import functools
import json
import os

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1.1e-19, "np.longdouble is not the 80-bit extended format here: the references would be no better than the kernels"
U = 2.0 ** -53  # unit roundoff of double
NB = 64
NOISES = (1e-2, 1e-6)
SIZES = (64, 128, 192, 256, 320)
SEEDS = (0, 1, 2)  # one matrix per cell of a batched call
CANARY_BITS = np.uint64(0x7FF8C0DEC0DEC0DE)  # a quiet NaN no arithmetic produces
BOUNDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blocks_bounds.json")


# ---- canaries --------------------------------------------------------------------------------------------------------------
def canary(shape) -> np.ndarray:
    return np.full(shape, CANARY_BITS, dtype=np.uint64).view(np.float64)


def is_canary(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint64) == CANARY_BITS


# ---- products ------------------------------------------------------------------------------------------------------------
def gemm_ref(ta, tb, alpha, a, b, beta, c0):
    """(alpha op(A) op(B) + beta C0, |alpha| |op(A)| |op(B)| + |beta| |C0|), both in longdouble."""
    oa = (a.T if ta else a).astype(LD)
    ob = (b.T if tb else b).astype(LD)
    ref = LD(alpha) * (oa @ ob)
    mag = abs(LD(alpha)) * (np.abs(oa) @ np.abs(ob))
    if beta != 0.0:
        ref = ref + LD(beta) * c0.astype(LD)
        mag = mag + abs(LD(beta)) * np.abs(c0.astype(LD))
    return ref, mag


def gemm_bound(k, mag, nsplit=0):
    """|got - ref| <= 2 (K [+ nsplit] + 2) u (|alpha| |op(A)| |op(B)| + |beta| |C0|): K products and K - 1 additions in any order, the
    scaling by alpha and the update with beta C0 (the + 2), the additions of the split-K slabs; the factor 2 covers the rounding of
    the reference to double and keeps first-order terms honest."""
    return 2.0 * (k + nsplit + 2) * U * mag


def assert_gemm(got, ref, mag, k, where=None, nsplit=0, what=""):
    """got (float64) against the longdouble reference under the derived bound, on the elements `where` selects (default all)."""
    err = np.abs(got.astype(LD) - ref)
    bound = gemm_bound(k, mag, nsplit)
    sel = np.ones(got.shape, bool) if where is None else where
    assert not np.any(np.isnan(got[sel])), f"{what}: {int(np.sum(np.isnan(got[sel])))} elements of the result were never written (NaN)"
    bad = sel & ~(err <= bound)
    if np.any(bad):
        idx = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, LD(1e-300)), 0)), got.shape)
        raise AssertionError(f"{what}: {int(np.sum(bad))} elements outside the bound, worst at {idx}: got {got[idx]!r}, ref {float(ref[idx])!r}, "
                             f"err {float(err[idx]):.3e}, bound {float(bound[idx]):.3e}")


# ---- the matrices of the solve tests ----------------------------------------------------------------------------------------
def chol_ld(a: np.ndarray) -> np.ndarray:
    """Lower Cholesky factor in longdouble (column by column)."""
    a = a.astype(LD)
    n = a.shape[0]
    low = np.zeros((n, n), LD)
    for j in range(n):
        col = a[j:, j] - low[j:, :j] @ low[j, :j]
        d = np.sqrt(col[0])
        low[j, j] = d
        low[j + 1:, j] = col[1:] / d
    return low


def solve_lower_ld(low: np.ndarray, b: np.ndarray, transpose: bool = False) -> np.ndarray:
    """L x = b (or L^T x = b) by substitution in longdouble; b (n,) or (n, m)."""
    low = low.astype(LD)
    x = np.array(b, dtype=LD)
    n = low.shape[0]
    if not transpose:
        for i in range(n):
            x[i] = (x[i] - low[i, :i] @ x[:i]) / low[i, i]
    else:
        for i in range(n - 1, -1, -1):
            x[i] = (x[i] - low[i + 1:, i] @ x[i + 1:]) / low[i, i]
    return x


def inv_lower_ld(low: np.ndarray) -> np.ndarray:
    return solve_lower_ld(low, np.eye(low.shape[0], dtype=LD))


@functools.lru_cache(maxsize=None)
def _rbf(noise: float, seed: int):
    """RBF matrix on max(SIZES) random points in 3-D plus noise on the diagonal.  Read-only."""
    n = max(SIZES)
    x = np.random.default_rng([7, seed]).uniform(0.0, 1.0, (n, 3))
    d = x[:, None, :] - x[None, :, :]
    r2 = d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1] + d[:, :, 2] * d[:, :, 2]
    # (exp in longdouble, rounded: numpy's double exp differs in the last bit between CPU generations, and the recorded bounds must
    # come out the same everywhere)
    k = np.exp((-0.5 * r2 / 0.3 ** 2).astype(LD)).astype(np.float64) + noise * np.eye(n)
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def _factor(noise: float, seed: int):
    """The longdouble Cholesky factor of _rbf(noise, seed), rounded to double.
    The factor of the leading n x n block is the leading block of the factor, so one factorisation serves every size."""
    low = chol_ld(_rbf(noise, seed)).astype(np.float64)
    low.setflags(write=False)
    return low


def potrf_input(n: int, noise: float, seed: int = 0) -> np.ndarray:
    """The matrix whose factor solve_inputs(n, noise, seed) holds: the input of the factorisation tests.  Read-only."""
    return _rbf(noise, seed)[:n, :n]


@functools.lru_cache(maxsize=None)
def solve_inputs(n: int, noise: float, seed: int = 0):
    """(L, inv_diag): L (n, n) float64 lower with zeros above the diagonal, inv_diag (n / 64, 64, 64) the longdouble inverses of its
    diagonal blocks rounded to double.  Built on the host: nothing here depends on the device factorisation.  Read-only."""
    low = _factor(noise, seed)[:n, :n]
    inv = np.stack([inv_lower_ld(low[i:i + NB, i:i + NB]).astype(np.float64) for i in range(0, n, NB)])
    inv.setflags(write=False)
    return low, inv


@functools.lru_cache(maxsize=None)
def inverse_input(n: int, noise: float, seed: int = 0) -> np.ndarray:
    """L^-1 in longdouble, rounded to double: the reference of trtri_lower and the input of alpha_from_inverse.  Read-only."""
    x = inv_lower_ld(solve_inputs(n, noise, seed)[0]).astype(np.float64)
    x.setflags(write=False)
    return x


def rhs(n: int, ncols: int, seed: int) -> np.ndarray:
    """The right-hand side of a solve case: the same numbers in the bounds script and in the GPU test."""
    r = np.random.default_rng([11, n, ncols, seed]).standard_normal((n, max(ncols, 1)))
    return r[:, 0].copy() if ncols == 0 else r  # (ncols == 0: a vector)


def vec(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng([13, n, seed]).standard_normal(n)


# ---- componentwise ratios ----------------------------------------------------------------------------------------------------
def solve_ratio(low, x, b, transpose=False) -> float:
    """max |op(L) X - B| / (n u (|op(L)| |X| + |B|))"""
    lo = (low.T if transpose else low).astype(LD)
    x, b = x.astype(LD), b.astype(LD)
    res = np.abs(lo @ x - b)
    den = low.shape[0] * U * (np.abs(lo) @ np.abs(x) + np.abs(b))
    return float(np.max(res / den))


def inverse_ratio(low, x) -> float:
    """max |X L - I| / (n u (|X| |L| + I)) with X taken as lower triangular"""
    lo, x = low.astype(LD), np.tril(x).astype(LD)
    eye = np.eye(low.shape[0], dtype=LD)
    res = np.abs(x @ lo - eye)
    den = low.shape[0] * U * (np.abs(x) @ np.abs(lo) + eye)
    return float(np.max(res / np.where(den > 0, den, LD(1))))  # (den == 0 only above the diagonal, where the residual is exactly 0)


def factor_ratio(a, low_hat) -> float:
    """max over the lower triangle of |A - L L^T| / (u |L| |L|^T) for a computed factor L (its lower triangle is taken).  Higham,
    Accuracy and Stability, theorem 10.3: at most gamma_{n+1} = (n + 1) u / (1 - (n + 1) u) < (n + 2) u componentwise, whatever
    the order of the sums."""
    lo = np.tril(low_hat).astype(LD)
    res = np.abs(np.asarray(a).astype(LD) - lo @ lo.T)
    mag = np.abs(np.tril(low_hat))
    den = U * dot64(mag, mag.T)  # (a sum of positive terms: float64 in a fixed order is exact enough for a ratio, and three times as fast)
    sel = np.tril(np.ones(lo.shape, bool))
    return float(np.max(res[sel] / np.where(den[sel] > 0, den[sel], U)))  # (den == 0: every term is zero, so must the entry of A be)


def sum_ratio(got, ref, mag) -> float:
    """Relative error of sums: max |got - ref| / (sum of the magnitudes of the terms), never reported below u -- neither the reference
    rounded to double nor the result's own last rounding can be resolved finer than that."""
    got, ref, mag = np.atleast_1d(got).astype(LD), np.atleast_1d(ref).astype(LD), np.atleast_1d(mag).astype(LD)
    return max(float(np.max(np.abs(got - ref) / mag)), U)


def rel_err(got, ref) -> float:
    return float(np.max(np.abs(got.astype(LD) - ref.astype(LD))) / np.max(np.abs(ref.astype(LD))))


# ---- float64 restatement of solve.h ---------------------------------------------------------------------------------------------
def dot64(a, b):
    """a @ b in float64, k ascending, one rounding per product and per addition: the same bits on every machine (a BLAS chooses its
    summation order by CPU)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    b2 = b.reshape(b.shape[0], -1)
    acc = np.zeros((a.shape[0], b2.shape[1]))
    for k in range(a.shape[1]):
        acc += a[:, k, None] * b2[k, None, :]
    return acc.reshape((a.shape[0],) + b.shape[1:])


def log_ld(x):
    """log in longdouble by +, -, *, / alone (the x87 instruction behind logl differs between CPU vendors in the last bits, and a
    recorded ratio must come out the same everywhere): x = 2^k m with sqrt(1/2) <= m < sqrt(2), log m = 2 atanh(t) =
    2 t sum t^2j / (2j + 1) with t = (m - 1) / (m + 1), |t| < 0.172; k ln 2 with ln 2 in two parts."""
    m, k = np.frexp(np.asarray(x, dtype=LD))
    low = m < np.sqrt(LD(0.5))
    m, k = np.where(low, m + m, m), (k - low).astype(LD)
    t = (m - LD(1)) / (m + LD(1))
    t2 = t * t
    s = np.zeros_like(t)
    for j in range(14, -1, -1):  # (0.172^30 / 31 < 1e-24)
        s = LD(1) / LD(2 * j + 1) + t2 * s
    return (LD(2) * t * s + k * LD("1.9082149292705878161442656807550013e-10")) + k * LD(0.6931471803691238)


def sum64(x, axis=0):
    """Sequential float64 sum along an axis (np.sum's pairwise blocking is an implementation detail)."""
    return np.take(np.cumsum(np.asarray(x, np.float64), axis=axis), -1, axis=axis)


def emu_trsv(low, inv, b, transpose):
    nb = low.shape[0] // NB
    x = np.array(b, dtype=np.float64)
    blk = lambda i: slice(NB * i, NB * i + NB)
    if not transpose:
        x[blk(0)] = dot64(inv[0], x[blk(0)])
        for i in range(nb - 1):
            for j in range(i + 1, nb):
                x[blk(j)] -= dot64(low[blk(j), blk(i)], x[blk(i)])
            x[blk(i + 1)] = dot64(inv[i + 1], x[blk(i + 1)])
    else:
        x[blk(nb - 1)] = dot64(inv[nb - 1].T, x[blk(nb - 1)])
        for i in range(nb - 1, 0, -1):
            for j in range(i):
                x[blk(j)] -= dot64(low[blk(i), blk(j)].T, x[blk(i)])
            x[blk(i - 1)] = dot64(inv[i - 1].T, x[blk(i - 1)])
    return x


def emu_trsm(low, inv, b):
    """Recursive halving of trsm_lower_left."""
    n = low.shape[0]
    if n == NB:
        return dot64(inv[0], b)
    n1 = (n // NB // 2) * NB
    x1 = emu_trsm(low[:n1, :n1], inv[: n1 // NB], b[:n1])
    b2 = b[n1:] - dot64(low[n1:, :n1], x1)
    return np.vstack([x1, emu_trsm(low[n1:, n1:], inv[n1 // NB:], b2)])


def emu_trtri(low, inv):
    """Bottom-up doubling of trtri_lower, ragged last pair included."""
    n = low.shape[0]
    x = np.zeros((n, n))
    for i in range(n // NB):
        x[NB * i:NB * i + NB, NB * i:NB * i + NB] = inv[i]
    s = NB
    while s < n:
        full = n // (2 * s)
        rem = n - full * 2 * s
        pairs = [(2 * s * i, s, s) for i in range(full)] + ([(full * 2 * s, s, rem - s)] if rem > s else [])
        for off, n1, n2 in pairs:
            a, m, e = off, off + n1, off + n1 + n2
            t21 = dot64(low[m:e, a:m], x[a:m, a:m])
            x[m:e, a:m] = -dot64(x[m:e, m:e], t21)
        s *= 2
    return x


def emu_potrf(a, extra_rows=None, by_inverse=False):
    """float64 restatement of the blocked factorisation of csrc/potrf.h and csrc/potrf_cell.h: right-looking by 64 columns, the
    diagonal block factored column by column, its inverse formed explicitly by substitution on the identity (what the panel kernel's
    identity rows do), the rows below it (right-hand-side rows included) by substitution against the diagonal block as in
    potrf_panel_kernel and potrf_rows_kernel, the trailing update one product per block column.  by_inverse: the rows below a
    diagonal block (right-hand-side rows included) are products with its explicit inverse instead, as potrf_cell.h forms them.  Only
    substitution has Higham's componentwise bound, which test_blocks_reference.py holds its recorded factor ratios to; the
    product's error grows with the condition of the diagonal block (recorded under potrf_cell/: up to 162 where substitution has 13).  Elementwise
    operations, sqrt, division and dot64 only: the same bits on every machine.
    Returns (L with zeros above the diagonal, inv_diag (n / 64, 64, 64), the solved rows)."""
    n = a.shape[0]
    extra = 0 if extra_rows is None else extra_rows.shape[0]
    w = np.zeros((n + extra, n))
    w[:n] = np.tril(a)
    if extra:
        w[n:] = extra_rows
    inv = np.zeros((n // NB, NB, NB))
    for j0 in range(0, n, NB):
        j1 = j0 + NB
        d = w[j0:j1, j0:j1]
        for k in range(NB):
            d[k, k] = np.sqrt(d[k, k])
            d[k + 1:, k] /= d[k, k]
            d[k + 1:, k + 1:] -= np.tril(np.outer(d[k + 1:, k], d[k + 1:, k]))
        x = inv[j0 // NB]
        for i in range(NB):
            e = np.zeros(NB)
            e[i] = 1.0
            x[i] = ((e - dot64(d[i:i + 1, :i], x[:i])[0]) if i else e) / d[i, i]
        rows = w[j1:, j0:j1]
        if by_inverse and j1 < n + extra:
            rows[...] = dot64(rows, x.T)
        for k in range(NB if j1 < n + extra and not by_inverse else 0):
            if k:
                rows[:, k] -= dot64(rows[:, :k], d[k, :k])
            rows[:, k] /= d[k, k]
        if j1 < n:
            low = w[j1:, j0:j1]
            upd = dot64(low, low[: n - j1].T)
            w[j1:n, j1:] -= np.tril(upd[: n - j1])
            w[n:, j1:] -= upd[n - j1:]
    return w[:n].copy(), inv, w[n:].copy()


POTRF_RHS_ROWS = 128  # the right-hand-side rows of a factorisation case; a test takes the first `extra` of them, a vector the first


def potrf_rhs(n: int, seed: int) -> np.ndarray:
    """(POTRF_RHS_ROWS, n): the rows carried below the matrix of potrf_input(n, ., seed)."""
    return np.ascontiguousarray(rhs(n, POTRF_RHS_ROWS, seed).T)


@functools.lru_cache(maxsize=4)  # (35 MB per matrix at n = 2112)
def exact_factor(n: int, seed: int = 0, nrhs: int = NB):
    """(A, L0, inv_diag, Y, Z): a positive definite matrix that EVERY blocked schedule factors without a rounding error.
    L0 = M diag(d), d_j = 2^e with e in -1 .. 2, M unit lower triangular with integers in -2 .. 2: its 64 x 64 blocks below the
    diagonal sparse (density 0.3), its diagonal blocks I + N with N non-zero only in rows >= 32 and columns < 32 of the block, so
    N^2 = 0 and the inverse of a diagonal block of L0 is diag(1 / d) (I - N) exactly.  A = L0 L0^T, Y = Z L0^T with integer Z in
    -3 .. 3 (nrhs right-hand-side rows; row 0 serves as the vector).  Every pivot is a power of four and every intermediate value
    of any blocked schedule a small multiple of 1/4 (or of 1/16 in an inverse), far below 2^53 of them: L0, the inverses and Z
    must come back bit for bit, under every summation order.  Read-only."""
    rng = np.random.default_rng([23, n, seed])
    m = np.eye(n)
    for bi in range(n // NB):
        for bj in range(bi):
            m[NB * bi:NB * bi + NB, NB * bj:NB * bj + NB] = rng.integers(-2, 3, (NB, NB)) * (rng.random((NB, NB)) < 0.3)
        m[NB * bi + NB // 2:NB * bi + NB, NB * bi:NB * bi + NB // 2] = rng.integers(-2, 3, (NB // 2, NB // 2)) * (rng.random((NB // 2, NB // 2)) < 0.3)
    d = 2.0 ** rng.integers(-1, 3, n)
    low = m * d[None, :]
    inv = np.stack([(2.0 * np.eye(NB) - m[i:i + NB, i:i + NB]) / d[i:i + NB, None] for i in range(0, n, NB)])
    z = rng.integers(-3, 4, (nrhs, n)).astype(np.float64)
    out = (low @ low.T, low, inv, z @ low.T, z)  # (sums of a few thousand multiples of 1/4 below 2^20: exact in any order)
    for v in out:
        v.setflags(write=False)
    return out


def emu_colreduce(m, w, rows_per_chunk):
    """colreduce_partial + the chunk sum of colreduce_final: rows of a chunk alternate between two accumulators."""
    nrows = m.shape[0]
    total = np.zeros(m.shape[1])
    for r0 in range(0, nrows, rows_per_chunk):
        s = [np.zeros(m.shape[1]), np.zeros(m.shape[1])]
        for q, r in enumerate(range(r0, min(nrows, r0 + rows_per_chunk))):
            s[q & 1] = s[q & 1] + (w[r] * m[r] if w is not None else m[r] * m[r])
        total = total + (s[0] + s[1])
    return total


# ---- the cases whose bounds are recorded ----------------------------------------------------------------------------------------------
TRSM_NCOLS = (64, 40, 200)
LOGDET_N = (1, 63, 64, 300)
COLREDUCE_SHAPES = [(nr, nc) for nr in (64, 200) for nc in (1, 37, 130)]
ROWREDUCE_SHAPES = [(nr, nc) for nr in (1, 5, 130) for nc in (2, 64, 190)]
ROWS_PER_CHUNK = 48  # (several chunks, a ragged last one, an odd row count inside it at nrows = 200)


ALPHA_N = (448, 512, 576)  # one chunk of alpha_from_inverse's rows not filled, filled exactly, and two chunks


def alpha_input(n, seed):
    """A lower triangular matrix in the place of L^-1: alpha_from_inverse only forms X^T beta."""
    return np.tril(np.random.default_rng([19, n, seed]).standard_normal((n, n)))


def reduce_matrix(nrows, ncols, seed):
    return np.random.default_rng([17, nrows, ncols, seed]).standard_normal((nrows, ncols))


def tag(noise) -> str:
    return f"noise{noise:.0e}"


def compute_bounds() -> dict:
    """Every recorded ratio, from the float64 emulation against the longdouble reference.  Deterministic: same file bit for bit."""
    out = {}
    for noise in NOISES:
        for seed in SEEDS:
            for n in SIZES:
                low, inv = solve_inputs(n, noise, seed)
                key = f"n{n}/{tag(noise)}/seed{seed}"
                b = rhs(n, 0, seed)
                out[f"trsv_fwd/{key}"] = solve_ratio(low, emu_trsv(low, inv, b, False), b)
                out[f"trsv_bwd/{key}"] = solve_ratio(low, emu_trsv(low, inv, b, True), b, True)
                for ncols in TRSM_NCOLS:
                    bm = rhs(n, ncols, seed)
                    out[f"trsm/c{ncols}/{key}"] = solve_ratio(low, emu_trsm(low, inv, bm), bm)
                x = emu_trtri(low, inv)
                out[f"trtri/{key}"] = inverse_ratio(low, x)
                # the factorisation itself: beta and the inverse blocks against the emulation's OWN factor, as the tests take the device's
                bp = potrf_rhs(n, seed)
                lh, ih, bh = emu_potrf(potrf_input(n, noise, seed), bp)
                out[f"potrf/{key}"] = factor_ratio(potrf_input(n, noise, seed), lh)
                out[f"potrf_beta/{key}"] = solve_ratio(lh, bh.T, bp.T)
                out[f"potrf_inv/{key}"] = max(inverse_ratio(lh[i:i + NB, i:i + NB], ih[i // NB]) for i in range(0, n, NB))
                # the same with the rows as products with the explicit inverses (potrf_cell.h): not within Higham's constant
                out[f"potrf_cell/{key}"] = factor_ratio(potrf_input(n, noise, seed), emu_potrf(potrf_input(n, noise, seed), by_inverse=True)[0])
    for seed in SEEDS:
        for n in ALPHA_N:
            xin, beta = alpha_input(n, seed), vec(n, seed)
            out[f"alpha/n{n}/seed{seed}"] = sum_ratio(dot64(xin.T, beta), xin.astype(LD).T @ beta.astype(LD),
                                                      np.abs(xin).astype(LD).T @ np.abs(beta).astype(LD))
        for n in LOGDET_N:
            low, _ = solve_inputs(max(SIZES), NOISES[0], seed)
            d, v = np.diag(low)[:n], vec(n, seed)
            lg = log_ld(d)  # (each term rounded from longdouble: numpy's double log is not the same on every CPU, nor is its longdouble log)
            out[f"logdet/n{n}/seed{seed}"] = sum_ratio(sum64(lg.astype(np.float64)), np.sum(lg), np.sum(np.abs(lg)))
            out[f"quad/n{n}/seed{seed}"] = sum_ratio(sum64(v * v), np.sum(v.astype(LD) ** 2), np.sum(v.astype(LD) ** 2))
        for nr, nc in COLREDUCE_SHAPES:
            m, w = reduce_matrix(nr, nc, seed), vec(nr, seed)
            ml, wl = m.astype(LD), w.astype(LD)
            out[f"colreduce_w/r{nr}c{nc}/seed{seed}"] = sum_ratio(emu_colreduce(m, w, ROWS_PER_CHUNK), wl @ ml, np.abs(wl) @ np.abs(ml))
            out[f"colreduce_sq/r{nr}c{nc}/seed{seed}"] = sum_ratio(emu_colreduce(m, None, ROWS_PER_CHUNK), np.sum(ml * ml, 0), np.sum(ml * ml, 0))
    for nr, nc in ROWREDUCE_SHAPES:
        m, w = reduce_matrix(nr, nc, 0), vec(nc, 0)
        ml, wl = m.astype(LD), w.astype(LD)
        out[f"rowreduce_w/r{nr}c{nc}"] = sum_ratio(dot64(m, w), ml @ wl, np.abs(ml) @ np.abs(wl))
        out[f"rowreduce_sq/r{nr}c{nc}"] = sum_ratio(sum64(m * m, 1), np.sum(ml * ml, 1), np.sum(ml * ml, 1))
    return out


@functools.lru_cache(maxsize=None)
def bounds() -> dict:
    with open(BOUNDS_PATH) as fh:
        return json.load(fh)


# ---- padded device images ------------------------------------------------------------------------------------------------------------
class Image:
    """A host image of `cells` cells, each holding the named matrices (name -> rows, cols, ld) `batch` times, laid out as the kernels
    address them: leading dimension ld >= cols, `extra_rows` rows of padding below each matrix, a gap after each, every matrix 16-byte
    aligned, cells `cs` doubles apart with a gap of their own.  The whole image starts as `fill`: the canary by default (outputs), a
    plain NaN for the inputs of a product (padding that is read poisons the result).  After the call everything that is not part of a
    specified result -- inputs, padding, gaps -- must hold the bits that were uploaded."""

    def __init__(self, cells=1, batch=1, fill=None, extra_rows=0, gap=6, cell_gap=20, **parts):
        self.cells, self.batch, self.shape, self.extra_rows = cells, batch, parts, extra_rows
        off, self.off, self.stride = 0, {}, {}
        for name, (rows, cols, ld) in parts.items():
            st = (rows + extra_rows) * ld + gap
            st += st & 1  # (strides stay even: every matrix starts 16-byte aligned)
            self.off[name], self.stride[name] = off, st
            off += batch * st
        self.cs = off + cell_gap
        self.cs += self.cs & 1
        self.flat = canary(cells * self.cs) if fill is None else np.full(cells * self.cs, fill, dtype=np.float64)
        self.result = np.zeros(self.flat.size, bool)  # elements of a specified result: the only ones a call may change
        self.dev = None

    def ld(self, name):
        return self.shape[name][2]

    def offset(self, name, c=0, e=0):
        return c * self.cs + self.off[name] + e * self.stride[name]

    def view(self, name, c=0, flat=None, e=0):
        rows, cols, ld = self.shape[name]
        o = self.offset(name, c, e)
        return (self.flat if flat is None else flat)[o:o + rows * ld].reshape(rows, ld)[:, :cols]

    def mark_result(self, name, c=0, e=0, where=None):
        m = self.view(name, c, self.result, e)
        if where is None:
            m[...] = True
        else:
            m[where] = True

    def set_result(self, name, values, c=0, e=0, where=None):
        """Store what a result region holds on entry (all of the matrix, or the elements `where` selects) and mark it as result."""
        v = self.view(name, c, None, e)
        if where is None:
            v[...] = values
        else:
            v[where] = values[where]
        self.mark_result(name, c, e, where)

    def upload(self):
        from gpras_amd._lib import DeviceBuffer  # (ctypes only; nothing touches a device before a test calls this)

        self.dev = DeviceBuffer.from_array(self.flat)
        return self.dev

    def ptr(self, name):
        return self.dev.at(self.off[name])

    def download(self):
        got = self.dev.to_array(self.flat.shape)
        self.dev.free()
        return got

    def assert_unchanged_except(self, got, names, what):
        """Everything but the named matrices and the marked result elements holds the bits that were uploaded."""
        mask = ~self.result
        for name in names:
            for c in range(self.cells):
                for e in range(self.batch):
                    self.view(name, c, mask, e)[...] = False
        same = np.ascontiguousarray(got).view(np.uint64)[mask] == self.flat.view(np.uint64)[mask]
        assert np.all(same), f"{what}: {int(np.sum(~same))} elements outside the result changed (first at flat index " \
                             f"{int(np.flatnonzero(mask)[np.argmin(same)])})"
