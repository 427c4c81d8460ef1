"""A numpy restatement of the device eigensolver (gpras_amd/csrc/eig_jacobi.h): parallel two-sided
block Jacobi with the same block partition, the same round-robin tournament (a bye per round for an odd block count), the same
inner ordering (eigenvectors of a pair problem by ascending eigenvalue), the same stop rule and sweep cap and the same final
sort and sign rule.  The pair problem is solved by ``numpy.linalg.eigh`` here and by cyclic Jacobi in LDS on the device.
Shared by the CPU tests and the GPU tests, together with the list of test matrices."""

import numpy as np

BLOCK = 32  # EIG_B
MAX_SWEEPS = 30  # EIG_MAX_SWEEPS
EPS = np.finfo(np.float64).eps


def rr_pair(mm, t, k):
    """Pair k (0 <= k < mm / 2) of round t (0 <= t < mm - 1) over mm players, mm even: player mm - 1 stays (eig_rr_pair)."""
    if k == 0:
        a, b = mm - 1, t
    else:
        a, b = (t + k) % (mm - 1), (t - k) % (mm - 1)
    return (a, b) if a < b else (b, a)


def schedule(m):
    """The rounds of one sweep over m blocks: a list of rounds, each a list of pairs (i, j), i < j.  Even m: m - 1 rounds of
    m / 2 pairs; odd m: m rounds of (m - 1) / 2 pairs, the block that would meet player m sitting out."""
    if m < 2:
        return []
    mm = m + (m & 1)
    rounds = []
    for t in range(mm - 1):
        rounds.append([p for p in (rr_pair(mm, t, k) for k in range(mm // 2)) if p[1] < m])
    return rounds


def blocks(n, b=BLOCK):
    return [np.arange(s, min(s + b, n)) for s in range(0, n, b)]


def off_norms(a):
    """(off(A)_F^2 over the strict lower triangle, doubled; sum of the squared diagonal)."""
    low = np.tril(a, -1)
    return 2.0 * np.sum(low * low), np.sum(np.diag(a) ** 2)


def sort_and_sign(lam, v):
    """Ascending eigenvalues (ties by index); every column's entry of largest magnitude (first on ties) made positive."""
    order = np.argsort(lam, kind="stable")
    lam, v = lam[order], v[:, order]
    piv = v[np.argmax(np.abs(v), axis=0), np.arange(v.shape[1])]
    return lam, v * np.where(piv < 0.0, -1.0, 1.0)


class NoConvergence(np.linalg.LinAlgError):
    pass


def eigh_jacobi(g, b=BLOCK, max_sweeps=MAX_SWEEPS):
    """(lam, v, sweeps, off_rel) of the symmetric matrix whose lower triangle is that of g."""
    g = np.asarray(g, dtype=np.float64)
    n = g.shape[0]
    a = np.tril(g) + np.tril(g, -1).T
    v = np.eye(n)
    blk = blocks(n, b)
    m = len(blk)
    sets = [[blk[0]]] if m == 1 else [[np.concatenate([blk[i], blk[j]]) for i, j in rnd] for rnd in schedule(m)]
    fro2 = None
    sweeps = 0
    while True:
        off2, diag2 = off_norms(a)
        if fro2 is None:
            fro2 = off2 + diag2
        off_rel = np.sqrt(off2 / fro2) if fro2 > 0.0 else off2
        if not (np.isfinite(off2) and np.isfinite(fro2)):
            raise NoConvergence("the matrix is not finite")
        if off2 <= (n * EPS) ** 2 * fro2:
            break
        if sweeps == max_sweeps:
            raise NoConvergence(f"no convergence in {max_sweeps} sweeps: off / norm = {off_rel:.3e}")
        for rnd in sets:
            qs = []
            for idx in rnd:  # 1. pair solves: lower triangle of the submatrix, eigenvectors by ascending eigenvalue
                lam, q = np.linalg.eigh(a[np.ix_(idx, idx)], UPLO="L")
                qs.append((idx, lam, q))
            for idx, _, q in qs:  # 2. columns of A and V
                a[:, idx] = a[:, idx] @ q
                v[:, idx] = v[:, idx] @ q
            for idx, lam, q in qs:  # 3. rows; the pair's own block is diag(lam) exactly
                a[idx, :] = q.T @ a[idx, :]
                a[np.ix_(idx, idx)] = np.diag(lam)
        sweeps += 1
    lam, v = sort_and_sign(np.diag(a).copy(), v)
    return lam, v, sweeps, off_rel


# ---- the test matrices ---------------------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 31, 64, 65, 127, 128, 129, 200, 257, 520)
KINDS = ("gram", "diagonal", "repeated", "indefinite", "upper_garbage", "near_diagonal")
DISTINCT = ("gram", "indefinite", "near_diagonal")  # no repeated eigenvalue: eigenvectors comparable with LAPACK's


def _field_rows(rng, n_s, cells):
    """Field-like rows as in test_random_shapes_equal_restatement of tests/test_gpu_pca_fit.py."""
    r = 6
    scales = 3.0 * 0.6 ** np.arange(r)
    return 11.0 + 0.5 * (rng.standard_normal((n_s, r)) * scales) @ rng.standard_normal((r, cells)) + 0.01 * rng.standard_normal((n_s, cells))


def make_matrix(kind, n, seed=0):
    rng = np.random.default_rng(1000 * KINDS.index(kind) + n + seed)
    if kind == "gram":
        x = _field_rows(rng, n, 4 * n + 8)
        x = x - x.mean(axis=0)
        return x @ x.T
    if kind == "diagonal":
        return np.diag(rng.standard_normal(n) * 3.0 + 0.5)
    if kind == "repeated":
        u, w = rng.standard_normal(n), rng.standard_normal(n)
        return 2.5 * np.eye(n) + np.outer(u, u) + np.outer(w, w)
    if kind in ("indefinite", "upper_garbage"):
        rng = np.random.default_rng(1000 * KINDS.index("indefinite") + n + seed)
        s = rng.standard_normal((n, n))
        s = (s + s.T) / 2.0
        if kind == "upper_garbage":
            s = np.tril(s) + np.triu(np.random.default_rng(7).standard_normal((n, n)) * 1e3, 1)
        return s
    if kind == "near_diagonal":
        d = 1.0 + np.arange(n) + rng.random(n) * 0.25
        s = rng.standard_normal((n, n))
        s = (s + s.T) / 2.0
        np.fill_diagonal(s, 0.0)
        return np.diag(d) + 1e-9 * np.sqrt(np.outer(d, d)) * s
    raise ValueError(kind)


def cases():
    return [(kind, n) for kind in KINDS for n in SIZES]


def residual(g, lam, v):
    """||G V - V diag(lam)||_F and ||G||_F, with G the matrix of g's lower triangle."""
    a = np.tril(g) + np.tril(g, -1).T
    return np.linalg.norm(a @ v - v * lam), np.linalg.norm(a)
