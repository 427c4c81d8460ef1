"""Numpy restatement of the k-means++ seeding (``sklearn.cluster._kmeans._kmeans_plusplus``, behind ``gpr.py:313``) FOR GIVEN
DRAWS, with the margins that say how far an input is from an outcome decided by rounding.  The GPU tests
(test_gpu_kmeans_kernels.py) hold ``gprx_kmeans_pp`` (csrc/kmeans.h: kpp_dist_kernel, kpp_select_kernel) to the picked rows;
test_kmeans.py pins this restatement to scikit-learn's own ``kmeans_plusplus`` on the ``RandomState(0)`` draws.

The arithmetic is scikit-learn's: distances in the expanded form ``max(-2 x.c + |c|^2 + |x|^2, 0)`` on
``row_norms(xc, squared=True)``, the search ``searchsorted(cumsum(closest), u * closest.sum())`` clipped to n - 1, the candidate
with the smallest potential (first on ties).  The device differs from it in summation order and fused multiply-add only: a few
n 2^-53 relative to the potential.  An index can differ only where a margin is of that size:

  gap_search     min over the draws with 0 < u < 1 of |cumsum[i] - v| / potential over all i (a draw of exactly 0.0 gives
                 row 0 -- every cumulative sum is >= 0 -- and a draw >= 1.0 gives row n - 1 after the clip: exact, left out);
  gap_potential  min over the centres of (second-best - best potential) / best potential among candidates that are different
                 rows (centres whose best potential is 0 are skipped).
"""

import numpy as np
from sklearn.utils.extmath import row_norms


def distances(xc, xsq, rows):
    """(len(rows), n) squared distances of every point to the given rows, expanded form (sklearn's _euclidean_distances)."""
    d2 = -2.0 * (xc[rows] @ xc.T)
    d2 += xsq[rows][:, None]
    d2 += xsq[None, :]
    np.maximum(d2, 0.0, out=d2)
    return d2


def kmeans_pp_replay(xc, m, trials, first_id, uniforms):
    """Rows picked by ``_kmeans_plusplus`` on the centred data xc (n, d) when its random stream gives `first_id` and then
    `uniforms[c - 1]` (trials values) for centre c.  `uniforms` may be None when m == 1.
    Returns (indices (m,) int64, gap_search, gap_potential); a margin nothing contributed to is inf."""
    xc = np.ascontiguousarray(xc, dtype=np.float64)
    n = xc.shape[0]
    xsq = row_norms(xc, squared=True)
    indices = np.empty(m, dtype=np.int64)
    indices[0] = first_id
    closest = distances(xc, xsq, np.array([first_id]))[0]
    gap_search = gap_potential = np.inf
    for c in range(1, m):
        u = np.asarray(uniforms[c - 1], dtype=np.float64)[:trials]
        pot = closest.sum()
        v = u * pot
        cum = np.cumsum(closest)
        cand = np.searchsorted(cum, v)
        np.clip(cand, None, n - 1, out=cand)
        if pot > 0.0:
            for t in np.flatnonzero((u > 0.0) & (u < 1.0)):
                gap_search = min(gap_search, float(np.min(np.abs(cum - v[t])) / pot))
        to_cand = np.minimum(closest, distances(xc, xsq, cand))
        pots = (to_cand @ np.ones((n, 1)))[:, 0]  # (scikit-learn's own product: where two potentials tie mathematically, its last bit)
        same = np.all(xc[cand] == xc[cand[int(np.argmin(pots))]], axis=1)
        best = int(np.argmax(same))  # (copies of a row have one potential: the first of them, whatever a matrix product's last bit says)
        others = pots[~same]
        if others.size and pots[best] > 0.0:
            gap_potential = min(gap_potential, float((others.min() - pots[best]) / pots[best]))
        closest = to_cand[best]
        indices[c] = cand[best]
    return indices, gap_search, gap_potential
