"""Numpy restatement of the temporal clipping of gpras/preprocess.py (:89-155: _align_datasets, get_cutoff, _delta_cols_norm) IN THE
DEVICE'S SUMMATION ORDER (gpras_amd/csrc/align.h), operation by operation.  The GPU tests hold the device to it bit for bit; the
fixture (tests/golden/align_ref_golden.npz, the reference's own outputs) records how far its curve is from the reference's.

The order, fixed by the column index c of the side-by-side matrix alone:
  n_c    the difference rows in ascending order (numpy's own order for sum(axis=0) of a C-ordered array);
  r_t    wave strips of W = 64 columns (0.0 beyond the last column) by a balanced tree over adjacent columns, six levels; the four
         wave strips of a strip of S = 256 columns as ((w0 + w1) + w2) + w3; the strips in ascending order;
  total  r_0 + r_1 + ... in ascending order; cum the same way over r_t / total.
"""

import numpy as np

W, S, ROW_TILE, FINISH_CHUNK = 64, 256, 32, 1024  # csrc/align.h: a wave, AL_NT, AL_RT, AL_FC
START_THRESHOLD = 10e-4  # preprocess.py:146


def rows_used(combo) -> int:
    """The rows before the first one that holds a NaN in any column (:138-140)."""
    bad = np.isnan(combo).any(axis=1)
    return int(np.argmax(bad)) if bad.any() else combo.shape[0]


def normalisers(a):
    """n_c of the (T', C) block a, zeros as 1 (:151-153)."""
    acc = np.zeros(a.shape[1])
    for t in range(a.shape[0] - 1):
        acc = acc + np.abs(a[t + 1] - a[t])
    acc[acc == 0.0] = 1.0
    return acc


def row_sums(a, n):
    """r_t = sum_c |a[t+1, c] - a[t, c]| / n_c in the device's order."""
    nd, C = a.shape[0] - 1, a.shape[1]
    strips = -(-C // S)
    q = np.zeros((nd, strips * S))
    q[:, :C] = np.abs(np.diff(a, axis=0)) / n
    v = q.reshape(nd, strips * (S // W), W)
    while v.shape[2] > 1:  # adjacent pairs, six levels
        v = v[:, :, 0::2] + v[:, :, 1::2]
    w = v.reshape(nd, strips, S // W)
    s = w[:, :, 0]
    for i in range(1, S // W):
        s = s + w[:, :, i]
    r = s[:, 0].copy()
    for i in range(1, strips):
        r = r + s[:, i]
    return r


def curve(combo):
    """(cum (T' - 1,), T'): cumsum of the normalised row sums of the trimmed block (:138-143)."""
    combo = np.asarray(combo, dtype=np.float64)
    tp = rows_used(combo)
    if tp < 2:
        raise ValueError("fewer than 2 rows are left after the NaN trim")  # the reference: argmax of an empty sequence
    a = combo[:tp]
    with np.errstate(invalid="ignore", divide="ignore"):
        r = row_sums(a, normalisers(a))
        total = 0.0
        for t in range(tp - 1):
            total = total + r[t]
        u = r / total
        cum = np.empty(tp - 1)
        acc = 0.0
        for t in range(tp - 1):
            acc = acc + u[t]
            cum[t] = acc
    return cum, tp


def cutoff_of_curve(cum, threshold):
    """(start, stop) with numpy's argmax semantics: the first crossing, 0 when there is none (:145-146)."""
    with np.errstate(invalid="ignore"):
        return int(np.argmax(cum > START_THRESHOLD)), int(np.argmax(cum > threshold))


def get_cutoff(combo, threshold=0.95):
    return cutoff_of_curve(curve(combo)[0], threshold)


def align(plan_data, threshold=0.95, cutoffs=None):
    """_align_datasets (:89-116) on arrays: plan_data an iterable of (plan, hf (T, n_hf), lf (T, n_lf)); a plan already in `cutoffs`
    keeps its entry.  Returns (hf_aligned, lf_aligned, runs, t, cutoffs)."""
    cutoffs = dict(cutoffs or {})
    hf_store, lf_store, runs, ts = [], [], [], []
    for plan, hf, lf in plan_data:
        if plan not in cutoffs:
            cutoffs[plan] = get_cutoff(np.concatenate([hf, lf], axis=1), threshold)
        start, stop = cutoffs[plan]
        hf_store.append(hf[start:stop])
        lf_store.append(lf[start:stop])
        dur = max(len(hf[start:stop]), 0)
        runs += [plan] * dur
        ts.append(np.arange(0, dur))
    return np.concatenate(hf_store), np.concatenate(lf_store), np.array(runs), np.concatenate(ts), cutoffs
