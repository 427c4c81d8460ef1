"""numpy restatement of the diagnostics kernels (gpras_amd/csrc/diag.h): what the reference's plotting functions compute
(gpras/utils/plotting.py: performance_cdf :201-233, performance_scatterplot :155-198, map_detection_categories :716-859), with the
one floating-point sum (the sum of squares behind the rmse) taken in the DEVICE's order.  The sort needs no restatement: the sorted
sequence of a multiset is unique, np.sort is the reference.
"""

import numpy as np

SUM_PT, NT, WAVE = 32, 256, 64
SUM_CHUNK = SUM_PT * NT  # csrc/diag.h: DG_SUM_CHUNK
CATEGORY_NAMES = ("", "Detected", "Miss", "False Alarm", "Correct Negative")


def sum_depth(n):
    """D(n): the additions on the longest path of the tree below (csrc/diag.h: dg_sum_depth)."""
    chunks = -(-int(n) // SUM_CHUNK)
    return SUM_PT + 6 + 3 + -(-chunks // NT) + 6 + 3


def _workgroup_sum(rows):
    """rows (k, m, 256): thread t adds rows[k, 0, t], rows[k, 1, t], ... to 0.0; the 64 lanes of a wave by a balanced tree over adjacent
    lanes; the four waves as ((w0 + w1) + w2) + w3.  -> (k,)"""
    acc = np.zeros((rows.shape[0], NT))
    for j in range(rows.shape[1]):
        acc = acc + rows[:, j, :]
    w = acc.reshape(-1, NT // WAVE, WAVE)
    while w.shape[-1] > 1:
        w = w[..., 0::2] + w[..., 1::2]
    w = w[..., 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def sum_sq(p, hf):
    """sum (p - hf)^2 in the order of dg_summary_kernel / dg_summary_final_kernel.  (A slot past the end holds +0.0 here and is skipped on the
    device: adding +0.0 to a sum that is never -0.0 changes nothing.)"""
    p, hf = np.asarray(p, dtype=np.float64).ravel(), np.asarray(hf, dtype=np.float64).ravel()
    r = p - hf
    q = r * r
    chunks = -(-q.size // SUM_CHUNK)
    padded = np.zeros(chunks * SUM_CHUNK)
    padded[: q.size] = q
    part = _workgroup_sum(padded.reshape(chunks, SUM_PT, NT))
    m = -(-chunks // NT)
    padded = np.zeros(m * NT)
    padded[:chunks] = part
    return float(_workgroup_sum(padded.reshape(1, m, NT))[0])


def scatter_summary(p, hf):
    """ll, ur (plotting.py:183) and rmse (plotting.py:185) with the device's sum."""
    p, hf = np.asarray(p, dtype=np.float64).ravel(), np.asarray(hf, dtype=np.float64).ravel()
    s = sum_sq(p, hf)
    return {"ll": float(min(p.min(), hf.min())), "ur": float(max(p.max(), hf.max())), "rmse": float((np.float64(s) / np.float64(p.size)) ** 0.5),
            "sum_sq": s, "n": int(p.size)}


def sorted_abs_residual(a, b):
    return np.sort(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).flatten())


def event_max(field, lo, hi):
    """DataFrame.max(axis=0) of rows [lo, hi): the maximum ignoring NaN, NaN for an all-NaN column."""
    part = np.asarray(field, dtype=np.float64)[lo:hi]
    allnan = np.all(np.isnan(part), axis=0)
    out = np.max(np.where(np.isnan(part), -np.inf, part), axis=0)
    out[allnan] = np.nan
    return out


def detection_codes(y_true, y_pred, events, wet_threshold_depth=0.0, include_correct_negative=False):
    """(E, cells) uint8 codes of plotting.py:765-802 in input column order; ValueError as plotting.py:776-777."""
    codes = np.zeros((len(events), np.shape(y_true)[1]), dtype=np.uint8)
    for e, (lo, hi) in enumerate(events):
        t, p = event_max(y_true, lo, hi), event_max(y_pred, lo, hi)
        if (t < 0).any() or (p < 0).any():
            raise ValueError(f"y_true and y_pred must be non-negative. (event {e!r})")
        t[t < wet_threshold_depth] = 0
        p[p < wet_threshold_depth] = 0
        codes[e][(t > 0) & (p > 0)] = 1
        codes[e][(t > 0) & (p == 0)] = 2
        codes[e][(t == 0) & (p > 0)] = 3
        if include_correct_negative:
            codes[e][(t == 0) & (p == 0)] = 4
    return codes
