"""The numpy mirror of the depth-frequency maps (gpras_amd.frequency, csrc/frequency.h): the accumulation of a
weighted catalogue of peak blocks into exceedance rates per level and the inversion to the depth at a target rate, in numpy's rounded
``/ * + -`` -- one rounding per operation, no fma --, so that the device's numbers can be compared for equality."""

import numpy as np

INTERPS = ("linear", "step")


def accumulate(peaks, weights, levels):
    """``(rate (L, cells) float64, nan_members (cells,) int32)`` after the events ``peaks[e] (S_e, cells)`` with weights ``weights[e]``,
    added in order: per level ``n = #{s: peak[s, c] > d_l}`` (strict; a NaN exceeds nothing), ``t = n / S``, ``u = w t``, ``rate += u``."""
    levels = np.asarray(levels, dtype=np.float64)
    peaks = [np.asarray(p, dtype=np.float64) for p in peaks]
    cells = peaks[0].shape[1]
    rate = np.zeros((levels.size, cells))
    nan_members = np.zeros(cells, dtype=np.int32)
    for peak, w in zip(peaks, weights):
        members = np.float64(peak.shape[0])
        n = np.empty((levels.size, cells), dtype=np.int64)
        with np.errstate(invalid="ignore"):
            for l, d in enumerate(levels):
                n[l] = (peak > d).sum(axis=0)
        t = n.astype(np.float64) / members
        u = np.float64(w) * t
        rate = rate + u
        nan_members = nan_members + np.isnan(peak).sum(axis=0).astype(np.int32)
    return rate, nan_members


def invert(rate, nan_members, levels, aep, interp="linear"):
    """``(depth (n_aep, cells) float64, bracket (n_aep, cells) int32)``: per target ``p`` and cell ``k = #{l: rate[l, c] >= p}``; depth ``-inf``
    where ``k = 0``, ``+inf`` where ``k = L``, else ``d_{k-1}`` (step) or ``d_{k-1} + (d_k - d_{k-1}) ((r_{k-1} - p) / (r_{k-1} - r_k))`` (linear);
    a cell with ``nan_members > 0``: depth NaN, bracket -1."""
    if interp not in INTERPS:
        raise ValueError(f"interp must be one of {INTERPS}")
    rate = np.asarray(rate, dtype=np.float64)
    levels = np.asarray(levels, dtype=np.float64)
    p = np.atleast_1d(np.asarray(aep, dtype=np.float64))
    n_lev, cells = rate.shape
    k = np.zeros((p.size, cells), dtype=np.int32)
    for l in range(n_lev):
        k += rate[l][None, :] >= p[:, None]
    lo, hi = np.clip(k - 1, 0, n_lev - 1), np.clip(k, 0, n_lev - 1)
    cols = np.arange(cells)[None, :]
    r_lo, r_hi = rate[lo, cols], rate[hi, cols]
    d_lo, d_hi = levels[lo], levels[hi]
    if interp == "step":
        depth = d_lo.copy()
    else:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            a = r_lo - p[:, None]
            b = r_lo - r_hi
            f = a / b
            g = d_hi - d_lo
            depth = d_lo + g * f
    depth = np.where(k == 0, -np.inf, np.where(k == n_lev, np.inf, depth))
    flagged = np.asarray(nan_members)[None, :] > 0
    return np.where(flagged, np.nan, depth), np.where(flagged, np.int32(-1), k).astype(np.int32)
