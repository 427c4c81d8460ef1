"""numpy restatement of the pseudo-surface kernels (gpras_amd/csrc/pseudo.h), operation by operation: the cubic B-spline in the
order of FITPACK's fpbspl / splev, the masked column median as a sort and a pick, and the floored surface.  The CPU tests pin it
to the fixture recorded from the reference (tests/golden/pseudo_ref_golden.npz); the GPU tests hold the device to both."""

import numpy as np


def spline_eval(knots, coef, x):
    """s(x) for FITPACK's knot vector (boundary knots repeated four times) and coefficients; any shape of x.  The interval is the
    largest l in [3, n - 5] with t[l] <= x (l = 3 when there is none), so arguments outside the knots extrapolate the end pieces."""
    t = np.asarray(knots, dtype=np.float64)
    c = np.asarray(coef, dtype=np.float64)
    xv = np.asarray(x, dtype=np.float64)
    flat = xv.reshape(-1)
    n = len(t)
    l = np.clip(np.searchsorted(t, flat, side="right") - 1, 3, n - 5)
    l = np.where(np.isnan(flat), 3, l)
    h = [np.ones_like(flat), np.zeros_like(flat), np.zeros_like(flat), np.zeros_like(flat)]
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(1, 4):
            hh = [h[i].copy() for i in range(j)]
            h[0] = np.zeros_like(flat)
            for i in range(1, j + 1):
                tli, tlj = t[l + i], t[l + i - j]
                same = tli == tlj
                f = hh[i - 1] / np.where(same, 1.0, tli - tlj)
                h[i - 1] = np.where(same, h[i - 1], h[i - 1] + f * (tli - flat))
                h[i] = np.where(same, 0.0, f * (flat - tlj))
        sp = np.zeros_like(flat)
        for j in range(4):
            sp = sp + c[l - 3 + j] * h[j]
    return sp.reshape(xv.shape)


def fit_centerline(us_wse, ds_wse, us_q, ds_q, centerline_wse):
    """Column medians of (us - wse) / (us - ds) over the rows with a positive flow: sort, pick the middle one or (a + b) / 2 of
    the middle two; a NaN anywhere in a column gives NaN (np.sort puts NaN last, so the pick sees it only through the flag)."""
    us, ds = np.ravel(us_wse), np.ravel(ds_wse)
    keep = (np.ravel(us_q) > 0) | (np.ravel(ds_q) > 0)
    if not keep.any():
        raise ValueError("no row has a positive upstream or downstream flow")
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = (us[keep, None] - np.asarray(centerline_wse)[keep]) / (us[keep] - ds[keep])[:, None]
    s = np.sort(ratio, axis=0)
    n = s.shape[0]
    with np.errstate(invalid="ignore"):
        med = s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0
    return np.where(np.isnan(ratio).any(axis=0), np.nan, med)


def interpolate_centerline(us_wse, ds_wse, w):
    us, ds = np.ravel(us_wse)[:, None], np.ravel(ds_wse)[:, None]
    return us - (us - ds) * np.asarray(w)[None, :]


def surface(us_wse, ds_wse, w, idx, elev, fluvial=None):
    full = interpolate_centerline(us_wse, ds_wse, w)[:, np.asarray(idx)]
    full = np.maximum(full, np.asarray(elev)[None, :])
    return full if fluvial is None else np.maximum(full, fluvial)
