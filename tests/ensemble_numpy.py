"""A numpy mirror of the peak ensemble (gpras_amd.ensemble, csrc/ensemble.h): the joint predictive covariance of a sparse model over one
event's rows and its Cholesky factor, the packing of draws into score rows, the reverse -> depth -> peak chain per member with the
device's operation order (one fused multiply-add per mode, emulated exactly), and the statistics over the members with sums in member
order.  Shared by the CPU pins (test_ensemble.py) and the GPU parity tests (test_gpu_ensemble.py)."""

import numpy as np
from scipy.linalg import solve_triangular

from oracle import kernels as kn
from oracle import sgpr as osg


# ---- an exact fused multiply-add in float64 ---------------------------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a  # 2^27 + 1 (Veltkamp)
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _round_odd_sum(a, b):
    """a + b rounded to odd: the nearest-even sum, moved to the neighbour with an odd last bit when the sum is inexact and it is even."""
    s, e = _two_sum(a, b)
    bits = np.ascontiguousarray(s).view(np.int64).copy()
    need = (e != 0) & ((bits & 1) == 0)
    step = np.where((e > 0) == (s > 0), 1, -1)
    bits = np.where(need, bits + step, bits)
    return bits.view(np.float64)


def fma(a, b, c):
    """round(a * b + c) with ONE rounding, elementwise (Boldo and Melquiond, "Emulation of a FMA and correctly rounded sums", 2008): the
    product and the first sum are split into exact pairs, the two small parts are added with rounding to odd, and the last addition
    rounds once.  Valid away from overflow and underflow, which the tests' magnitudes are."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, uh)
    return th + _round_odd_sum(tl, ul)


# ---- joint prediction --------------------------------------------------------------------------------------------------------------------
def joint_covariance(kernel, X, y, Z, variance, lengthscales, noise, Xs, include_noise=True, jitter=osg.JITTER, form="direct"):
    """``(mean, C)``: the terms of ``oracle.sgpr.predict`` with the diagonal kept joint, ``C = Kss - tmp1^T tmp1 + tmp2^T tmp2`` plus
    ``noise I`` (``include_noise``) or ``jitter variance I`` (without it: what makes the noise-free covariance factorisable)."""
    t = osg.common_terms(kernel, X, y, Z, variance, lengthscales, noise, jitter, form)
    Kus = kn.kmat(kernel, Z, Xs, variance, lengthscales, form)
    tmp1 = solve_triangular(t["L"], Kus, lower=True)
    tmp2 = solve_triangular(t["LB"], tmp1, lower=True)
    mean = tmp2.T @ t["c"]
    C = kn.kmat(kernel, Xs, Xs, variance, lengthscales, form) - tmp1.T @ tmp1 + tmp2.T @ tmp2
    C = C + (noise if include_noise else jitter * variance) * np.eye(Xs.shape[0])
    return mean, C


def padded_cholesky(C, tp):
    """The lower factor of ``C`` in the leading block of a ``(tp, tp)`` identity."""
    out = np.eye(tp)
    n = C.shape[0]
    out[:n, :n] = np.linalg.cholesky(C)
    return out


def pack_scores(mean, Lc, Zn, rows_e):
    """``scores[s, t, k] = mean[k, t] + (Zn[k] Lc[k]^T)[s, t]`` for ``t < rows_e``.  mean (K, rows_e); Lc (K, Tp, Tp); Zn (K, S, Tp)."""
    W = np.einsum("ksj,ktj->kst", Zn, Lc)[:, :, :rows_e]
    return np.ascontiguousarray(np.transpose(mean[:, None, :] + W, (1, 2, 0)))


# ---- reverse -> depth -> peak, per member ----------------------------------------------------------------------------------------------------
def expanded(state):
    """The per-cell parameters on the full cell axis, as ``gprx_pca_create`` lays them out: ``(E (k, cells), w, base, elev)``."""
    dry = state["dry"]
    cells, k = dry.shape[0], state["eofs"].shape[0]
    E = np.zeros((k, cells))
    E[:, ~dry] = state["eofs"]
    w = np.ones(cells)
    if state["weights"] is not None:
        w[~dry] = state["weights"]
    base = np.where(dry, 0.0 if state["hp"] == "depth" else state["elevations"], 0.0)
    base[~dry] = state["input_mean"]
    return E, w, base, state["elevations"]


def member_fields(state, scores):
    """``(S, rows_e, cells)``: every member's field as the metrics would see it, operation by operation as the device forms it."""
    E, w, base, elev = expanded(state)
    m = fma(scores, state["x_std"], state["x_mean"])  # (S, T, K)
    s = np.zeros(scores.shape[:2] + (E.shape[1],))
    for kk in range(E.shape[0]):
        s = fma(m[:, :, kk, None], E[kk][None, None, :], s)
    y = s / w + base
    if state["hp"] != "velocity":
        if state["hp"] == "depth":
            y = y + elev
        y = y - elev
        y = np.where(y < 0.0, 0.0, y)
    return y


def member_peaks(state, scores):
    """``(S, cells)``: the first maximum over an event's rows, a NaN taken as the maximum (``np.argmax``'s rule, metrics.h's)."""
    y = member_fields(state, scores)
    arg = np.argmax(y, axis=1)
    return np.take_along_axis(y, arg[:, None, :], axis=1)[:, 0, :]


# ---- statistics over the members -------------------------------------------------------------------------------------------------------------
def quantile_ranks(quantiles, members):
    """``floor(q (S - 1))``: the rank ``np.quantile(..., method="lower")`` reads."""
    return np.array([int(np.floor(q * (members - 1))) for q in quantiles], dtype=np.int32)


def member_stats(peak, thresholds, ranks, areas=None):
    """The statistics of ``gprx_pca_member_stats_dev``; ``mean`` and ``std`` with the device's member-order loops."""
    S, cells = peak.shape
    thr = np.asarray(thresholds, dtype=np.float64)
    exceed = np.stack([(peak > t).sum(axis=0) for t in thr]).astype(np.int32) if thr.size else np.zeros((0, cells), dtype=np.int32)
    total = np.zeros(cells)
    for s in range(S):
        total = total + peak[s]
    mean = total / S
    dev = np.zeros(cells)
    for s in range(S):
        d = peak[s] - mean
        dev = dev + d * d
    std = np.sqrt(dev / S)
    order = np.sort(peak, axis=0)[np.asarray(ranks, dtype=np.int64)] if len(ranks) else np.zeros((0, cells))
    a = np.ones(cells) if areas is None else np.asarray(areas, dtype=np.float64)
    wet = np.stack([((peak > t) * a).sum(axis=1) for t in thr], axis=1) if thr.size else np.zeros((S, 0))
    return {"exceed": exceed, "mean": mean, "std": std, "order": order, "wet_area": wet}
