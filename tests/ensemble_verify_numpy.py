"""A numpy mirror of the ensemble verification (gpras_amd.ensemble.verify_peaks, csrc/verify.h): the members of every cell sorted, then a
Python loop over the ranks on whole rows -- the device's walk, operation for operation: per rank a rounded subtraction, a rounded product
and a rounded addition, in rank order.

The sort is ``np.sort(axis=0)`` on the order-preserving 64-bit keys of csrc/ensemble.h (``ens_key``) and not on the doubles: the two orders
are the same (ascending values, NaN last) except that ``np.sort`` leaves the order of -0 and +0 open, where the keys put -0 first; the
order statistics are compared bit for bit, so the mirror takes the order that is defined."""

import numpy as np

SIGN = np.uint64(1) << np.uint64(63)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def ens_key(x):
    """``ens_key`` of csrc/ensemble.h: ascending keys are ascending values, -0 before +0, every NaN the largest key."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    u = x.view(np.uint64)
    key = np.where(u >> np.uint64(63) != 0, ~u, u | SIGN)
    return np.where(np.isnan(x), ALL, key)


def ens_unkey(key):
    key = np.ascontiguousarray(key, dtype=np.uint64)
    u = np.where(key >> np.uint64(63) != 0, key & ~SIGN, ~key)
    return np.ascontiguousarray(u).view(np.float64)


def sorted_members(peak):
    """``(S, cells)``: every column in key order."""
    return ens_unkey(np.sort(ens_key(peak), axis=0))


def verify_peaks(peak, obs, ranks=()):
    """``crps``, ``below``, ``equal`` ``(cells,)`` and ``order (n_rank, cells)`` of ``peak (S, cells)`` against ``obs (cells,)``."""
    peak, y = np.asarray(peak, dtype=np.float64), np.asarray(obs, dtype=np.float64)
    S, cells = peak.shape
    xs = sorted_members(peak)
    acc = np.zeros(cells)
    below, equal = np.zeros(cells, dtype=np.int32), np.zeros(cells, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for i in range(S):
            x = xs[i]
            w = np.where(x > y, (S - i) - 0.5, i + 0.5)
            t = np.abs(x - y) * w
            acc = acc + t
            below += x < y
            equal += x == y
        crps = (2.0 * acc) / (float(S) * float(S))
    bad = np.isnan(y) | np.isnan(peak).any(axis=0)
    crps[bad] = np.nan
    below[bad] = -1
    equal[bad] = -1
    order = xs[np.asarray(ranks, dtype=np.int64)] if len(ranks) else np.zeros((0, cells))
    return {"crps": crps, "below": below, "equal": equal, "order": order}


def crps_definition(members, y):
    """The CRPS of the empirical distribution of one cell by its definition, ``mean |x - y| - 1/2 mean |x - x'|``, in longdouble."""
    x = np.asarray(members, dtype=np.longdouble)
    y = np.longdouble(y)
    return np.mean(np.abs(x - y)) - np.mean(np.abs(x[:, None] - x[None, :])) / 2
