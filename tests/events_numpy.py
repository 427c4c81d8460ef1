"""Numpy restatement of the device path of gpras_amd/events.py (csrc/events.h), stage by stage: no pandas,
the incremental greedy loop with the lowest row on ties, and the device's summation orders for the column means and scales (chunks of
256 rows summed in row order, then the chunk sums in chunk order) and for the squared distances (the columns in order)."""

import numpy as np

SUM_CHUNK = 256  # csrc/events.h: EV_SUM_CHUNK


# ---- stage 0: the host sort -----------------------------------------------------------------------------------------------------------
def rank_and_hour(event_id, datetime):
    """(ids, rank, hour): sorted unique ids, each row's event rank and its position inside its event (rows in their original order)."""
    event_id, datetime = np.asarray(event_id), np.asarray(datetime)
    order = np.lexsort((datetime, event_id))
    ids, rank_sorted = np.unique(event_id[order], return_inverse=True)
    starts = np.searchsorted(rank_sorted, np.arange(ids.size))
    rank, hour = np.empty(order.size, dtype=np.int64), np.empty(order.size, dtype=np.int64)
    rank[order] = rank_sorted
    hour[order] = np.arange(order.size) - starts[rank_sorted]
    return ids, rank, hour


# ---- stages 1 and 2 ---------------------------------------------------------------------------------------------------------------------
def pivot(rank, hour, values, n_events, n_hours):
    out = np.zeros((n_events, n_hours))
    out[rank, hour] = values
    return out


def event_maxima(rank, values, n_events):
    """The maximum over each event's own rows: the zero fill of the pivot does not enter."""
    out = np.full(n_events, -np.inf)
    np.maximum.at(out, rank, values)
    return out


# ---- stage 3 ------------------------------------------------------------------------------------------------------------------------------
def knots(maxima, arrival_rate):
    """(x, y): ascending distinct block maxima and (n_blocks + 1) / rank of the first descending occurrence of each."""
    maxima = np.asarray(maxima, dtype=np.float64)
    blocks = np.array([maxima[i : i + arrival_rate].max() for i in range(0, maxima.size, arrival_rate)]) + 0.0
    asc = np.sort(blocks)
    nb = asc.size
    last = np.ones(nb, dtype=bool)
    last[:-1] = asc[1:] != asc[:-1]
    i = np.flatnonzero(last)
    if i.size < 2:
        raise ValueError("at least two distinct block maxima are needed")
    return asc[i], np.float64(nb + 1) / (nb - i).astype(np.float64)


def rp_eval(x, y, v):
    """scipy.interpolate.interp1d._call_linear, one rounding per operation."""
    v = np.asarray(v, dtype=np.float64)
    idx = np.clip(np.searchsorted(x, v), 1, x.size - 1)
    lo, hi = idx - 1, idx
    with np.errstate(all="ignore"):
        slope = (y[hi] - y[lo]) / (x[hi] - x[lo])
        return slope * (v - x[lo]) + y[lo]


# ---- stage 4 ------------------------------------------------------------------------------------------------------------------------------
def column_sums(x):
    """Column sums in the device's order: rows in order inside chunks of 256, then the chunks in order."""
    n, m = x.shape
    chunks = -(-n // SUM_CHUNK)
    padded = np.zeros((chunks * SUM_CHUNK, m))
    padded[:n] = x
    padded = padded.reshape(chunks, SUM_CHUNK, m)
    lens = np.minimum(SUM_CHUNK, n - SUM_CHUNK * np.arange(chunks))
    part = np.zeros((chunks, m))
    for r in range(SUM_CHUNK):
        live = lens > r  # (a padded row must not even add +0.0: -0.0 + 0.0 changes the sign of a zero)
        part[live] = part[live] + padded[live, r]
    acc = np.zeros(m)
    for c in range(chunks):
        acc = acc + part[c]
    return acc


def column_means(x):
    return column_sums(x) / np.float64(x.shape[0])


def column_scales(x, mean):
    d = x - mean
    s = np.sqrt(column_sums(d * d) / np.float64(x.shape[0]))
    return np.where(s == 0.0, 1.0, s)


def sign_convention(components):
    pos = np.argmax(np.abs(components), axis=1)
    return components * np.sign(components[np.arange(components.shape[0]), pos])[:, None]


def pca_scores(x, k):
    """(scores (E, k), components (k, H), eigenvalues of the covariance, descending)."""
    xc = x - column_means(x)
    lam, v = np.linalg.eigh(xc.T @ xc / (x.shape[0] - 1))
    top = np.argsort(lam, kind="stable")[::-1]
    comps = sign_convention(v[:, top[:k]].T)
    return xc @ comps.T, comps, lam[top]


def standardise(s):
    mean = column_means(s)
    return (s - mean) / column_scales(s, mean)


def diverse_scores(p_excess, p_inflow, k):
    return standardise(np.concatenate([pca_scores(p_excess, k)[0], pca_scores(p_inflow, k)[0]], axis=1))


# ---- stage 5 ------------------------------------------------------------------------------------------------------------------------------
def sqdist(s, w):
    """Squared distances of every row of s to w: direct differences, the columns summed in order."""
    acc = np.zeros(s.shape[0])
    for j in range(s.shape[1]):
        t = s[:, j] - w[j]
        acc = acc + t * t
    return acc


def farthest(s, selected, num, margins=False):
    """(picks, distances[, relative margin of each pick over the runner-up]): incremental farthest-point selection."""
    s = np.asarray(s, dtype=np.float64)
    n = s.shape[0]
    mind = np.full(n, np.inf)
    is_sel = np.zeros(n, dtype=bool)
    is_sel[np.asarray(selected)] = True
    for r in np.flatnonzero(is_sel):
        mind = np.minimum(mind, sqdist(s, s[r]))
    mind[is_sel] = -1.0
    picks, dist, margin = [], [], []
    for _ in range(num):
        w = int(np.argmax(mind))  # (the first, i.e. lowest, row of the maximum)
        picks.append(w)
        dist.append(np.sqrt(mind[w]))
        if margins:
            rest = np.delete(mind, w)
            margin.append((mind[w] - rest.max()) / mind[w] if rest.size and rest.max() >= 0 else np.inf)
        mind = np.where(mind < 0.0, mind, np.minimum(mind, sqdist(s, s[w])))
        mind[w] = -1.0
    out = (np.array(picks, dtype=np.int64), np.array(dist))
    return out + (np.array(margin),) if margins else out
