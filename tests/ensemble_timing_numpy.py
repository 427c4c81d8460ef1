"""A numpy mirror of the event timing of a peak ensemble (gpras_amd.ensemble.member_timing_dev / timing_stats, csrc/timing.h): per member
and cell the row of the peak, and per threshold the rows above it and the first of them, from the fields ``ensemble_numpy.member_fields``
forms bit for bit as the device does; and the statistics over the members with plain integer numpy.  Shared by the CPU pins
(test_ensemble_timing.py) and the GPU parity tests (test_gpu_ensemble_timing.py)."""

import numpy as np

import ensemble_numpy as en


def field_timing(y, thr):
    """``(peak (S, cells), timing int32 (S, 1 + 2 n_thr, cells))`` of fields ``y (S, rows, cells)``: map 0 ``np.argmax`` over the rows (the first
    maximum, a NaN taken as the maximum), map ``1 + j`` the count of ``y > thr[j]`` (a NaN is not above anything), map ``1 + n_thr + j`` the
    first such row, ``rows`` where there is none."""
    y = np.asarray(y, dtype=np.float64)
    thr = np.asarray(thr, dtype=np.float64).reshape(-1)
    rows = y.shape[1]
    arg = np.argmax(y, axis=1)
    peak = np.take_along_axis(y, arg[:, None, :], axis=1)[:, 0, :]
    maps = [arg]
    above = [y > t for t in thr]
    maps += [a.sum(axis=1) for a in above]
    maps += [np.where(a.any(axis=1), np.argmax(a, axis=1), rows) for a in above]
    return peak, np.stack(maps, axis=1).astype(np.int32)


def member_timing(state, scores, thr):
    """``(peak, timing)`` of the members' scores ``(S, rows, K)`` through the chain of ``ensemble_numpy.member_fields``."""
    return field_timing(en.member_fields(state, scores), thr)


def timing_stats(v, sentinel=-1, levels=(), ranks=(), obs=None):
    """The statistics of ``gprx_pca_timing_stats_dev`` over the members of integer maps ``v (S, n_sel, cells)``: ``cdf (n_sel, n_lev, cells)``,
    ``n_valid``, ``sum`` (int64) over the members whose value is not ``sentinel``, ``order (n_sel, n_rank, cells)`` = ``np.sort(v, axis=0)[ranks]``,
    and against ``obs (n_sel, cells)`` the counts ``below`` and ``equal``."""
    v = np.asarray(v).astype(np.int64)
    _, n_sel, cells = v.shape
    valid = v != sentinel
    out = {
        "cdf": np.stack([(v <= int(lv)).sum(axis=0) for lv in levels], axis=1).astype(np.int32) if len(levels) else np.zeros((n_sel, 0, cells), dtype=np.int32),
        "n_valid": valid.sum(axis=0).astype(np.int32),
        "sum": np.where(valid, v, 0).sum(axis=0),
        "order": (np.transpose(np.sort(v, axis=0)[np.asarray(ranks, dtype=np.int64)], (1, 0, 2)).astype(np.int32) if len(ranks)
                  else np.zeros((n_sel, 0, cells), dtype=np.int32)),
        "below": None, "equal": None,
    }
    if obs is not None:
        o = np.asarray(obs).astype(np.int64)[None]
        out["below"], out["equal"] = (v < o).sum(axis=0).astype(np.int32), (v == o).sum(axis=0).astype(np.int32)
    return out
