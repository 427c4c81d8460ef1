"""Leave-one-event-out (LOEO) predictions of a fitted ``GPRAS``: for every training event, ``predict`` at the event's rows of the model
built on all OTHER rows -- the held-out score of every training storm from one fit, where ``production/analysis/cross_validation.py``
scores one fixed split per pipeline run.

The hyperparameters and the inducing points stay the fitted ones: nothing is re-optimised per fold.  The numbers answer "how well does
this configuration predict a storm it has not seen, given these hyperparameters"; a full cross-validation, which also refits the
hyperparameters without the storm, is a different (and 35 times more expensive) quantity: ``gpras_amd.crossval.cross_validate``
(``GPRAS.cross_validate``) computes that one, with the folds as cells of one batched fit.

Three routes give the same quantity:

``"downdate"``  sparse models with M <= 64, d <= 64 and events of at most 4096 rows: one factorisation per mode, then one 64 x 64 Cholesky
                per (mode, event) on the device (``Engine.loeo_batch``, ``gprx_loeo_batch``).
``"refactor"``  the definition on existing calls: per event an ``Engine`` on the remaining rows and ``predict_batch`` at the event's rows.
                Serves every model (M > 64, d > 64, exact models, longer events).
``"blocked"``   sparse models with M <= 320, d <= 64 and events of at most 4096 rows: the same downdate with the M x M factor of every
                (mode, event) in a workspace in device memory -- kernels of its own around the library's batched Cholesky and
                triangular inverse (``Engine.loeo_batch_blocked``, ``gprx_loeo_batch_blocked``).  Opt-in.

``"auto"`` takes the downdate where it applies and the refactor route elsewhere; it never chooses ``"blocked"``.
"""

from __future__ import annotations

import numpy as np

from .diagnostics import check_ranges

DOWNDATE_MAX_M = 64
DOWNDATE_MAX_D = 64
DOWNDATE_MAX_ROWS = 4096  # rows of one event: a tile of the sparse predict
BLOCKED_MAX_M = 320
ROUTES = ("auto", "downdate", "refactor", "blocked")


def check_event_ranges(ranges, rows: int):
    """``check_ranges`` plus what leaving events out needs: the ranges in ascending order and disjoint.  Two int64 arrays."""
    lo, hi = check_ranges(ranges, rows)
    for e in range(1, lo.size):
        if lo[e] < hi[e - 1]:
            raise ValueError(f"event {e}: ranges must be sorted and disjoint, got ({lo[e]}, {hi[e]}) after ({lo[e - 1]}, {hi[e - 1]})")
    return lo, hi


def label_ranges(labels):
    """``[(lo, hi)]`` of one label per row whose equal labels are contiguous runs of rows (the rule of ``diagnostics.event_ranges``), in
    row order."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.size == 0:
        raise ValueError("labels must be one value per row")
    cuts = np.flatnonzero(labels[1:] != labels[:-1]) + 1
    starts = np.concatenate([[0], cuts])
    ends = np.concatenate([cuts, [labels.size]])
    seen = set()
    for lo in starts:
        key = labels[lo].item() if hasattr(labels[lo], "item") else labels[lo]
        if key in seen:
            raise ValueError(f"the rows of event {key!r} are not contiguous (sort the rows by event first)")
        seen.add(key)
    return [(int(lo), int(hi)) for lo, hi in zip(starts, ends)]


def resolve_events(events, rows: int):
    """``events`` as sorted, disjoint row ranges (two int64 arrays): a list of ``(lo, hi)``, one label per row, or a pandas index whose
    first level is the event."""
    if hasattr(events, "get_level_values"):
        events = np.asarray(events.get_level_values(0))
    arr = events if isinstance(events, np.ndarray) else None
    if arr is None:
        events = list(events)
        if not events:
            raise ValueError("no events")
        first = events[0]
        is_pair = isinstance(first, (tuple, list, np.ndarray)) and len(first) == 2
        arr = None if is_pair else np.asarray(events)
    elif arr.ndim == 2 and arr.shape[1] == 2:
        events, arr = [tuple(r) for r in arr], None
    if arr is not None:
        if arr.ndim != 1 or arr.shape[0] != rows:
            raise ValueError(f"labels: need one per row ({rows}), got shape {arr.shape}")
        events = label_ranges(arr)
    return check_event_ranges(events, rows)


def downdate_applies(gpr, lo, hi) -> str | None:
    """None when the downdate kernel takes this model and these events, else the reason it does not."""
    if not gpr.models:
        return "the model is not fitted"
    if any(m.Z is None for m in gpr.models):
        return "exact model (n_inducing=None)"
    if max(np.shape(m.Z)[0] for m in gpr.models) > DOWNDATE_MAX_M:
        return f"more than {DOWNDATE_MAX_M} inducing points"
    if gpr.x.shape[1] > DOWNDATE_MAX_D:
        return f"more than {DOWNDATE_MAX_D} features"
    if int((hi - lo).max()) > DOWNDATE_MAX_ROWS:
        return f"an event of more than {DOWNDATE_MAX_ROWS} rows"
    if not all(hasattr(m.backend, "loeo_batch") for m in gpr.models):
        return "the backend has no loeo_batch"
    return None


def blocked_applies(gpr, lo, hi) -> str | None:
    """None when the blocked downdate takes this model and these events, else the reason it does not."""
    if not gpr.models:
        return "the model is not fitted"
    if any(m.Z is None for m in gpr.models):
        return "exact model (n_inducing=None)"
    if max(np.shape(m.Z)[0] for m in gpr.models) > BLOCKED_MAX_M:
        return f"more than {BLOCKED_MAX_M} inducing points"
    if gpr.x.shape[1] > DOWNDATE_MAX_D:
        return f"more than {DOWNDATE_MAX_D} features"
    if int((hi - lo).max()) > DOWNDATE_MAX_ROWS:
        return f"an event of more than {DOWNDATE_MAX_ROWS} rows"
    if not all(hasattr(m.backend, "loeo_batch_blocked") for m in gpr.models):
        return "the backend has no loeo_batch_blocked"
    return None


def _by_engine(gpr):
    groups: dict[int, list[int]] = {}
    for i, m in enumerate(gpr.models):
        groups.setdefault(id(m.backend), []).append(i)
    return groups.values()


def _downdate(gpr, lo, hi, include_noise, call="loeo_batch"):
    n, k = gpr.x.shape[0], len(gpr.models)
    mean, var = np.full((n, k), np.nan), np.full((n, k), np.nan)
    ranges = list(zip(lo.tolist(), hi.tolist()))
    for idx in _by_engine(gpr):
        eng = gpr.models[idx[0]].backend
        chunk = max(1, min(64, eng.max_cells(want_grad=False))) if hasattr(eng, "max_cells") else len(idx)
        for c0 in range(0, len(idx), chunk):
            part = idx[c0 : c0 + chunk]
            units = [gpr.models[i].unit for i in part]
            thetas = np.stack([gpr.models[i].theta() for i in part])
            zs = np.stack([gpr.models[i].Z for i in part])
            mu, vv, status = getattr(eng, call)(units, thetas, zs, ranges, include_noise=include_noise)
            if status.any():
                cell, ev = np.argwhere(status)[0]
                raise np.linalg.LinAlgError(f"mode {part[cell]}, event {ev}: the downdated factor is not positive definite")
            mean[:, part], var[:, part] = mu.T, vv.T
    return mean, var


def _blocked(gpr, lo, hi, include_noise):
    """``_downdate`` through ``Engine.loeo_batch_blocked``: the same chunks of modes, the same error."""
    return _downdate(gpr, lo, hi, include_noise, call="loeo_batch_blocked")


def _refactor(gpr, lo, hi, include_noise):
    from .engine import Engine

    x, y = gpr.x, gpr.y
    n, k = x.shape[0], len(gpr.models)
    mean, var = np.full((n, k), np.nan), np.full((n, k), np.nan)
    sparse = gpr.models[0].Z is not None
    m = np.shape(gpr.models[0].Z)[0] if sparse else 0
    units = [mod.unit for mod in gpr.models]
    thetas = np.stack([mod.theta() for mod in gpr.models])
    zs = np.stack([mod.Z for mod in gpr.models]) if sparse else None
    for a, b in zip(lo.tolist(), hi.tolist()):
        keep = np.r_[0:a, b:n]
        if keep.size == 0:
            raise ValueError("an event covers every row: nothing is left to predict from")
        eng = Engine(gpr.kernel_str, x[keep], y[keep], m, ard=gpr.ard, device=gpr.device, distance_form=gpr.distance_form)
        try:
            chunk = max(1, min(64, eng.max_cells(want_grad=False)))
            for c0 in range(0, k, chunk):
                sl = slice(c0, c0 + chunk)
                mu, vv = eng.predict_batch(units[sl], thetas[sl], x[a:b], zs=None if zs is None else zs[sl], include_noise=include_noise)
                mean[a:b, sl], var[a:b, sl] = mu.T, vv.T
        finally:
            eng.close()
    return mean, var


def leave_event_out(gpr, events, route: str = "auto", include_noise: bool = True):
    """``(mean, var)``, each ``(N, K)`` as ``gpr.predict(gpr.x)`` returns them: at the rows of every event the prediction of the model on
    all other rows, at the fitted hyperparameters and inducing points (NOT re-optimised per fold); NaN at rows of no event.  ``events``:
    a list of ``(lo, hi)`` row ranges, one label per row, or a pandas index whose first level is the event.  Every argument is checked
    before the first library call; ``gpr.last_loeo_route`` names the route that ran.  ``route``: ``"auto"`` (the downdate where it
    applies, else the refactor route), ``"downdate"``, ``"refactor"`` or ``"blocked"`` (M <= 320, opt-in); a named route that does not
    apply is a ``ValueError``."""
    if route not in ROUTES:
        raise ValueError(f"route must be one of {ROUTES}, got {route!r}")
    if gpr.x is None or not gpr.models:
        raise ValueError("leave_event_out needs a fitted model")
    lo, hi = resolve_events(events, gpr.x.shape[0])
    if route == "blocked":
        why_not = blocked_applies(gpr, lo, hi)
        if why_not is not None:
            raise ValueError(f"route='blocked' does not apply: {why_not}")
        use = "blocked"
    else:
        why_not = downdate_applies(gpr, lo, hi)
        if route == "downdate" and why_not is not None:
            raise ValueError(f"route='downdate' does not apply: {why_not}")
        use = "downdate" if (route != "refactor" and why_not is None) else "refactor"
    out = {"downdate": _downdate, "blocked": _blocked, "refactor": _refactor}[use](gpr, lo, hi, include_noise)
    gpr.last_loeo_route = use
    return out


def event_scores(y, mean, var, ranges):
    """``(rmse, nlpd)``, each ``(events, K)``: per event and mode the root mean square error and the mean negative log predictive density
    ``0.5 log(2 pi var) + 0.5 (y - mean)^2 / var`` over the event's rows (host arithmetic on the small results)."""
    y, mean, var = (np.asarray(a, dtype=np.float64) for a in (y, mean, var))
    if y.ndim != 2 or mean.shape != y.shape or var.shape != y.shape:
        raise ValueError("y, mean and var must be (N, K) arrays of one shape")
    lo, hi = check_ranges(ranges, y.shape[0])
    rmse, nlpd = np.empty((lo.size, y.shape[1])), np.empty((lo.size, y.shape[1]))
    for e, (a, b) in enumerate(zip(lo, hi)):
        r = y[a:b] - mean[a:b]
        rmse[e] = np.sqrt(np.mean(r * r, axis=0))
        nlpd[e] = np.mean(0.5 * np.log(2.0 * np.pi * var[a:b]) + 0.5 * r * r / var[a:b], axis=0)
    return rmse, nlpd
