"""Event-fold cross-validation: for every training event the model is REFITTED on all other rows -- inducing points, hyperparameters and
all -- and predicts at the event's rows.  This is the quantity ``production/analysis/cross_validation.py`` of the reference is about, for
every event of the training set; ``gpras_amd.loeo`` gives the cheaper one that keeps the fitted parameters.

A fold is the reference's fit on the remaining rows (gpr.py:277-308): initial Z from ``_create_inducing(x[keep], ...)``, initial
lengthscale ``mean(|x[keep]|)``, variance 1 and noise 1, then the chosen optimiser.

Two routes:

``"held"``     ONE ``Engine`` on the full data.  The K modes x E events are E K cells of the batched drivers, ordered fold-major
               (event, mode); cell (e, k) holds the rows of event e out (``Engine.*_batch(holds=...)``, ``gprx_*_held``).  The resident
               optimiser loops are at their best with many cells, and E K of them share one training set.  Serves sparse models with
               M <= 64 and d <= 64 and the drivers that are batched loops from end to end (``adam``, ``two-stage``, ``adadelta``).
``"held_general"`` the held route for 64 < M <= 320: the same cells, drivers and predict calls on an engine whose handle has
               ``"held_general"`` = 1, so that the general launch sequence masks the held rows.  Only on request:
               ``"auto"`` does not take it.
``"engines"``  the definition: per fold ``GPRAS(kernel).fit(x[keep], y[keep], ...)`` then ``.predict(x[a:b])``.  Serves everything.

``"auto"`` takes ``"held"`` where it applies.  The routes agree at a fold's initial state to rounding (1e-8); after optimiser steps
their trajectories differ in the last digits, as any two summation orders do.
"""

from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import Any

import numpy as np

from .loeo import event_scores, resolve_events

ROUTES = ("auto", "held", "held_general", "engines")
HELD_MAX_M = 64
HELD_GENERAL_MAX_M = 320  # the bound of the blocked leave-one-event-out route
HELD_MAX_D = 64
HELD_METHODS = ("adam", "two-stage", "adadelta")  # drivers whose every evaluation goes through the batched loops
HELD_MAX_CELLS = 128  # cells per batched driver call, as GPRAS._run_optimizers


@dataclass
class CrossValidationResult:
    """``mean`` / ``var``: ``(N, K)`` as ``leave_event_out`` returns them -- at every event's rows the prediction of the fold that did not
    see them, NaN at rows of no event.  ``ranges``: the events as ``(lo, hi)``.  ``thetas (E, K, n_theta)`` and ``Z (E, K, M, d)``: every
    fold's fitted unconstrained hyperparameters and inducing points (``Z`` is None for exact models).  ``n_evals (E, K)``: evaluations
    per fold cell.  ``first_loss`` / ``last_loss (E, K)``: the training loss, all parameters trainable, before and after the optimiser.
    ``route``: the route that ran; ``last_timings_ms``: wall time of its stages."""

    mean: np.ndarray
    var: np.ndarray
    ranges: list
    thetas: np.ndarray
    Z: np.ndarray | None
    n_evals: np.ndarray
    first_loss: np.ndarray
    last_loss: np.ndarray
    route: str
    last_timings_ms: dict = field(default_factory=dict)

    def scores(self, y):
        """``(rmse, nlpd)``, each ``(events, K)`` (``gpras_amd.loeo.event_scores``)."""
        return event_scores(y, self.mean, self.var, self.ranges)


def fold_cells(n_events: int, n_modes: int):
    """The cells of the held route in batch order, fold-major: ``[(event, mode)]`` with cell ``e * n_modes + k`` = (e, k), so that a
    fold's modes are consecutive (one ``predict_batch`` per fold takes a slice) and a part of the batch covers whole folds first."""
    return [(e, k) for e in range(int(n_events)) for k in range(int(n_modes))]


def held_applies(n_inducing, d: int, optimization_method: str) -> str | None:
    """None when the held route takes this configuration, else the reason it does not."""
    if n_inducing is None:
        return "exact model (n_inducing=None)"
    if int(n_inducing) > HELD_MAX_M:
        return f"more than {HELD_MAX_M} inducing points"
    if d > HELD_MAX_D:
        return f"more than {HELD_MAX_D} features"
    if optimization_method not in HELD_METHODS:
        return f"optimization_method {optimization_method!r} is not one batched loop (held route: {', '.join(HELD_METHODS)})"
    return None


def held_general_applies(n_inducing, d: int, optimization_method: str) -> str | None:
    """None when ``route="held_general"`` takes this configuration (sparse, 64 < M <= 320, d <= 64, one batched loop), else the reason it
    does not."""
    if n_inducing is None:
        return "exact model (n_inducing=None)"
    if int(n_inducing) <= HELD_MAX_M:
        return f"no more than {HELD_MAX_M} inducing points (route='held' serves them)"
    if int(n_inducing) > HELD_GENERAL_MAX_M:
        return f"more than {HELD_GENERAL_MAX_M} inducing points"
    if d > HELD_MAX_D:
        return f"more than {HELD_MAX_D} features"
    if optimization_method not in HELD_METHODS:
        return f"optimization_method {optimization_method!r} is not one batched loop (held routes: {', '.join(HELD_METHODS)})"
    return None


def _checked(kernel, x, y, events, n_inducing, inducing_initializer, optimization_method, route, start):
    """Every argument error, before any library call.  Returns ``(x, y, lo, hi, route that will run)``."""
    from .gpr import _REFERENCE_ONLY, KERNEL_FACTORY
    from .optimizers import OPTIMIZERS

    if route not in ROUTES:
        raise ValueError(f"route must be one of {ROUTES}, got {route!r}")
    if kernel not in KERNEL_FACTORY or kernel in _REFERENCE_ONLY:
        raise ValueError(f"kernel {kernel!r} cannot be fitted")
    if optimization_method not in OPTIMIZERS:
        raise ValueError(f"unknown optimization_method {optimization_method!r}")
    if inducing_initializer not in ("kmeans", "grid"):
        raise ValueError(f"unknown inducing initializer {inducing_initializer!r}")
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if x.ndim != 2 or y.ndim != 2 or x.shape[0] != y.shape[0] or x.shape[0] == 0:
        raise ValueError("x must be (N, d) and y (N, K) with matching N")
    if n_inducing is not None and (int(n_inducing) != n_inducing or int(n_inducing) < 1):
        raise ValueError(f"n_inducing must be a positive integer or None, got {n_inducing!r}")
    lo, hi = resolve_events(events, x.shape[0])
    if int((hi - lo).max()) >= x.shape[0]:
        raise ValueError("an event covers every row: nothing is left to fit a fold on")
    if start is not None:
        models = getattr(start, "models", None)
        if not models or len(models) != y.shape[1]:
            raise ValueError("start must be a fitted GPRAS with one model per column of y")
        if any((m.Z is None) != (n_inducing is None) for m in models) or (n_inducing is not None and any(np.shape(m.Z) != (int(n_inducing), x.shape[1]) for m in models)):
            raise ValueError("start: its inducing points do not have the shape (n_inducing, d) of this call")
    why_not = held_applies(n_inducing, x.shape[1], optimization_method)
    if route == "held" and why_not is not None:
        raise ValueError(f"route='held' does not apply: {why_not}")
    if route == "held_general":
        why_not_general = held_general_applies(n_inducing, x.shape[1], optimization_method)
        if why_not_general is not None:
            raise ValueError(f"route='held_general' does not apply: {why_not_general}")
        return x, y, lo, hi, "held_general"
    return x, y, lo, hi, ("engines" if (route == "engines" or why_not is not None) else "held")


def _assign_start(models, start):
    """Every fold's mode k starts from the fitted parameters of ``start.models[k]`` in place of the reference's initial state."""
    for mod in models:
        src = start.models[mod.unit]
        mod.w_var, mod.w_len, mod.w_noise = src.w_var, src.w_len.copy(), src.w_noise
        if src.Z is not None:
            mod.Z = src.Z.copy()


def _losses(models):
    """The training loss of every model, all parameters trainable (what a fold's first and last loss are compared by)."""
    from .optimizers import _evaluate_many

    out = np.empty(len(models))
    for c0 in range(0, len(models), HELD_MAX_CELLS):
        part = models[c0 : c0 + HELD_MAX_CELLS]
        out[c0 : c0 + len(part)], _ = _evaluate_many(part, want_grad=False)
    return out


def _held(helper, x, y, lo, hi, n_inducing, inducing_initializer, optimization_method, ard, include_noise, start, opt_kwargs, general=False):
    from .engine import Engine
    from .model import GPModel
    from .optimizers import BATCHED_OPTIMIZERS

    n, k = x.shape[0], y.shape[1]
    ranges = list(zip(lo.tolist(), hi.tolist()))
    t0 = time.perf_counter()
    inits = []
    for a, b in ranges:
        keep = np.r_[0:a, b:n]
        inits.append((helper._create_inducing(x[keep], int(n_inducing), inducing_initializer), np.mean(abs(x[keep]))))
    eng = Engine(helper.kernel_str, x, y, int(n_inducing), ard=bool(ard), device=helper.device, distance_form=helper.distance_form)
    try:
        if general:
            eng.set_handle_tuning("held_general", 1)
        models = []
        for e, mode in fold_cells(len(ranges), k):
            mod = GPModel(eng, mode, inits[e][0], 1.0, inits[e][1], 1.0)
            mod.hold = ranges[e]
            models.append(mod)
        if start is not None:
            _assign_start(models, start)
        t1 = time.perf_counter()
        first = _losses(models)
        before = np.array([m.n_evals for m in models])
        per = max(1, min(HELD_MAX_CELLS, eng.max_cells(want_grad=True)))
        for c0 in range(0, len(models), per):
            BATCHED_OPTIMIZERS[optimization_method](models[c0 : c0 + per], **opt_kwargs)
        n_evals = np.array([m.n_evals for m in models]) - before
        last = _losses(models)
        eng.synchronize()
        t2 = time.perf_counter()
        mean, var = np.full((n, k), np.nan), np.full((n, k), np.nan)
        for e, (a, b) in enumerate(ranges):
            part = models[e * k : (e + 1) * k]
            mu, vv = eng.predict_batch([m.unit for m in part], np.stack([m.theta() for m in part]), x[a:b], zs=np.stack([m.Z for m in part]),
                                       include_noise=include_noise, holds=[m.hold for m in part])
            mean[a:b], var[a:b] = mu.T, vv.T
        t3 = time.perf_counter()
        thetas = np.stack([m.theta() for m in models]).reshape(len(ranges), k, -1)
        zs = np.stack([m.Z for m in models]).reshape(len(ranges), k, int(n_inducing), x.shape[1])
    finally:
        eng.close()
    shape = (len(ranges), k)
    timings = {"init_ms": 1e3 * (t1 - t0), "fit_ms": 1e3 * (t2 - t1), "predict_ms": 1e3 * (t3 - t2), "total_ms": 1e3 * (t3 - t0)}
    return CrossValidationResult(mean, var, ranges, thetas, zs, n_evals.reshape(shape), first.reshape(shape), last.reshape(shape),
                                 "held_general" if general else "held", timings)


def _engines(helper, x, y, lo, hi, n_inducing, inducing_initializer, optimization_method, ard, include_noise, start, opt_kwargs):
    from .gpr import GPRAS

    n, k = x.shape[0], y.shape[1]
    ranges = list(zip(lo.tolist(), hi.tolist()))
    mean, var = np.full((n, k), np.nan), np.full((n, k), np.nan)
    thetas, zs, n_evals, first, last = [], [], [], [], []
    t_fit = t_pred = 0.0
    t0 = time.perf_counter()
    for a, b in ranges:
        keep = np.r_[0:a, b:n]
        g = GPRAS(helper.kernel_str, device=helper.device, distance_form=helper.distance_form)
        try:
            # GPRAS.fit(x[keep], y[keep], ...) in its two halves, with the fold's first and last loss taken around the second
            g.x, g.y = x[keep], y[keep]
            g._init_models(g.x, g.y, n_inducing, inducing_initializer, ard)
            if start is not None:
                _assign_start(g.models, start)
            first.append(_losses(g.models))
            before = np.array([m.n_evals for m in g.models])
            g._run_optimizers(g.models, optimization_method, None, opt_kwargs)
            n_evals.append(np.array([m.n_evals for m in g.models]) - before)
            last.append(_losses(g.models))
            t1 = time.perf_counter()
            mu, vv = g.predict(x[a:b])
            if not include_noise:
                vv = vv - np.array([m.noise for m in g.models])[None, :]
            mean[a:b], var[a:b] = mu, vv
            t_pred += time.perf_counter() - t1
            thetas.append(np.stack([m.theta() for m in g.models]))
            zs.append(None if n_inducing is None else np.stack([m.Z for m in g.models]))
        finally:
            for eng in g.engines:
                eng.close()
    total = time.perf_counter() - t0
    t_fit = total - t_pred
    timings = {"init_ms": 0.0, "fit_ms": 1e3 * t_fit, "predict_ms": 1e3 * t_pred, "total_ms": 1e3 * total}
    return CrossValidationResult(mean, var, ranges, np.stack(thetas), None if n_inducing is None else np.stack(zs), np.stack(n_evals),
                                 np.stack(first), np.stack(last), "engines", timings)


def cross_validate(kernel, x, y, events, n_inducing, inducing_initializer="kmeans", optimization_method="two-stage", ard=False, route="auto",
                   include_noise=True, device=0, distance_form=None, start=None, **opt_kwargs: Any) -> CrossValidationResult:
    """Event-fold cross-validation of ``GPRAS(kernel).fit(x, y, n_inducing, inducing_initializer, optimization_method, ard, **opt_kwargs)``:
    for every event (``events``: ``(lo, hi)`` row ranges, one label per row, or a pandas index whose first level is the event --
    ``loeo.resolve_events``) that fit on all OTHER rows, and its ``predict`` at the event's rows.  Every argument is checked before the
    first library call.  ``start`` (optional, a fitted ``GPRAS`` on the same columns): every fold starts from its modes' fitted
    parameters instead of the reference's initial state (a warm start; with ``adam`` at ``max_iter=0`` the result is
    ``leave_event_out``'s quantity)."""
    from .gpr import GPRAS

    x, y, lo, hi, use = _checked(kernel, x, y, events, n_inducing, inducing_initializer, optimization_method, route, start)
    helper = GPRAS(kernel, device=device, distance_form=distance_form)
    if use == "held_general":
        return _held(helper, x, y, lo, hi, n_inducing, inducing_initializer, optimization_method, ard, include_noise, start, opt_kwargs, general=True)
    run = _held if use == "held" else _engines
    return run(helper, x, y, lo, hi, n_inducing, inducing_initializer, optimization_method, ard, include_noise, start, opt_kwargs)
