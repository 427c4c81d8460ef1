"""A numpy mirror of what the reference computes for ONE spatial mode count when ``run_spatial_modes`` varies it
(production/analysis/cross_validation.py:96-102): ``reverse_transform`` (gpras/preprocess.py:1052-1094) on the state sliced to ``k`` modes,
the depth conversion of production/analysis/pipeline.py:262-277, and the accumulators and tables of gpras/metrics.py.  Shared by the CPU
pins (test_sweep.py) and the GPU parity tests (test_gpu_sweep.py), with the synthetic cases both use."""

import numpy as np

from oracle import metrics as om


def sliced(state: dict, k: int) -> dict:
    """The fitted state with the first ``k`` modes: what ``EOFProjector.truncate(k)`` holds."""
    out = dict(state)
    out["eofs"], out["x_mean"], out["x_std"] = state["eofs"][:k], state["x_mean"][:k], state["x_std"][:k]
    return out


def reverse_transform(state: dict, mean, var=None):
    """preprocess.py:1067-1085 with ``_linear_transform_for_var`` (:1087-1094), numpy operation by numpy operation."""
    dry = state["dry"]
    m = (mean * state["x_std"]) + state["x_mean"]
    m = np.dot(m, state["eofs"])
    if state["weights"] is not None:
        m /= state["weights"]
    m += state["input_mean"]
    full = np.empty((m.shape[0], dry.shape[0]))
    full[:, dry] = 0 if state["hp"] == "depth" else state["elevations"][dry]
    full[:, ~dry] = m
    if var is None:
        return full, None
    a = np.diag(state["x_std"]).dot(state["eofs"])
    if state["weights"] is not None:
        a /= state["weights"].reshape(1, -1)
    vfull = np.empty_like(full)
    vfull[:, dry] = 0
    vfull[:, ~dry] = var.dot(a**2)
    return full, vfull


def wse_2_depth(x, elevations):
    d = x - elevations  # preprocess.py:1041-1045
    d[d < 0] = 0
    return d


def truth_in_metric_space(state: dict, truth):
    return truth.copy() if state["hp"] == "velocity" else wse_2_depth(truth, state["elevations"])


def metric_fields(state: dict, k: int, mean, var, truth):
    """(x, y, conf) as ``export_metric_summary`` receives them at ``spatial_mode_count = k`` (pipeline.py:261-286); ``conf`` None without var."""
    st = sliced(state, k)
    y, v = reverse_transform(st, mean[:, :k], None if var is None else var[:, :k])
    if state["hp"] != "velocity":
        if state["hp"] == "depth":
            y += state["elevations"]
        y = wse_2_depth(y, state["elevations"])
    return truth_in_metric_space(state, truth), y, None if v is None else np.sqrt(v)


def accumulators(x, y, conf, v_tol: float) -> dict:
    """Per event: the quantities the sweep returns, by numpy's own reductions."""
    e = x - y
    cols = np.arange(x.shape[1])
    y_mts, x_mts = np.argmax(y, axis=0), np.argmax(x, axis=0)
    zeros = np.zeros_like(e)
    c = zeros if conf is None else conf
    return {
        "cell_sum_e": e.sum(axis=0), "cell_sum_e2": (e * e).sum(axis=0), "cell_sum_conf": c.sum(axis=0), "cell_sum_abs": np.abs(e).sum(axis=0),
        "y_peak": y[y_mts, cols], "x_at_y_mts": x[y_mts, cols], "y_mts": y_mts, "x_peak": x[x_mts, cols], "x_mts": x_mts,
        "row_sum_e": e.sum(axis=1), "row_sum_e2": (e * e).sum(axis=1), "row_sum_conf": c.sum(axis=1),
        "matches": int(np.sum(np.abs(y - x) <= v_tol)),
    }


def peak_margins(x, y, depth_threshold: float, v_tol: float) -> float:
    """The smallest distance of any decision the integer outputs depend on from its tie: every column's maximum above its runner-up
    (of x and of y), every peak and every truth-at-the-prediction's-peak from ``depth_threshold``, every |y - x| from ``v_tol``."""
    out = [np.min(np.abs(np.abs(y - x) - v_tol))]
    cols = np.arange(x.shape[1])
    for f in (x, y):
        s = np.sort(f, axis=0)
        if f.shape[0] > 1:
            out.append(np.min(s[-1] - s[-2]))
        out.append(np.min(np.abs(s[-1] - depth_threshold)))
    out.append(np.min(np.abs(x[np.argmax(y, axis=0), cols] - depth_threshold)))
    return float(min(out))


def tables(x, y, conf, index, columns, depth_threshold, v_tol, hp):
    """The three tables of ``export_metric_summary`` at t_tol = 0 (oracle.metrics, the repository's restatement of metrics.py:11-82)."""
    import pandas as pd

    frame = lambda a: pd.DataFrame(a, index=index, columns=columns)  # noqa: E731
    return om.export_metric_tables(frame(x), frame(y), frame(np.zeros_like(x) if conf is None else conf), depth_threshold, 0, v_tol, hp)


def make_case(cells, k, event_lens, hp, weighted=True, dry=(), seed=0, gap=0, nan_at=None, deep=False):
    """A fitted state, a prediction in EOF-score space and a native-space truth.  ``event_lens``: rows per event, laid out one after the
    other with ``gap`` rows of no event in front of each; ``dry``: indices of always-dry cells; ``deep``: the water stays metres above the
    ground everywhere, so that no depth is clamped to zero (no ties at zero)."""
    rng = np.random.default_rng(seed)
    dry_mask = np.zeros(cells, dtype=bool)
    dry_mask[list(dry)] = True
    n_wet = int(cells - dry_mask.sum())
    elevations = rng.uniform(0.0, 2.0, size=cells)
    offset = 0.0 if hp == "velocity" else (3.0 if deep else 0.4)
    native_mean = rng.uniform(0.2, 1.0, size=n_wet) + offset + (0.0 if hp != "wse" else elevations[~dry_mask])
    state = {
        "dry": dry_mask, "elevations": elevations, "hp": hp, "input_mean": native_mean,
        "weights": rng.uniform(0.5, 1.5, size=n_wet) if weighted else None,
        "eofs": rng.normal(size=(k, n_wet)) / np.sqrt(n_wet), "x_mean": rng.normal(size=k) * 0.1, "x_std": rng.uniform(0.5, 2.0, size=k) * np.sqrt(n_wet) * 0.05,
    }
    ranges, row = [], 0
    for n in event_lens:
        row += gap
        ranges.append((row, row + n))
        row += n
    rows = row
    mean = rng.normal(size=(rows, k))
    var = rng.uniform(0.01, 0.3, size=(rows, k))
    clean, _ = reverse_transform(state, mean)
    if hp == "depth":
        clean = clean + elevations  # a "depth" model reconstructs depths; the truth arrives as water-surface elevations
    truth = clean + 0.2 * rng.normal(size=clean.shape)
    if nan_at is not None:
        for t, c in nan_at:
            truth[t, c] = np.nan
    return state, mean, var, truth, ranges
