"""Mode-count sweep (gpras_amd.sweep), host logic: the prefix property of the fit that the sweep rests on, ``EOFProjector.truncate``,
``FieldSummary.peaks`` and its refusals, ``scalar_table`` / ``export`` from hand-made accumulators against the numpy mirror
(sweep_numpy.py), and the argument errors that are raised before any device work."""

import sqlite3
import types

import numpy as np
import pandas as pd
import pytest

import sweep_numpy as sn
from pca_fit_numpy import fit_reference


# ---- the leading k modes of a k-mode fit are the sliced state of a K-mode fit ------------------------------------------------------------
@pytest.mark.parametrize("mode,weighted", [("wse", True), ("depth", False), ("velocity", True)])
def test_leading_modes_do_not_depend_on_the_count_kept(mode, weighted):
    rng = np.random.default_rng(5)
    rows, cells, k_full = 24, 60, 9
    elev = rng.uniform(0.0, 2.0, size=cells)
    modes = rng.normal(size=(k_full + 3, cells)) * np.linspace(2.0, 0.3, k_full + 3)[:, None]
    x = np.abs(rng.normal(size=(rows, k_full + 3)) @ modes) + (elev if mode != "velocity" else 0.0)
    w = rng.uniform(0.5, 1.5, size=cells) if weighted else None
    full = fit_reference(x, elev, w, k_full, mode)
    lam_max = full["eigenvalues"][0]
    for k in (1, 4, k_full):
        part = fit_reference(x, elev, w, k, mode)
        assert np.array_equal(part["wetness_classes"], full["wetness_classes"]) and np.array_equal(part["input_mean"], full["input_mean"])
        # the bounds tests/pca_fit_numpy.py:assert_fit_close allows a fit against its restatement
        for i in range(k):
            assert np.max(np.abs(part["eofs"][i] - full["eofs"][i])) <= 1e-13 * lam_max / full["eigenvalues"][i]
        assert np.max(np.abs(part["x_mean"] - full["x_mean"][:k])) <= 1e-12 * full["x_std"][0]
        assert np.max(np.abs(part["x_std"] - full["x_std"][:k]) / full["x_std"][:k]) <= 1e-11


# ---- EOFProjector.truncate ------------------------------------------------------------------------------------------------------
def _projector(monkeypatch, state):
    from gpras_amd.preprocess import EOFProjector

    monkeypatch.setattr(EOFProjector, "_create", lambda self: None)  # no device in this test: the handle stays null
    monkeypatch.setattr(EOFProjector, "close", lambda self: None)
    return EOFProjector(state["dry"], state["elevations"], state["input_mean"], state["weights"], state["eofs"], state["x_mean"], state["x_std"], state["hp"])


def test_truncate_keeps_the_leading_modes(monkeypatch):
    state, *_ = sn.make_case(40, 7, [5], "wse", weighted=True, dry=(3, 9), seed=1)
    proj = _projector(monkeypatch, state)
    for k in (1, 3, 7):
        sub = proj.truncate(k)
        want = sn.sliced(state, k)
        assert sub is not proj and sub.spatial_mode_count == k and sub.n_cells == 40 and sub.hydraulic_parameter == "wse"
        for name, attr in (("eofs", "eofs"), ("x_mean", "x_mean"), ("x_std", "x_std"), ("input_mean", "input_mean"), ("weights", "weights"),
                           ("elevations", "elevations"), ("dry", "dry_indices")):
            assert np.array_equal(getattr(sub, attr), want[name])
    assert proj.spatial_mode_count == 7 and proj.eofs.shape[0] == 7
    for bad in (0, 8, -1, 2.5):
        with pytest.raises(ValueError, match=r"k must be an integer in \[1, 7\]"):
            proj.truncate(bad)


# ---- a SweepResult made by hand from the mirror's accumulators -----------------------------------------------------------------------
def _hand_made(hp, v_tol=0.05, with_var=True):
    from gpras_amd.sweep import SweepResult

    state, mean, var, truth, ranges = sn.make_case(23, 6, [7, 1, 9], hp, weighted=True, dry=(4,), seed=11)
    if not with_var:
        var = None
    counts = [1, 4, 6]
    rows = truth.shape[0]
    names = ["a", "b", "c"]
    row_sums = np.zeros((len(counts), rows, 3))
    matches = np.zeros((len(counts), len(ranges)), dtype=np.uint64)
    host, fields = {}, {}
    for j, k in enumerate(counts):
        x, y, conf = sn.metric_fields(state, k, mean, var, truth)
        fields[k] = (x, y, conf)
        for i, (lo, hi) in enumerate(ranges):
            acc = sn.accumulators(x[lo:hi], y[lo:hi], None if conf is None else conf[lo:hi], v_tol)
            row_sums[j, lo:hi] = np.stack([acc["row_sum_e"], acc["row_sum_e2"], acc["row_sum_conf"]], axis=1)
            matches[j, i] = acc["matches"]
            host[(j, i)] = (np.stack([acc[n] for n in ("cell_sum_e", "cell_sum_e2", "cell_sum_conf", "cell_sum_abs", "y_peak", "x_at_y_mts")]),
                            acc["y_mts"].astype(np.int32))
            host[("x", i)] = (acc["x_peak"], acc["x_mts"].astype(np.int32))
    res = SweepResult(counts, ranges, names, rows, 23, v_tol, 0, with_var, "fused", row_sums, matches, {"total": 0.0}, cell_host=host)
    index = pd.MultiIndex.from_tuples([(n, 10 * t) for n, (lo, hi) in zip(names, ranges) for t in range(hi - lo)], names=["event", "timestep"])
    columns = [f"c{c}" for c in range(23)]
    return res, fields, index, columns, ranges, names


def test_field_summary_peaks_and_refusals():
    res, fields, _, _, ranges, names = _hand_made("wse")
    fs = res.summary(4, "c")
    lo, hi = ranges[2]
    x, y, _ = fields[4]
    x, y = x[lo:hi], y[lo:hi]
    cols = np.arange(x.shape[1])
    assert fs.rows == hi - lo and fs.cells == 23
    xp, yp = fs.peaks()
    assert np.array_equal(xp, x.max(axis=0)) and np.array_equal(yp, y.max(axis=0))
    xp, yp = fs.peaks(fs.x_mts, fs.y_mts)
    assert np.array_equal(xp, x.max(axis=0)) and np.array_equal(yp, y.max(axis=0))
    # the reference's positional f2_mts(x, y, x_mts, y_mts): the truth at the prediction's argmax (metrics.py:52-53)
    xp, yp = fs.peaks(fs.y_mts.copy(), None)
    assert np.array_equal(xp, x[np.argmax(y, axis=0), cols]) and np.array_equal(yp, y.max(axis=0))
    other = (fs.x_mts + 1) % fs.rows
    assert not np.array_equal(other, fs.x_mts) and not np.array_equal(other, fs.y_mts)
    with pytest.raises(ValueError, match="no field is resident"):
        fs.peaks(other, None)
    with pytest.raises(ValueError, match="no field is resident"):
        fs.peaks(None, other)
    with pytest.raises(ValueError, match="no field is resident"):
        fs.rmse_aoi_mts(np.zeros(23, dtype=np.int64) + 99, None)
    with pytest.raises(KeyError):
        res.summary(5, "a")
    with pytest.raises(KeyError):
        res.summary(4, "nope")
    assert fs.mae_aoi_toi() == pytest.approx(np.abs(x - y).mean(), rel=1e-14)
    assert fs.fi_aoi_toi() == np.sum(np.abs(y - x) <= 0.05) / x.size


@pytest.mark.parametrize("hp,with_var", [("wse", True), ("depth", True), ("velocity", False)])
def test_scalar_table_and_export_equal_the_mirror(tmp_path, hp, with_var):
    from gpras_amd.sweep import SCALAR_COLUMNS

    res, fields, index, columns, ranges, names = _hand_made(hp, with_var=with_var)
    table = res.scalar_table(depth_threshold=0.5, hydraulic_parameter=hp)
    assert list(table.columns) == ["spatial_mode_count", "event", *SCALAR_COLUMNS]
    assert list(table["spatial_mode_count"]) == [1] * 3 + [4] * 3 + [6] * 3 and list(table["event"]) == names * 3
    paths = res.export(tmp_path / "spatial_mode_count", index, columns, depth_threshold=0.5, hydraulic_parameter=hp)
    assert [p.relative_to(tmp_path).as_posix() for p in paths] == [f"spatial_mode_count/{i}/performance_metrics.db" for i in range(3)]
    exact = {"event", "timestep", "cell_id", "fi_aoi_toi", "pod_mts", "rfa_mts", "csi_mts", "f2_mts", "f3_mts", "err_cell_mts"}
    for pos, k in enumerate(res.counts):
        x, y, conf = fields[k]
        want = dict(zip(("scalar_metrics", "timeseries_metrics", "cell_metrics"), sn.tables(x, y, conf, index, columns, 0.5, 0.05, hp)))
        for name, frame in want.items():
            with sqlite3.connect(paths[pos]) as con:
                got = pd.read_sql(f"select * from {name}", con)
            frame = frame.reset_index(drop=True)
            assert list(got.columns) == list(frame.columns) and len(got) == len(frame)
            for col in frame.columns:
                if col in ("event", "cell_id"):
                    assert list(got[col]) == list(frame[col]), (name, col)
                elif col in exact:  # (a NaN column comes back from sqlite as NULLs)
                    assert np.array_equal(got[col].values.astype(float), frame[col].values.astype(float), equal_nan=True), (name, col)
                else:
                    np.testing.assert_allclose(got[col].values, frame[col].values, rtol=1e-12, atol=1e-15, err_msg=f"{name}.{col}")
        sub = table[table["spatial_mode_count"] == k].drop(columns="spatial_mode_count").reset_index(drop=True)
        with sqlite3.connect(paths[pos]) as con:
            pd.testing.assert_frame_equal(sub, pd.read_sql("select * from scalar_metrics", con), check_exact=True, check_dtype=False)
    with pytest.raises(ValueError, match="one entry per row"):
        res.export(tmp_path / "x", index[:-1], columns)


# ---- argument errors before any device work ----------------------------------------------------------------------------------------
def test_counts_are_checked():
    from gpras_amd.sweep import check_counts

    assert check_counts([1, 3, 50], 50).dtype == np.int32
    for bad in ([], [0, 1], [1, 1], [3, 2], [1, 51], [[1, 2]], [1.0, 2.0], list(range(1, 66))):
        with pytest.raises(ValueError):
            check_counts(bad, 64 if len(bad) > 60 else 50)


def test_evaluate_refuses_before_touching_the_device():
    from gpras_amd.sweep import ModeCountSweep

    proj = types.SimpleNamespace(spatial_mode_count=5, n_cells=7, device=0, hydraulic_parameter="wse", elevations=np.zeros(7))
    with pytest.raises(ValueError, match="strictly increasing"):
        ModeCountSweep(proj, [2, 6])
    sweep = ModeCountSweep(proj, [1, 5])
    mean, truth = np.zeros((10, 5)), np.zeros((10, 7))
    with pytest.raises(ValueError, match="route"):
        sweep.evaluate(mean, None, truth, [(0, 10)], route="eager")
    with pytest.raises(ValueError, match="t_tol = 0 only"):
        sweep.evaluate(mean, None, truth, [(0, 10)], t_tol=1, route="fused")
    with pytest.raises(ValueError, match="t_tol"):
        sweep.evaluate(mean, None, truth, [(0, 10)], t_tol=9, route="refield")
    with pytest.raises(ValueError, match="v_tol"):
        sweep.evaluate(mean, None, truth, [(0, 10)], v_tol=-1.0)
    with pytest.raises(ValueError, match="no events"):
        sweep.evaluate(mean, None, truth, [])
    for bad in ([(0, 0)], [(0, 11)], [(-1, 3)], [(4, 2)]):
        with pytest.raises(ValueError, match="need 0 <= lo < hi <= rows"):
            sweep.evaluate(mean, None, truth, bad)
    with pytest.raises(ValueError, match="overlap"):
        sweep.evaluate(mean, None, truth, [(0, 6), (5, 10)])
    proj.elevations = None
    with pytest.raises(ValueError, match="elevations"):
        sweep.evaluate(mean, None, truth, [(0, 10)])
