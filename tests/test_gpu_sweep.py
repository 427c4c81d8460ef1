"""Mode-count sweep on the GPU (gpras_amd.sweep, csrc/sweep.h): the fused pass against ``route="refield"`` (the per-count chain on the
kernels that existed before it) bit for bit per cell and under a derived bound per timestep, repeatability and the grouping of counts,
the numpy mirror (sweep_numpy.py), ``DevicePipeline.mode_count_sweep`` against one ``export_metric_summary`` per truncated pipeline, and
every GPRX_EINVAL path of ``gprx_pca_sweep_dev``.

The bound of the per-timestep sums.  Both routes add the same, bit-identical terms ``v_c`` (``e``, ``e*e`` or ``conf``) over the cells of a
row, in two different fixed orders without compensation.  A sum ``s`` in which no term passes through more than ``m`` roundings satisfies
``|s - sum v| <= gamma_m sum |v|`` with ``gamma_m = m u / (1 - m u)``, ``u = 2**-53`` (Higham, Accuracy and Stability, section 4.2); ``m`` is at
most ``cells - 1`` for any order of plain additions, so two such sums differ by at most ``2 gamma_{cells-1} sum_c |v_c|``.  (``e*e`` enters the
chain's sum through one fused multiply-add per term and the sweep's as a rounded product: one rounding either way, and the partial sums per
thread and the reduction trees of both kernels stay far below ``cells - 1`` roundings at the sizes tested; at one cell both are ``fl(e*e)``.)
The right-hand side is evaluated in longdouble from the refield route's fields.  For one cell the bound is zero: the sums must be equal."""

import copy
import ctypes as C
import sqlite3

import numpy as np
import pandas as pd
import pytest

import sweep_numpy as sn

pytestmark = pytest.mark.gpu

U = 2.0**-53


def gamma(m: int):
    return np.longdouble(m * U) / (1 - np.longdouble(m * U))


def _projector(state):
    from gpras_amd.preprocess import EOFProjector

    return EOFProjector(state["dry"], state["elevations"], state["input_mean"], state["weights"], state["eofs"], state["x_mean"], state["x_std"], state["hp"])


def _refield_fields(sweep, counts, mean, var, rows, cells):
    """The per-count fields of the refield route on the host: {count: (y, conf or None)}."""
    from gpras_amd._lib import DeviceBuffer

    by_mode = [DeviceBuffer.from_array(np.ascontiguousarray(mean.T)), None if var is None else DeviceBuffer.from_array(np.ascontiguousarray(var.T))]
    out = {}
    try:
        for k in counts:
            pred, conf = sweep.refield(int(k), by_mode[0], by_mode[1], rows)
            out[int(k)] = (pred.to_array((rows, cells)), None if conf is None else conf.to_array((rows, cells)))
            pred.free()
            if conf is not None:
                conf.free()
    finally:
        for b in by_mode:
            if b is not None:
                b.free()
    return out


def _within(a, b, bound):
    """|a - b| <= bound elementwise; where the reference sum is NaN (a NaN in the truth) both must be NaN."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan)
    assert np.all(np.abs(a - b)[~nan] <= np.asarray(bound)[~nan]), float(np.max((np.abs(a - b)[~nan] - np.asarray(bound)[~nan])))


def _assert_routes_agree(sweep, fused, refield, x, fields, ranges, cells, depth_threshold=0.5):
    assert np.array_equal(fused.matches, refield.matches)
    g = gamma(cells - 1)
    for j, k in enumerate(fused.counts):
        y, conf = fields[k]
        e_dev = x - y  # the device's e = fl(x - y): the same IEEE subtraction of the same bits
        terms = (np.abs(e_dev), e_dev * e_dev, np.zeros_like(x) if conf is None else conf)
        for q, v in enumerate(terms):
            bound = 2 * g * np.abs(v.astype(np.longdouble)).sum(axis=1)
            rows_in = np.zeros(x.shape[0], dtype=bool)
            for lo, hi in ranges:
                rows_in[lo:hi] = True
            _within(fused.row_sums[j, rows_in, q], refield.row_sums[j, rows_in, q], bound[rows_in])
            assert np.all(fused.row_sums[j, ~rows_in, q] == 0.0)
        for i, (lo, hi) in enumerate(ranges):
            cf, af = fused.cell_block(j, i)
            cr, ar = refield.cell_block(j, i)
            for q in (0, 1, 2, 4, 5):
                assert np.array_equal(cf[q], cr[q], equal_nan=True), (k, i, q)
            # the sixth array: the chain's kernels keep no per-cell sum |e|; its fields give it, added row by row as the device does
            acc = np.zeros(cells)
            for t in range(lo, hi):
                acc = acc + np.abs(x[t] - y[t])
            assert np.array_equal(cf[3], acc, equal_nan=True), (k, i)
            assert np.array_equal(af, ar), (k, i)
            for a, b in zip(fused.truth_block(i), refield.truth_block(i)):
                assert np.array_equal(a, b, equal_nan=True)
            fs, rs = fused.summary(k, fused.names[i]), refield.summary(k, refield.names[i])
            assert fs.fi_aoi_toi() == rs.fi_aoi_toi()
            nan_peaks = np.isnan(fs.x_peak).any()
            for name in ("rmse_aoi_mts", "err_aoi_mts", "nse_aoi_mts"):
                assert np.array_equal(getattr(fs, name)(fs.x_mts, fs.y_mts), getattr(rs, name)(rs.x_mts, rs.y_mts), equal_nan=True), name
            assert np.array_equal(fs.err_cell_mts(fs.x_mts, fs.y_mts), rs.err_cell_mts(rs.x_mts, rs.y_mts), equal_nan=True)
            for thr in (depth_threshold, fs.x_mts):  # (the second: the reference's positional f2_mts / f3_mts call)
                args = (thr, fs.x_mts, fs.y_mts) if thr is not fs.x_mts else (fs.x_mts, fs.y_mts)
                assert tuple(int(v) for v in fs.contingency(*args)) == tuple(int(v) for v in rs.contingency(*args))
            if not nan_peaks:
                assert fs.f2_mts(fs.x_mts, fs.y_mts) == rs.f2_mts(rs.x_mts, rs.y_mts) and fs.f3_mts(fs.x_mts, fs.y_mts) == rs.f3_mts(rs.x_mts, rs.y_mts)
            # scalar totals: the rows' sums are added on the host by numpy in the same order on both sides, each total within
            # gamma_{rows-1} sum_t |row sum| of its exact value; the rows themselves differ by at most their bounds
            n_rows = hi - lo
            for q, v in enumerate(terms):
                vt = np.abs(v[lo:hi].astype(np.longdouble))
                tf, tr = fused.row_sums[j, lo:hi, q], refield.row_sums[j, lo:hi, q]
                if np.isnan(tr).any():
                    assert np.isnan(tf.sum())
                    continue
                bound = 2 * g * vt.sum() + gamma(max(n_rows - 1, 0)) * (np.abs(tf.astype(np.longdouble)).sum() + np.abs(tr.astype(np.longdouble)).sum())
                assert abs(np.longdouble(tf.sum()) - np.longdouble(tr.sum())) <= bound
            # the mean absolute error: sum_c of the per-cell sums against sum_t of the chain's per-row sums, the same |e| in two orders
            va = np.abs(terms[0][lo:hi].astype(np.longdouble)).sum()
            if not np.isnan(va):
                assert abs(np.longdouble(cf[3].sum()) - np.longdouble(refield.row_abs[j, lo:hi].sum())) <= 2 * gamma(n_rows + cells) * va


def _case_run(case, counts, v_tol, with_var=True, nan_rows=()):
    from gpras_amd.sweep import ModeCountSweep

    state, mean, var, truth, ranges = case
    if not with_var:
        var = None
    rows, cells = truth.shape
    x = sn.truth_in_metric_space(state, truth)
    proj = _projector(state)
    sweep = ModeCountSweep(proj, counts)
    fused = sweep.evaluate(mean, var, x, ranges, v_tol=v_tol, route="fused")
    refield = sweep.evaluate(mean, var, x, ranges, v_tol=v_tol, route="refield")
    fields = _refield_fields(sweep, counts, mean, var, rows, cells)
    return proj, sweep, fused, refield, fields, x, ranges, cells


CASES = {
    # name: (cells, K, event lengths, hp, weighted, dry cells, gap, counts, v_tol, with_var, nan_at)
    "one_cell": (1, 1, [1], "velocity", False, (), 0, [1], 0.0, True, None),
    "255_k16": (255, 16, [31, 1, 33], "wse", True, (0, 7, 254), 0, [1, 3, 16], 0.05, True, None),
    "256_k17": (256, 17, [70], "depth", False, (), 0, [17], 0.0, True, None),
    "257_k64_novar": (257, 64, [32, 70, 33], "wse", True, (5, 256), 0, [1, 3, 64], 0.1, False, None),
    "600_groups_nan": (600, 64, [33, 32, 1], "depth", True, tuple(range(256, 512)), 0, [1, 2, 3, 5, 8, 13, 21, 34, 64], 0.05, True, [(2, 3), (40, 599), (65, 100)]),
    "600_k17_gaps": (600, 17, [32], "velocity", False, (), 3, [1], 0.0, True, None),
    "257_k16_last": (257, 16, [70, 31], "velocity", True, (), 2, [16], 0.2, True, [(2, 0), (104, 256)]),  # a NaN in an event's first and last row
    "255_k1": (255, 1, [33, 1, 32], "depth", True, (100,), 0, [1], 0.05, True, None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_fused_equals_refield(lib, name):
    cells, k, lens, hp, weighted, dry, gap, counts, v_tol, with_var, nan_at = CASES[name]
    assert lib.gprx_pca_sweep_group() < 9  # "600_groups_nan" must form more than one group of counts
    case = sn.make_case(cells, k, lens, hp, weighted=weighted, dry=dry, seed=len(name) + cells, gap=gap, nan_at=nan_at)
    proj, sweep, fused, refield, fields, x, ranges, cells = _case_run(case, counts, v_tol, with_var)
    try:
        assert fused.route == "fused" and refield.route == "refield" and fused.has_conf == with_var
        _assert_routes_agree(sweep, fused, refield, x, fields, ranges, cells)
        assert set(fused.stage_timings_ms()) >= {"upload", "evaluate", "download", "total", "device_sweep"}
    finally:
        fused.close()
        refield.close()
        proj.close()


def test_repeatable_and_independent_of_the_grouping(lib):
    from gpras_amd.sweep import ModeCountSweep

    cells, k, lens, hp, weighted, dry, gap, counts, v_tol, with_var, nan_at = CASES["600_groups_nan"]
    state, mean, var, truth, ranges = sn.make_case(cells, k, lens, hp, weighted=weighted, dry=dry, seed=3, gap=gap, nan_at=nan_at)
    x = sn.truth_in_metric_space(state, truth)
    proj = _projector(state)
    full = ModeCountSweep(proj, counts)
    a = full.evaluate(mean, var, x, ranges, v_tol=v_tol, route="fused")
    b = full.evaluate(mean, var, x, ranges, v_tol=v_tol, route="fused")
    part_counts = [3, 13, 64]  # other groups, other positions inside a group
    c = ModeCountSweep(proj, part_counts).evaluate(mean, var, x, ranges, v_tol=v_tol, route="fused")
    try:
        assert np.array_equal(a.row_sums, b.row_sums, equal_nan=True) and np.array_equal(a.matches, b.matches)
        for j in range(len(counts)):
            for i in range(len(ranges)):
                for u, v in zip(a.cell_block(j, i) + a.truth_block(i), b.cell_block(j, i) + b.truth_block(i)):
                    assert np.array_equal(u, v, equal_nan=True)
        for jc, kc in enumerate(part_counts):
            j = counts.index(kc)
            assert np.array_equal(a.row_sums[j], c.row_sums[jc], equal_nan=True) and np.array_equal(a.matches[j], c.matches[jc])
            for i in range(len(ranges)):
                for u, v in zip(a.cell_block(j, i) + a.truth_block(i), c.cell_block(jc, i) + c.truth_block(i)):
                    assert np.array_equal(u, v, equal_nan=True)
    finally:
        for r in (a, b, c):
            r.close()
        proj.close()


@pytest.mark.parametrize("hp", ["wse", "depth", "velocity"])
def test_fused_equals_numpy_mirror(lib, hp):
    """Integer outputs equal, continuous ones within the tolerances tests/test_metrics.py uses for FieldMetrics against the oracle module.
    The margins are a condition of the test: every decision an integer output depends on is at least 1e-6 away from its tie in the mirror."""
    from gpras_amd.sweep import ModeCountSweep

    counts, v_tol, thr = [1, 3, 17], 0.15, (1.3 if hp == "velocity" else 4.3)  # (a threshold that splits the peaks about two to one)
    state, mean, var, truth, ranges = sn.make_case(257, 17, [33, 1, 31], hp, weighted=True, dry=(), seed=77, deep=True)
    x = sn.truth_in_metric_space(state, truth)
    proj = _projector(state)
    res = ModeCountSweep(proj, counts).evaluate(mean, var, x, ranges, v_tol=v_tol, route="fused")
    rel = 1e-12
    try:
        for k in counts:
            xm, ym, cm = sn.metric_fields(state, k, mean, var, truth)
            assert np.array_equal(xm, x)
            for i, (lo, hi) in enumerate(ranges):
                xe, ye, ce = xm[lo:hi], ym[lo:hi], cm[lo:hi]
                assert sn.peak_margins(xe, ye, thr, v_tol) >= 1e-6
                want = sn.accumulators(xe, ye, ce, v_tol)
                fs = res.summary(k, i)
                assert np.array_equal(fs.y_mts, want["y_mts"]) and np.array_equal(fs.x_mts, want["x_mts"]) and fs.matches == want["matches"]
                assert np.array_equal(fs.x_peak, want["x_peak"]) and np.array_equal(fs.x_at_y_mts, want["x_at_y_mts"])
                for args in ((thr, fs.x_mts, fs.y_mts), (fs.x_mts, fs.y_mts)):
                    wargs = (thr, want["x_mts"], want["y_mts"]) if len(args) == 3 else (want["x_mts"], want["y_mts"])
                    assert tuple(int(v) for v in fs.contingency(*args)) == tuple(int(v) for v in sn.om.contingency(xe, ye, *wargs))
                np.testing.assert_allclose(fs.y_peak, want["y_peak"], rtol=rel)
                np.testing.assert_allclose(fs.rmse_aoi_ts(), sn.om.rmse_aoi_ts(xe, ye), rtol=rel)
                np.testing.assert_allclose(fs.err_aoi_ts(), sn.om.err_aoi_ts(xe, ye), rtol=1e-9, atol=1e-14)
                np.testing.assert_allclose(fs.conf_aoi_ts(), sn.om.conf_aoi_ts(ce), rtol=rel)
                np.testing.assert_allclose(fs.rmse_cell_toi(), sn.om.rmse_cell_toi(xe, ye), rtol=rel)
                np.testing.assert_allclose(fs.err_cell_toi(), sn.om.err_cell_toi(xe, ye), rtol=1e-9, atol=1e-14)
                np.testing.assert_allclose(fs.conf_cell_toi(), sn.om.conf_cell_toi(ce), rtol=rel)
                assert fs.rmse_aoi_toi() == pytest.approx(sn.om.rmse_aoi_toi(xe, ye), rel=rel)
                assert fs.mae_aoi_toi() == pytest.approx(sn.om.mae_aoi_toi(xe, ye), rel=rel)
                assert fs.err_aoi_toi() == pytest.approx(sn.om.err_aoi_toi(xe, ye), rel=1e-10, abs=1e-15)
                assert fs.conf_aoi_toi() == pytest.approx(sn.om.conf_aoi_toi(ce), rel=rel)
                assert fs.rmse_aoi_mts(fs.x_mts, fs.y_mts) == pytest.approx(sn.om.rmse_aoi_mts(xe, ye), rel=rel)
                assert fs.err_aoi_mts(fs.x_mts, fs.y_mts) == pytest.approx(sn.om.err_aoi_mts(xe, ye), rel=1e-10, abs=1e-15)
                if hi - lo > 1:
                    assert fs.nse_aoi_mts(fs.x_mts, fs.y_mts) == pytest.approx(sn.om.nse_aoi_mts(xe, ye), rel=1e-10)
                assert fs.fi_aoi_toi() == sn.om.fi_aoi_toi(xe, ye, 0, v_tol)
    finally:
        res.close()
        proj.close()


def test_refield_serves_a_lag_tolerance(lib):
    """t_tol > 0 is the refield route's: the fused kernel refuses it, the chain's metrics kernel evaluates it."""
    from gpras_amd.sweep import ModeCountSweep

    state, mean, var, truth, ranges = sn.make_case(70, 5, [12, 9], "wse", seed=4)
    x = sn.truth_in_metric_space(state, truth)
    proj = _projector(state)
    sweep = ModeCountSweep(proj, [2, 5])
    with pytest.raises(ValueError, match="t_tol = 0 only"):
        sweep.evaluate(mean, var, x, ranges, v_tol=0.1, t_tol=2, route="fused")
    res = sweep.evaluate(mean, var, x, ranges, v_tol=0.1, t_tol=2, route="refield")
    for k in (2, 5):
        xm, ym, _ = sn.metric_fields(state, k, mean, var, truth)
        for i, (lo, hi) in enumerate(ranges):
            assert res.summary(k, i).fi_aoi_toi() == sn.om.fi_aoi_toi(xm[lo:hi], ym[lo:hi], 2, 0.1)
    res.close()
    proj.close()


# ---- DevicePipeline.mode_count_sweep against one export_metric_summary per truncated pipeline ------------------------------------------
@pytest.mark.parametrize("hp,route", [("wse", "fused"), ("depth", "fused"), ("velocity", "fused"), ("wse", "refield")])
def test_pipeline_sweep_writes_the_tables_of_the_truncated_pipelines(lib, tmp_path, hp, route):
    from gpras_amd.pipeline import DevicePipeline
    from test_gpu_pipeline import _setup

    rng = np.random.default_rng(31)
    gpr, proj, x_test, truth_df, _ = _setup(hp, 16, rng, k=5)
    counts = [1, 3, 5]
    cells = truth_df.shape[1]
    with DevicePipeline(gpr, proj).mode_count_sweep(x_test, truth_df, counts, v_tol=0.1, route=route) as res:
        assert res.names == ["e1", "e2"] and res.ranges == [(0, 20), (20, 37)]
        paths = res.export(tmp_path / "spatial_mode_count", truth_df.index, truth_df.columns, depth_threshold=0.5, hydraulic_parameter=hp)
        table = res.scalar_table(depth_threshold=0.5, hydraulic_parameter=hp)
    assert list(table["spatial_mode_count"]) == [1, 1, 3, 3, 5, 5]
    g = gamma(cells - 1)
    for pos, k in enumerate(counts):
        part = copy.copy(gpr)
        part.models = gpr.models[:k]
        sub = proj.truncate(k)
        want_db = tmp_path / f"want_{k}.db"
        fields = DevicePipeline(part, sub).export_metric_summary(x_test, truth_df, want_db, depth_threshold=0.5, t_tol=0, v_tol=0.1, hydraulic_parameter=hp)
        y, conf = fields.to_host()
        fields.close()
        sub.close()
        x = truth_df.values.copy()
        if hp != "velocity":
            x = sn.wse_2_depth(x, proj.elevations)
        e = (x - y).astype(np.longdouble)
        mean_bound = {"err_aoi_ts": 2 * g * np.abs(e).sum(axis=1) / cells, "conf_aoi_ts": 2 * g * conf.astype(np.longdouble).sum(axis=1) / cells}
        ms = (e * e).sum(axis=1) / cells
        for name in ("scalar_metrics", "timeseries_metrics", "cell_metrics"):
            with sqlite3.connect(paths[pos]) as con:
                got = pd.read_sql(f"select * from {name}", con)
            with sqlite3.connect(want_db) as con:
                want = pd.read_sql(f"select * from {name}", con)
            assert list(got.columns) == list(want.columns) and len(got) == len(want)
            for col in want.columns:
                a, b = got[col].values, want[col].values
                if col in ("event", "cell_id"):
                    assert list(a) == list(b)
                elif col in ("err_aoi_ts", "conf_aoi_ts"):
                    # a mean over the cells: the sums' bound over `cells`, and one rounding of each division
                    _within(a, b, mean_bound[col] + 2 * U * np.abs(b.astype(np.longdouble)))
                elif col == "rmse_aoi_ts":
                    # sqrt(S / cells) with |dS| <= 2 gamma sum e^2 = 2 gamma S: the root moves by at most (gamma + 2u) of itself to first
                    # order; 2 (gamma + 2u) also covers the second-order term and the roundings of the division and the root
                    _within(a, b, 2 * (g + 2 * U) * np.sqrt(ms) + 4 * U * np.abs(b.astype(np.longdouble)))
                elif name == "scalar_metrics" and col in ("rmse_aoi_toi", "mae_aoi_toi", "conf_aoi_toi", "err_aoi_toi"):
                    # totals of the sums above over the event's rows, in two orders (mae: over the cells' sums): (rows + cells) terms at most
                    _within(a, b, 4 * gamma(cells + 20) * {"rmse_aoi_toi": np.abs(b), "mae_aoi_toi": np.abs(b), "conf_aoi_toi": np.abs(b),
                                                            "err_aoi_toi": np.array([np.abs(e[lo:hi]).mean() for lo, hi in ((0, 20), (20, 37))])}[col].astype(np.longdouble))
                else:
                    assert np.array_equal(a.astype(float), b.astype(float), equal_nan=True), (name, col)
            if name == "scalar_metrics":
                sub_table = table[table["spatial_mode_count"] == k].drop(columns="spatial_mode_count").reset_index(drop=True)
                pd.testing.assert_frame_equal(sub_table, got, check_exact=True, check_dtype=False)


# ---- argument checks of the C ABI ------------------------------------------------------------------------------------------------
def test_sweep_argument_checks(lib):
    from gpras_amd import _lib
    from gpras_amd._lib import DeviceBuffer, ptr
    from gpras_amd.preprocess import EOFProjector

    rows, cells, k = 12, 9, 4
    state, mean, var, truth, _ = sn.make_case(cells, k, [rows], "wse", seed=2)
    proj = _projector(state)
    bare = EOFProjector(np.zeros(cells, dtype=bool), None, state["input_mean"], None, state["eofs"], state["x_mean"], state["x_std"], "velocity")
    d_mean, d_var, d_truth = (DeviceBuffer.from_array(a) for a in (mean, var, sn.truth_in_metric_space(state, truth)))
    out = [DeviceBuffer(8 * 4 * 2 * 6 * cells), DeviceBuffer(4 * 4 * 2 * cells), DeviceBuffer(8 * 2 * cells), DeviceBuffer(4 * 2 * cells), DeviceBuffer(8 * 4 * rows * 3)]
    matches = np.zeros((4, 2), dtype=np.uint64)

    def call(handle=proj.handle, mean=d_mean.ptr, var=d_var.ptr, n_rows=rows, truth=d_truth.ptr, lo=(0, 6), hi=(6, 12), counts=(1, 4), n_counts=None,
             depth=1, v_tol=0.0, outs=None, m=ptr(matches), n_events=None):
        lo_a, hi_a, cnt = np.array(lo, dtype=np.int64), np.array(hi, dtype=np.int64), np.array(counts, dtype=np.int32)
        o = [b.ptr for b in out] if outs is None else outs
        return lib.gprx_pca_sweep_dev(handle, mean, var, n_rows, truth, len(lo) if n_events is None else n_events, ptr(lo_a), ptr(hi_a),
                                      len(counts) if n_counts is None else n_counts, ptr(cnt), depth, v_tol, o[0], o[1], o[2], o[3], o[4], m)

    bad = {
        "null handle": dict(handle=None), "no mean": dict(mean=None), "missing truth": dict(truth=None), "no rows": dict(n_rows=0),
        "unsorted counts": dict(counts=(3, 2)), "repeated count": dict(counts=(2, 2)), "count of zero": dict(counts=(0, 2)),
        "count beyond k": dict(counts=(1, 5)), "no counts": dict(n_counts=0), "too many counts": dict(n_counts=65),
        "overlapping events": dict(lo=(0, 5), hi=(6, 12)), "empty event": dict(lo=(0, 6), hi=(6, 6)), "event past the rows": dict(lo=(0, 6), hi=(6, 13)),
        "negative event": dict(lo=(-1, 6), hi=(6, 12)), "no events": dict(n_events=0), "unknown depth mode": dict(depth=3),
        "depth mode without elevations": dict(handle=bare.handle, depth=1), "negative v_tol": dict(v_tol=-0.5), "NaN v_tol": dict(v_tol=float("nan")),
        "no matches": dict(m=None), "no row sums": dict(outs=[b.ptr for b in out[:4]] + [None]), "no cell sums": dict(outs=[None] + [b.ptr for b in out[1:]]),
    }
    try:
        for what, kwargs in bad.items():
            assert call(**kwargs) == _lib.GPRX_EINVAL, what
            assert _lib.last_error(), what
        msg = {"unsorted counts": "strictly increasing", "overlapping events": "overlap", "missing truth": "truth", "depth mode without elevations": "elevations"}
        for what, text in msg.items():
            call(**bad[what])
            assert text in _lib.last_error(), (what, _lib.last_error())
        # the handles stay usable; the events may come in any order
        assert call() == _lib.GPRX_OK and call(lo=(6, 0), hi=(12, 6)) == _lib.GPRX_OK
        assert call(handle=bare.handle, depth=0) == _lib.GPRX_OK
        assert 0 < matches.sum() <= 2 * 2 * rows * cells or matches.sum() == 0
    finally:
        for b in [d_mean, d_var, d_truth, *out]:
            b.free()
        proj.close()
        bare.close()
