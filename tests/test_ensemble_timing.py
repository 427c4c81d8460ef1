"""The event timing of a peak ensemble on the host: the numpy mirror (ensemble_timing_numpy.py) against a plain triple loop, the rules of
the definitions (the sentinel, the strict compare, NaN rows), ``EventTiming``'s arithmetic from hand-made counts, and the argument checks of
``evaluate`` and ``timing_stats`` (gpras_amd.ensemble)."""

import numpy as np
import pytest

import ensemble_timing_numpy as et
import sweep_numpy as sn
from gpras_amd import ensemble as ge


def _loops(y, thr):
    """The definitions written out: one member, one cell, one row at a time, with the rule of the device's running maximum."""
    members, rows, cells = y.shape
    n_thr = len(thr)
    peak = np.zeros((members, cells))
    timing = np.zeros((members, 1 + 2 * n_thr, cells), dtype=np.int32)
    for s in range(members):
        for c in range(cells):
            pk, tpk = y[s, 0, c], 0
            for t in range(1, rows):
                v = y[s, t, c]
                if not (pk != pk) and (v > pk or v != v):
                    pk, tpk = v, t
            peak[s, c], timing[s, 0, c] = pk, tpk
            for j, th in enumerate(thr):
                hit = [t for t in range(rows) if y[s, t, c] > th]
                timing[s, 1 + j, c] = len(hit)
                timing[s, 1 + n_thr + j, c] = hit[0] if hit else rows
    return peak, timing


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_mirror_against_the_loops():
    rng = np.random.default_rng(0)
    y = np.round(rng.normal(size=(3, 7, 5)), 1)  # rounded: ties within a column, so "the first maximum" and "strictly above" both bite
    y[1, 3, 2] = np.nan
    y[2, :, 4] = 0.3
    thr = [0.0, 0.3, -np.inf, np.inf, float(y[0, 2, 1])]
    peak, timing = et.field_timing(y, thr)
    want_peak, want = _loops(y, thr)
    assert _same(peak, want_peak) and np.array_equal(timing, want) and timing.dtype == np.int32
    assert et.field_timing(y, ())[1].shape == (3, 1, 5) and np.array_equal(et.field_timing(y, ())[1][:, 0], want[:, 0])
    # one row: the peak is row 0, an arrival is 0 or the sentinel 1
    _, one = et.field_timing(y[:, :1], [0.0])
    assert not one[:, 0].any() and np.array_equal(one[:, 2], np.where(y[:, 0] > 0.0, 0, 1)) and np.array_equal(one[:, 1], 1 - one[:, 2])


def test_the_rules():
    y = np.array([[0.1, 0.5, 0.5, np.nan, 0.9, 0.2]]).T[None]  # one member, six rows, one cell
    peak, t = et.field_timing(y, [0.5, 0.2, 1.0, -np.inf])
    assert np.isnan(peak[0, 0]) and t[0, 0, 0] == 3  # a NaN is the maximum and sticks: the later 0.9 does not replace it
    assert t[0, 1:5, 0].tolist() == [1, 3, 0, 5]  # strict: the two 0.5 rows are not above 0.5; the NaN row counts for nothing, not even -inf
    assert t[0, 5:9, 0].tolist() == [4, 1, 6, 0]  # the sentinel is the row count where no row exceeds
    peak, t = et.field_timing(np.array([[0.5, 0.7, 0.7, 0.1]]).T[None], [0.6])
    assert peak[0, 0] == 0.7 and t[0, :, 0].tolist() == [1, 2, 1]  # the FIRST maximum
    # consistency: arrival < rows <=> duration > 0 <=> peak > thr, and duration <= rows - arrival
    rng = np.random.default_rng(1)
    y = rng.normal(size=(4, 9, 6))
    thr = [-0.5, 0.0, 1.5, 3.0]
    peak, t = et.field_timing(y, thr)
    for j, th in enumerate(thr):
        dur, arr = t[:, 1 + j], t[:, 1 + len(thr) + j]
        assert np.array_equal(arr < 9, dur > 0) and np.array_equal(dur > 0, peak > th) and np.all(dur <= 9 - arr)


def test_member_timing_through_the_chain():
    state, *_ = sn.make_case(12, 3, [6], "depth", dry=(2,), seed=4)
    scores = np.random.default_rng(5).normal(size=(2, 6, 3))
    peak, timing = et.member_timing(state, scores, [0.0, 0.5])
    import ensemble_numpy as en

    y = en.member_fields(state, scores)
    assert np.array_equal(peak, en.member_peaks(state, scores)) and np.array_equal(timing[:, 0], np.argmax(y, axis=1))
    assert not timing[:, 1:3, 2].any() and np.all(timing[:, 3:5, 2] == 6)  # the dry cell never gets wet


def test_statistics_mirror():
    rng = np.random.default_rng(2)
    members, cells, rows = 9, 7, 12
    v = rng.integers(0, rows + 1, size=(members, 2, cells))
    v[:, 0, 0] = rows  # every member at the sentinel
    v[:, 1, 1] = 3
    obs = rng.integers(0, rows + 1, size=(2, cells))
    st = et.timing_stats(v, sentinel=rows, levels=(-1, 0, 3, rows - 1, rows), ranks=(0, 4, 8), obs=obs)
    for m in range(2):
        for c in range(cells):
            col = v[:, m, c].tolist()
            assert st["cdf"][m, :, c].tolist() == [sum(x <= lv for x in col) for lv in (-1, 0, 3, rows - 1, rows)]
            assert st["n_valid"][m, c] == sum(x != rows for x in col) and st["sum"][m, c] == sum(x for x in col if x != rows)
            assert st["order"][m, :, c].tolist() == [sorted(col)[r] for r in (0, 4, 8)]
            assert st["below"][m, c] == sum(x < obs[m, c] for x in col) and st["equal"][m, c] == sum(x == obs[m, c] for x in col)
    assert st["n_valid"][0, 0] == 0 and st["sum"][0, 0] == 0 and st["order"][0, :, 0].tolist() == [rows] * 3
    assert st["cdf"][0, 0].tolist() == [0] * cells and st["cdf"][0, 4].tolist() == [members] * cells
    plain = et.timing_stats(v)
    assert np.array_equal(plain["n_valid"], np.full((2, cells), members)) and np.array_equal(plain["sum"], v.sum(axis=0))
    assert plain["cdf"].shape == (2, 0, cells) and plain["order"].shape == (2, 0, cells) and plain["below"] is None


def test_event_timing_arithmetic():
    s, cells = 4, 3
    z = np.zeros
    tm = ge.EventTiming(
        t_peak_sum=np.array([[0, 6, 10]]), t_peak_quantiles=z((1, 1, cells), dtype=np.int32),
        duration_sum=np.array([[[0, 5, 16]]]), duration_quantiles=z((1, 1, 1, cells), dtype=np.int32),
        duration_below_counts=np.array([[[[0, 1, 4], [4, 3, 0]]]]),  # D = durations[0], durations[1]
        arrival_counts=np.array([[[0, 3, 4]]]), arrival_sum=np.array([[[0, 7, 2]]]), arrival_quantiles=z((1, 1, 1, cells), dtype=np.int32),
        arrival_by_counts=np.array([[[[0, 1, 4]]]]), rows=np.array([5]), members=s, thresholds=np.array([0.5]), quantiles=np.array([0.5]),
        durations=np.array([1, 4]), arrive_by=np.array([2]))
    assert tm.t_peak_mean.tolist() == [[0.0, 1.5, 2.5]]
    assert tm.duration_mean.tolist() == [[[0.0, 1.25, 4.0]]]
    assert tm.p_duration_at_least.tolist() == [[[[1.0, 0.75, 0.0], [0.0, 0.25, 1.0]]]]  # 1 - cdf(D - 1) / S
    assert tm.p_arrival.tolist() == [[[0.0, 0.75, 1.0]]]  # n_valid / S
    am = tm.arrival_mean
    assert np.isnan(am[0, 0, 0]) and am[0, 0, 1] == 7 / 3 and am[0, 0, 2] == 0.5  # over the members that arrive; NaN where none does
    assert tm.p_arrival_by.tolist() == [[[[0.0, 0.25, 1.0]]]]
    assert tm.observed is None and tm.below is None and tm.equal is None and tm.names == []


def test_argument_checks():
    assert ge.timing_maps(0) == 1 and ge.timing_maps(8) == 17
    dur, by = ge.check_timing_args(True, (0.5,), (0, 3), np.array([5], dtype=np.int64))
    assert dur.dtype == by.dtype == np.int32 and dur.tolist() == [0, 3] and by.tolist() == [5]
    assert [a.size for a in ge.check_timing_args(False, ())] == [0, 0] and [a.size for a in ge.check_timing_args(True, (0.0,))] == [0, 0]
    for timing, thr, durations, arrive_by in ((True, (), (), ()), (True, (0.5,), np.arange(9), ()), (True, (0.5,), (), np.arange(9)),
                                              (True, (0.5,), (-1,), ()), (True, (0.5,), (), (-1,)), (True, (0.5,), (1.5,), ()),
                                              (True, (0.5,), (), (2.0,)), (True, (0.5,), (2**31 - 1,), ()), (True, (0.5,), [[1, 2]], ()),
                                              (False, (0.5,), (1,), ()), (False, (0.5,), (), (1,))):
        with pytest.raises(ValueError):
            ge.check_timing_args(timing, thr, durations, arrive_by)
    lv, rk = ge.check_timing_stats_args(17, 5, 1, 2, 33, 33, (-1, 0, 32), (0, 16))
    assert lv.dtype == rk.dtype == np.int32 and lv.tolist() == [-1, 0, 32] and rk.tolist() == [0, 16]
    ok = dict(members=4, n_maps=5, map0=0, n_sel=5, rows=10, sentinel=-1, levels=(), ranks=())
    ge.check_timing_stats_args(**ok)
    for change in (dict(members=0), dict(members=4097), dict(rows=0), dict(rows=2**31 - 1), dict(n_maps=0), dict(n_maps=18), dict(map0=-1), dict(n_sel=0),
                   dict(map0=1), dict(sentinel=-2), dict(sentinel=11), dict(levels=np.arange(9)), dict(levels=(0.5,)), dict(levels=(2**31,)),
                   dict(ranks=(4,)), dict(ranks=(-1,)), dict(ranks=np.arange(9) % 4), dict(ranks=(0.5,))):
        with pytest.raises(ValueError):
            ge.check_timing_stats_args(**{**ok, **change})
    # evaluate keeps its signature's defaults: nothing new happens unless asked for
    import inspect

    sig = inspect.signature(ge.PeakEnsemble.evaluate).parameters
    assert sig["timing"].default is False and sig["durations"].default == () and sig["arrive_by"].default == ()
    assert "timing" not in ge.STAGES
