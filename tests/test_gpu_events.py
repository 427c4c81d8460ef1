"""EventSelector on the device (gprx_ev_*, csrc/events.h) against the fixture recorded from the reference's own ``EventSelection``
(tests/golden/make_golden_events_ref.py) and against the numpy restatement (tests/events_numpy.py).

``event_max`` is held to the fixture BIT FOR BIT: maxima are exact, and the return periods are IEEE operations in scipy's order.  The
standardised scores are held to 16 x ``score_dev_two_routes`` of the fixture (the difference of two CPU routes to the same matrix; 16 is
the margin for a third summation order over E terms on the same conditioning).  Picks are compared index for index: the generator
asserted that every pick beats its runner-up by 1e-6 relative, seven orders above that bound."""

import ctypes as C
import json
import os
import sys

import numpy as np
import pandas as pd
import pytest
from scipy.interpolate import interp1d

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import events_numpy as en  # noqa: E402
from make_golden_events_ref import CASES, align_signs, events_ref_cases  # noqa: E402  (it reads the reference only in main())

from gpras_amd import _lib  # noqa: E402
from gpras_amd._lib import DeviceBuffer, ptr  # noqa: E402
from gpras_amd.events import TIMING_NAMES, EventSelector  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "events_ref_golden.npz"))
INPUTS = events_ref_cases()
COLS = ("event_id", "datetime", "precip_excess", "precip_cum", "inflow")
_SELECTORS = {}


def selector(name, **kw):
    c = INPUTS[name]
    return EventSelector(*(c[k] for k in COLS), arrival_rate=c["arrival_rate"], test_rp_range=c["test_rp_range"], **kw)


def shared(name):
    """One EventSelector per case for the whole module: its tables are computed once."""
    if name not in _SELECTORS:
        _SELECTORS[name] = selector(name)
    return _SELECTORS[name]


def score_error(name, scores):
    rows, want = GOLDEN[f"{name}/scores_rows"], GOLDEN[f"{name}/scores"]
    return float(np.max(np.abs(align_signs(want, scores[rows]) - want)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_event_max_bit_for_bit(name):
    em = shared(name).event_max
    assert list(em.columns) == ["event_id", "precip-cum", "inflow", "RP_precip-cum", "RP_inflow"]
    assert np.array_equal(em["event_id"].to_numpy(), GOLDEN[f"{name}/event_max/event_id"])
    for col in ("precip-cum", "inflow", "RP_precip-cum", "RP_inflow"):
        got, want = em[col].to_numpy(), GOLDEN[f"{name}/event_max/{col}"]
        assert np.array_equal(got, want), f"{name} {col}: {np.count_nonzero(got != want)} values differ, worst {np.max(np.abs(got - want)):.3e}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_scores_against_the_reference(name):
    scores = shared(name).diverse_scores(INPUTS[name]["n_components"])
    err, two = score_error(name, scores), float(GOLDEN[f"{name}/score_dev_two_routes"])
    print(f"{name}: device scores differ from the reference's by {err:.3e}; the two CPU routes by {two:.3e}; bound {16 * two:.3e}")
    assert scores.shape == (INPUTS[name]["n_events"], 2 * INPUTS[name]["n_components"])
    assert err <= 16.0 * two


@pytest.mark.parametrize("name", sorted(CASES))
def test_selection_end_to_end(name):
    c, sel = INPUTS[name], shared(name)
    aep = sel.select_aep(c["target_rps"])
    assert np.array_equal(aep["event_id"].to_numpy(dtype=np.float64), GOLDEN[f"{name}/aep/event_id"])
    order = GOLDEN[f"{name}/diverse/order"]
    diverse = sel.select_diverse(aep["event_id"].tolist(), order.size, c["n_components"])
    assert np.array_equal(sel.diverse_order_, order)
    assert np.array_equal(diverse["event_id"].to_numpy(), GOLDEN[f"{name}/diverse/event_id"])
    assert set(diverse["Set"]) == {"Diverse"} and set(diverse["Type"]) == {"Train"}
    assert np.all(np.diff(sel.diverse_distance_) <= 0.0) and np.all(sel.diverse_distance_ > 0.0)
    # the recorded distances: those of the restatement on the device's own scores, one square root each
    rows = np.unique(np.searchsorted(sel.ids, aep["event_id"].to_numpy()))
    picks, dist = en.farthest(sel.diverse_scores(c["n_components"]), rows, order.size)
    assert np.array_equal(sel.ids[picks], order) and np.array_equal(dist, sel.diverse_distance_)
    selected, em = sel.run_selection(c["n_train"], c["n_test"], c["target_rps"])
    assert np.array_equal(selected["event_id"].to_numpy(dtype=np.float64), GOLDEN[f"{name}/run/event_id"])
    assert list(selected["Set"]) == list(GOLDEN[f"{name}/run/set"]) and list(selected["Type"]) == list(GOLDEN[f"{name}/run/type"])
    assert em is sel.event_max


def test_row_order_independence():
    """Case A with its rows permuted: the same bits everywhere."""
    c, base = INPUTS["A"], shared("A")
    perm = np.random.default_rng(3).permutation(c["event_id"].size)
    other = EventSelector(*(c[k][perm] for k in COLS), arrival_rate=c["arrival_rate"], test_rp_range=c["test_rp_range"])
    try:
        for col in base.event_max.columns:
            assert np.array_equal(other.event_max[col].to_numpy(), base.event_max[col].to_numpy()), col
        assert np.array_equal(other.diverse_scores(5), base.diverse_scores(5))
        aep = base.select_aep(c["target_rps"])["event_id"].tolist()
        other.select_diverse(aep, 6)
        base.select_diverse(aep, 6)
        assert np.array_equal(other.diverse_order_, base.diverse_order_) and np.array_equal(other.diverse_distance_, base.diverse_distance_)
    finally:
        other.close()


@pytest.mark.parametrize("which", ["precip-cum", "inflow"])
def test_return_period_outside_the_knots(which):
    sel = shared("A")
    mx = sel.event_max[which].to_numpy()
    xk, yk = en.knots(mx, sel.arrival_rate)
    span = xk[-1] - xk[0]
    values = np.concatenate([xk[0] - span * np.array([2.0, 0.5, 1e-3, 1e-9]), [np.nextafter(xk[0], -np.inf), xk[0], xk[3], 0.5 * (xk[4] + xk[5]), xk[-1],
                             np.nextafter(xk[-1], np.inf)], xk[-1] + span * np.array([1e-9, 1e-3, 0.7, 30.0])])
    want = interp1d(xk, yk, bounds_error=False, fill_value="extrapolate")(values)
    got = sel.return_period(which, values)
    assert np.array_equal(got, want), (got - want)
    assert got[0] < yk[0] and got[-1] > yk[-1]


def test_device_eigensolver_option():
    c = INPUTS["A"]
    sel, base = selector("A", eigensolver="device"), shared("A")
    try:
        scores = sel.diverse_scores(c["n_components"])
        err, two = score_error("A", scores), float(GOLDEN["A/score_dev_two_routes"])
        print(f"A, eigensolver='device': scores differ from the reference's by {err:.3e}; bound {16 * two:.3e}; sweeps {sel.last_eig_sweeps}")
        assert err <= 16.0 * two
        aep = base.select_aep(c["target_rps"])["event_id"].tolist()
        order = GOLDEN["A/diverse/order"]
        sel.select_diverse(aep, order.size)
        assert np.array_equal(sel.diverse_order_, order)
        assert sel.last_eig_sweeps >= 1
    finally:
        sel.close()


def test_timings_and_close():
    sel = selector("C")
    sel.select_diverse([int(sel.ids[0])], 3)
    ms = sel.stage_timings_ms()
    assert tuple(ms) == TIMING_NAMES and all(v >= 0.0 for v in ms.values())
    assert ms["pivot_maxima"] > 0.0 and ms["farthest"] > 0.0 and ms["cov_inflow"] > 0.0
    first = sel.diverse_order_.copy()
    sel.close()
    sel.close()
    assert isinstance(sel.event_max, pd.DataFrame)  # computed tables outlive the device state
    sel.select_diverse([int(sel.ids[0])], 3)  # and the device state comes back when it is needed
    assert np.array_equal(sel.diverse_order_, first)
    sel.close()


# ---- errors that only the device sees -------------------------------------------------------------------------------------------------
def test_abi_rejects_a_repeated_pair_and_a_gap(lib):
    vals = np.arange(6, dtype=np.float64)
    for rank, hour, text in (([0, 0, 0, 1, 1, 1], [0, 1, 1, 0, 1, 2], "pairs must be unique: 1 rows"), ([0, 0, 1, 1, 1], [0, 2, 0, 1, 2], "not exactly 0 .. len - 1"),
                             ([0, 0, 0, 1, 1, 2], [0, 1, 2, 0, 1, 0], "outside"), ([0, 0, 0, 1, 1, 1], [0, 1, 3, 0, 1, 2], "outside")):
        h = C.c_void_p()
        n = len(rank)
        rank, hour = np.array(rank, dtype=np.int32), np.array(hour, dtype=np.int32)  # (kept alive over the call)
        rc = lib.gprx_ev_create(0, n, 2, 3, ptr(rank), ptr(hour), ptr(vals), ptr(vals), ptr(vals), C.byref(h))
        assert rc == _lib.GPRX_EINVAL and not h.value and text in _lib.last_error(), (rc, _lib.last_error())
    h = C.c_void_p()
    rank, hour = np.array([0, 0, 1, 1], dtype=np.int32), np.array([0, 0, 0, 1], dtype=np.int32)  # (0, 0) twice, (0, 1) never: len 1 + 2 != 4 rows
    rc = lib.gprx_ev_create(0, 4, 2, 2, ptr(rank), ptr(hour), ptr(vals[:4]), ptr(vals[:4]), ptr(vals[:4]), C.byref(h))
    assert rc == _lib.GPRX_EINVAL and "pairs must be unique" in _lib.last_error(), _lib.last_error()


def test_one_distinct_block_maximum():
    """Thirty events with the same maxima: three blocks, one knot."""
    n_events, n_hours = 30, 4
    event_id = np.repeat(np.arange(n_events), n_hours)
    dt = np.datetime64("2026-01-01", "ns") + (np.tile(np.arange(n_hours), n_events) * 3600 * 10**9).astype("timedelta64[ns]")
    v = np.tile(np.array([0.0, 1.0, 2.0, 1.5]), n_events)
    with EventSelector(event_id, dt, v, v, v) as sel:
        with pytest.raises(ValueError, match="at least two distinct block maxima"):
            sel.event_max


def test_negative_maxima_survive_the_zero_fill():
    """Ragged events whose inflow stays below zero: the zeros of the pivot beyond an event's length must not become its maximum."""
    rng = np.random.default_rng(8)
    lengths = rng.integers(1, 9, size=40)
    lengths[5] = 8
    event_id = np.repeat(np.arange(40), lengths)
    hours = np.concatenate([np.arange(n) for n in lengths])
    dt = np.datetime64("2026-01-01", "ns") + (hours * 3600 * 10**9).astype("timedelta64[ns]")
    q = -1.0 - rng.random(event_id.size)
    with EventSelector(event_id, dt, rng.random(event_id.size), -q, q) as sel:
        em = sel.event_max
        want = np.array([q[event_id == e].max() for e in range(40)])
        assert np.array_equal(em["inflow"].to_numpy(), want) and np.all(want < 0.0)


# ---- the selection kernel alone ----------------------------------------------------------------------------------------------------------
def run_farthest(lib, handle, scores, selected, num):
    scores = np.ascontiguousarray(scores, dtype=np.float64)
    n, d = scores.shape
    buf = DeviceBuffer.from_array(scores)
    try:
        sel = np.ascontiguousarray(selected, dtype=np.int32)
        picks, dist = np.empty(num, dtype=np.int32), np.empty(num)
        rc = lib.gprx_ev_farthest(handle, buf.ptr, n, d, ptr(sel), sel.size, num, ptr(picks), ptr(dist))
        assert rc == _lib.GPRX_OK, _lib.last_error()
        return picks, dist
    finally:
        buf.free()


@pytest.fixture(scope="module")
def empty_handle(lib):
    h = C.c_void_p()
    assert lib.gprx_ev_create_empty(0, C.byref(h)) == _lib.GPRX_OK
    yield h
    lib.gprx_ev_destroy(h)


# 262221: past 1024 workgroups of 256 rows, where a workgroup walks more than one strip of rows
FARTHEST_SHAPES = [(n, d) for n in (2, 63, 64, 65, 1023, 1024, 1025, 70001) for d in (1, 2, 10, 64)] + [(262221, 1), (262221, 2)]


@pytest.mark.parametrize("n,d", FARTHEST_SHAPES)
def test_farthest_kernel_alone(lib, empty_handle, n, d):
    rng = np.random.default_rng([n, d])
    random = rng.standard_normal((n, d))
    lattice = rng.integers(0, 3, size=(n, d)).astype(np.float64)  # exact squared distances, ties everywhere
    few = min(5, n - 1)
    many = min(300, n // 2)
    plans = [(1, few), (1, 1)]
    if 60 < n < 2000:
        plans += [(n - few, few), (1, many), (n - many, many)]
    for data, what in ((random, "random"), (lattice, "lattice")):
        for n_sel, num in plans:
            selected = rng.choice(n, size=n_sel, replace=False)
            picks, dist = run_farthest(lib, empty_handle, data, selected, num)
            want, want_dist = en.farthest(data, selected, num)
            assert np.array_equal(picks, want), f"{what} n={n} d={d} n_sel={n_sel} num={num}: first difference at pick {int(np.argmax(picks != want))}"
            assert np.array_equal(dist, want_dist), f"{what} n={n} d={d}: distances"
            assert len(set(picks.tolist()) | set(selected.tolist())) == num + n_sel


def test_farthest_lowest_row_on_a_forced_tie(lib, empty_handle):
    """Four corners of a square and its centre selected: all four tie exactly, then the remaining ones tie again."""
    pts = np.array([[0.0, 0.0], [2.0, 2.0], [-2.0, 2.0], [2.0, -2.0], [-2.0, -2.0], [0.0, 3.0]])
    picks, dist = run_farthest(lib, empty_handle, pts, [0], 5)
    assert picks.tolist() == [5, 3, 4, 1, 2] == en.farthest(pts, [0], 5)[0].tolist()
    same = np.ones((70, 3))
    picks, dist = run_farthest(lib, empty_handle, same, [69], 69)
    assert picks.tolist() == list(range(69)) and np.all(dist == 0.0)


def test_farthest_rejects_bad_arguments(lib, empty_handle):
    buf = DeviceBuffer.from_array(np.zeros((8, 2)))
    picks, dist = np.empty(8, dtype=np.int32), np.empty(8)

    one = np.zeros(1, dtype=np.int32)

    def call(n, d, selected, num):
        sel = np.array(selected, dtype=np.int32)
        return lib.gprx_ev_farthest(empty_handle, buf.ptr, n, d, ptr(sel) if sel.size else ptr(one), sel.size, num, ptr(picks), ptr(dist))

    try:
        for args, text in (((8, 2, [], 1), "non-empty"), ((8, 2, [0, 1], 7), "number of candidates"), ((8, 65, [0], 1), "d <= 64"), ((8, 2, [8], 1), "outside"),
                           ((8, 2, [3, 3], 1), "twice"), ((1, 2, [0], 1), "n < 2^31"), ((8, 2, [0], 0), "number of candidates")):
            assert call(*args) == _lib.GPRX_EINVAL and text in _lib.last_error(), (args, _lib.last_error())
        assert lib.gprx_ev_farthest(empty_handle, None, 8, 2, ptr(one), 1, 1, ptr(picks), ptr(dist)) == _lib.GPRX_ESTATE
    finally:
        buf.free()
