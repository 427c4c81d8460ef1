"""Event selection on the CPU: the numpy restatement of the device path (tests/events_numpy.py) against the fixture recorded from the
reference's own ``EventSelection`` (tests/golden/make_golden_events_ref.py), the host-side selections of ``EventSelector`` against the
reference's frames, and every ``ValueError`` of the documented domain."""

import json
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import events_numpy as en  # noqa: E402
from make_golden_events_ref import CASES, align_signs, events_ref_cases, input_checksums  # noqa: E402  (it reads the reference only in main())

from gpras_amd import events as ev  # noqa: E402
from gpras_amd.events import EventSelector  # noqa: E402

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "events_ref_golden.npz"))
META = json.loads(str(GOLDEN["meta_json"]))
INPUTS = events_ref_cases()
RP_COLUMNS = ("precip-cum", "inflow", "RP_precip-cum", "RP_inflow")


def golden_event_max(name):
    return pd.DataFrame({c: GOLDEN[f"{name}/event_max/{c}"] for c in ("event_id",) + RP_COLUMNS})


def test_fixture_belongs_to_these_inputs():
    assert input_checksums(INPUTS) == META["input_checksums"]
    assert sorted(META["cases"]) == sorted(CASES)
    for name, c in INPUTS.items():
        assert (META["cases"][name]["E"], META["cases"][name]["H"]) == (c["n_events"], c["n_hours"])
        assert all(s != "randomized" for s in META["cases"][name]["solvers"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_event_max_bit_for_bit(name):
    c = INPUTS[name]
    ids, rank, hour = en.rank_and_hour(c["event_id"], c["datetime"])
    assert np.array_equal(ids, GOLDEN[f"{name}/event_max/event_id"])
    for col, key in (("precip_cum", "precip-cum"), ("inflow", "inflow")):
        mx = en.event_maxima(rank, c[col], ids.size)
        assert np.array_equal(mx, GOLDEN[f"{name}/event_max/{key}"])
        xk, yk = en.knots(mx, c["arrival_rate"])
        assert np.array_equal(en.rp_eval(xk, yk, mx), GOLDEN[f"{name}/event_max/RP_{key}"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_scores_and_picks(name):
    c = INPUTS[name]
    ids, rank, hour = en.rank_and_hour(c["event_id"], c["datetime"])
    E, H, k = ids.size, int(hour.max()) + 1, c["n_components"]
    scores = en.diverse_scores(en.pivot(rank, hour, c["precip_excess"], E, H), en.pivot(rank, hour, c["inflow"], E, H), k)
    rows, want = GOLDEN[f"{name}/scores_rows"], GOLDEN[f"{name}/scores"]
    err = float(np.max(np.abs(align_signs(want, scores[rows]) - want)))
    print(f"{name}: restatement scores differ from the reference's by {err:.3e}")
    assert err <= 16.0 * float(GOLDEN[f"{name}/score_dev_two_routes"])
    selected = np.unique(np.searchsorted(ids, GOLDEN[f"{name}/aep/event_id"]))
    order = GOLDEN[f"{name}/diverse/order"]
    picks, dist = en.farthest(scores, selected, order.size)
    assert np.array_equal(ids[picks], order)
    assert np.array_equal(np.sort(ids[picks]), GOLDEN[f"{name}/diverse/event_id"])
    assert np.all(np.diff(dist) <= 0.0)  # the min-distance of successive farthest points cannot grow


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_selections_from_event_max(name):
    c = INPUTS[name]
    sel = EventSelector.from_event_max(golden_event_max(name), arrival_rate=c["arrival_rate"], test_rp_range=c["test_rp_range"])
    aep = sel.select_aep(c["target_rps"])
    assert np.array_equal(aep["event_id"].to_numpy(dtype=np.float64), GOLDEN[f"{name}/aep/event_id"])
    assert np.array_equal(aep.index.to_numpy(), GOLDEN[f"{name}/aep/index"])
    assert list(aep["Set"]) == list(GOLDEN[f"{name}/aep/set"]) and set(aep["Type"]) == {"Train"}
    excluded = aep["event_id"].tolist() + GOLDEN[f"{name}/diverse/event_id"].tolist()
    test = sel.select_test(c["test_rp_range"], c["n_test"], excluded)
    assert np.array_equal(test["event_id"].to_numpy(), GOLDEN[f"{name}/test/event_id"])
    assert set(test["Set"]) == {"Test"} and set(test["Type"]) == {"Test"}
    with pytest.raises(RuntimeError, match="no long frame"):
        sel.diverse_scores()


def test_select_aep_on_negative_return_periods():
    """Case A holds extrapolated, negative return periods: their log distance is NaN and sorts last, as in the reference."""
    assert min(GOLDEN["A/event_max/RP_precip-cum"].min(), GOLDEN["A/event_max/RP_inflow"].min()) < 0.0


def test_rank_and_hour_matches_the_restatement():
    c = INPUTS["A"]
    ids, rank, hour, order = ev.rank_and_hour(c["event_id"], c["datetime"])
    ids2, rank2, hour2 = en.rank_and_hour(c["event_id"], c["datetime"])
    assert np.array_equal(ids, ids2) and np.array_equal(rank, rank2) and np.array_equal(hour, hour2)
    assert rank.dtype == np.int32 and hour.dtype == np.int32
    assert np.all(np.diff(c["event_id"][order]) >= 0)


# ---- the domain ---------------------------------------------------------------------------------------------------------------------------
def small_frame(n_events=30, n_hours=6):
    rng = np.random.default_rng(5)
    event_id = np.repeat(np.arange(n_events), n_hours)
    hours = np.tile(np.arange(n_hours), n_events)
    dt = np.datetime64("2026-01-01", "ns") + (hours * 3600 * 10**9).astype("timedelta64[ns]")
    return dict(event_id=event_id, datetime=dt, precip_excess=rng.random(event_id.size), precip_cum=rng.random(event_id.size), inflow=rng.random(event_id.size))


def test_non_finite_values_are_counted():
    f = small_frame()
    f["inflow"][[3, 17]] = [np.nan, np.inf]
    with pytest.raises(ValueError, match=r"'inflow' holds 2 non-finite"):
        EventSelector(**f)


def test_repeated_event_hour_pair():
    f = small_frame()
    f["datetime"][7] = f["datetime"][6]
    with pytest.raises(ValueError, match=r"pairs must be unique: 1 rows"):
        EventSelector(**f)


def test_empty_selection_and_too_many_picks():
    sel = EventSelector(**small_frame())
    with pytest.raises(ValueError, match="non-empty"):
        sel.select_diverse([], 3)
    with pytest.raises(ValueError, match="exceeds the number of candidates"):
        sel.select_diverse([0, 1], 29)
    with pytest.raises(ValueError, match="not among the events"):
        sel.select_diverse([1000], 2)


def test_too_many_components():
    sel = EventSelector(**small_frame(n_events=30, n_hours=6))
    with pytest.raises(ValueError, match=r"exceeds min\(E, H\)"):
        sel.diverse_scores(n_components=7)
    with pytest.raises(ValueError, match=r"exceeds min\(E, H\)"):
        EventSelector(**small_frame(n_events=4, n_hours=6)).diverse_scores(n_components=5)
    with pytest.raises(ValueError, match="n_components <= 32"):
        sel.diverse_scores(n_components=33)


def test_one_block_has_no_two_knots():
    sel = EventSelector(**small_frame(n_events=8), arrival_rate=10)
    with pytest.raises(ValueError, match="at least two distinct block maxima"):
        sel.event_max
    with pytest.raises(ValueError, match="at least two distinct block maxima"):
        en.knots(np.array([3.0, 1.0, 3.0, 2.0]), 2)  # two blocks, one value


def test_shape_bounds():
    ev.check_shape(ev.MAX_EVENTS, 1) if ev.MAX_EVENTS * 16 <= ev.MAX_CELLS else None
    with pytest.raises(ValueError, match="fewer than 2\\^31 events"):
        ev.check_shape(1 << 31, 1)
    with pytest.raises(ValueError, match="at most 4096"):
        ev.check_shape(10, 4097)
    with pytest.raises(ValueError, match="exceeds 2\\^28"):
        ev.check_shape((1 << 20) + 1, 256)
    ev.check_shape(1 << 20, 256)
    f = small_frame(n_events=2, n_hours=4097)
    with pytest.raises(ValueError, match="at most 4096"):
        EventSelector(**f)


def test_constructor_arguments():
    f = small_frame()
    with pytest.raises(ValueError, match="eigensolver"):
        EventSelector(**f, eigensolver="lapack")
    with pytest.raises(ValueError, match="arrival_rate"):
        EventSelector(**f, arrival_rate=0)
    with pytest.raises(ValueError, match="lacks the columns"):
        EventSelector.from_frame(pd.DataFrame({"event_id": [1]}))
