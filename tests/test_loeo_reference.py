"""The longdouble leave-one-event-out definition of loeo_reference.py against the float64 oracle on the reduced data, the recorded bounds
against their script, and the host side of gpras_amd/loeo.py: event resolution, the argument checks (which raise before any library
call) and event_scores.  CPU only."""

import importlib.util
import os

import numpy as np
import pandas as pd
import pytest

import loeo_reference as lr
from gpras_amd import _lib, loeo
from oracle import exact as oex
from oracle import sgpr as osg

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the definition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["M5", "M50", "ARD", "K-diff", "K-exp", "M70", "EXACT"])
def test_longdouble_definition_is_the_oracle_on_the_reduced_data(cid):
    """Per event: oracle.sgpr.predict (gpflow's SGPR.predict_y restated) of the model on the rows outside the event, at the event's rows."""
    c = lr.CASES[cid]
    x, y, zs = lr.data(cid)
    form = "direct" if c.form == "difference" else "expanded"
    for cell in (0, len(c.hypers) - 1):
        v, ls, s = lr.hyper(cid, cell)
        ls_arg = ls if c.ard else float(ls[0])
        ref_mean, ref_var = lr.loeo_ld(cid, cell)
        got_mean, got_var = np.full(c.n, np.nan), np.full(c.n, np.nan)
        for lo, hi in c.events:
            keep = lr.kept_rows(c.n, lo, hi)
            if c.m:
                got_mean[lo:hi], got_var[lo:hi] = osg.predict(c.kernel, x[keep], y[keep, cell], zs[cell], v, ls_arg, s, x[lo:hi], True, form=form)
            else:
                got_mean[lo:hi], got_var[lo:hi] = oex.predict(c.kernel, x[keep], y[keep, cell], v, ls_arg, s, x[lo:hi], True)
        assert lr.mean_err(cid, got_mean, ref_mean) <= 1e-9 and lr.var_err(cid, got_var, ref_var) <= 1e-9
        inside = lr.event_mask(cid)
        assert np.all(np.isnan(ref_mean[~inside].astype(np.float64))) and not np.any(np.isnan(ref_mean[inside].astype(np.float64)))


def test_the_downdate_formulas_give_the_definition():
    """H = I - t2 t2^T / s, c' = Lh^-1 (c - t2 y / s), W = Lh^-1 t2 in float64 against the longdouble refit: rounding apart, the same."""
    for cid in ("M5", "M64"):
        for cell in range(len(lr.CASES[cid].hypers)):
            mean, var = lr.emu_downdate(cid, cell)
            ref_mean, ref_var = lr.loeo_ld(cid, cell)
            assert lr.mean_err(cid, mean, ref_mean) <= 1e-10 and lr.var_err(cid, var, ref_var) <= 1e-10


def test_the_cases_cover_what_they_claim():
    lengths = {hi - lo for lo, hi in lr.BASE_EVENTS}
    assert {1, 3, 63, 64, 65, 300} <= lengths
    assert lr.BASE_EVENTS[0][0] > 0 and any(a[1] < b[0] for a, b in zip(lr.BASE_EVENTS, lr.BASE_EVENTS[1:])) and lr.BASE_EVENTS[-1][1] < 700
    t = lr.CASES["TILE"]
    assert t.events[1][1] - t.events[0][0] <= lr.TILE < t.events[2][1] - t.events[0][0]  # two events share the first tile, the third does not fit
    assert lr.CASES["M70"].m > loeo.DOWNDATE_MAX_M and lr.CASES["EXACT"].m == 0
    for cid, c in lr.CASES.items():
        x, y, zs = lr.data(cid)
        assert all(np.array_equal(a * 2.0 ** 20, np.rint(a * 2.0 ** 20)) for a in (x, y) + (() if zs is None else (zs,)))
        lo, hi = loeo.check_event_ranges(c.events, c.n)
        assert lo.size == len(c.events)


def test_recorded_bounds_are_what_the_script_writes():
    spec = importlib.util.spec_from_file_location("make_loeo_bounds", os.path.join(HERE, "golden", "make_loeo_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(lr.BOUNDS_PATH) as fh:
        assert fh.read() == mod.render()


def test_every_allowed_error_stays_inside_the_baseline_tolerance():
    """8 x the recorded ratio is at most 1e-8 for every case, cell, route and quantity; a case that needs more is a badly chosen case."""
    b = lr.bounds()
    assert b and all(lr.U <= r and lr.MARGIN * r <= 1e-8 for r in b.values()), max(b, key=b.get)
    expected = {f"{cid}/c{cell}/{route}/{q}" for cid, c in lr.CASES.items() for cell in range(len(c.hypers)) for route in c.routes for q in ("mean", "var")}
    assert set(b) == expected


def test_no_reference_variance_is_a_cancelled_number():
    for cid, c in lr.CASES.items():
        for cell in range(len(c.hypers)):
            assert float(np.min(lr.loeo_ld(cid, cell)[1][lr.event_mask(cid)])) >= lr.hyper(cid, cell)[2], (cid, cell)


# ---- events ----------------------------------------------------------------------------------------------------------------------------
def test_events_as_ranges_labels_and_pandas_index():
    want = ([0, 3, 5], [3, 5, 9])
    labels = np.array(["a"] * 3 + ["b"] * 2 + ["c"] * 4)
    index = pd.MultiIndex.from_arrays([labels, np.arange(9)], names=["event", "timestep"])
    for events in ([(0, 3), (3, 5), (5, 9)], np.array([[0, 3], [3, 5], [5, 9]]), labels, list(labels), [7, 7, 7, 2, 2, 5, 5, 5, 5], index):
        lo, hi = loeo.resolve_events(events, 9)
        assert lo.dtype == hi.dtype == np.int64 and lo.tolist() == want[0] and hi.tolist() == want[1]
    lo, hi = loeo.resolve_events([(2, 4), (6, 9)], 9)  # rows 0-1 and 4-5 belong to no event
    assert lo.tolist() == [2, 6] and hi.tolist() == [4, 9]


@pytest.mark.parametrize("events", [
    [(0, 5), (3, 8)],           # overlapping
    [(5, 8), (0, 3)],           # unsorted
    [(0, 3), (3, 3)],           # empty
    [(0, 10)],                  # outside [0, N]
    [(-1, 3)],
    [],
    ["a", "a", "b", "a", "a", "c", "c", "c", "c"],  # the rows of "a" are not one run
    ["a", "b"],                 # not one label per row
])
def test_bad_events_raise(events):
    with pytest.raises(ValueError):
        loeo.resolve_events(events, 9)


# ---- argument checks come before any library call ---------------------------------------------------------------------------------------
class _Untouchable:
    """A backend whose every use fails the test."""

    def __getattr__(self, name):
        if name == "loeo_batch":  # (hasattr: the downdate is offered)
            return self._fail
        raise AssertionError(f"backend.{name} touched before the arguments were checked")

    def _fail(self, *a, **k):
        raise AssertionError("the library was called")


class _Mode:
    def __init__(self, unit, z):
        self.unit, self.Z, self.backend = unit, z, _Untouchable()

    def theta(self):
        return np.zeros(3)


class _Gpr:
    kernel_str, ard, distance_form, device = "RBF", False, "difference", 0

    def __init__(self, n=40, d=3, m=8, k=2):
        rng = np.random.default_rng(0)
        self.x, self.y = rng.standard_normal((n, d)), rng.standard_normal((n, k))
        self.models = [_Mode(u, None if m is None else rng.standard_normal((m, d))) for u in range(k)]


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", refuse)


@pytest.mark.parametrize("events", [[(0, 5), (3, 8)], [(5, 8), (0, 3)], [(0, 3), (3, 3)], [0] * 10 + [1] * 10 + [0] * 20])
def test_bad_events_raise_before_any_library_call(no_library, events):
    for route in loeo.ROUTES:
        with pytest.raises(ValueError):
            loeo.leave_event_out(_Gpr(), events, route=route)


@pytest.mark.parametrize("kw, why", [(dict(m=70), "inducing"), (dict(m=None), "exact"), (dict(d=65), "features")])
def test_downdate_on_a_model_it_does_not_take_raises_before_any_library_call(no_library, kw, why):
    with pytest.raises(ValueError, match=why):
        loeo.leave_event_out(_Gpr(**kw), [(0, 10), (10, 40)], route="downdate")


def test_an_event_longer_than_a_tile_is_not_for_the_downdate(no_library):
    gpr = _Gpr(n=loeo.DOWNDATE_MAX_ROWS + 2, d=1, k=1)
    with pytest.raises(ValueError, match="rows"):
        loeo.leave_event_out(gpr, [(0, loeo.DOWNDATE_MAX_ROWS + 1)], route="downdate")
    assert loeo.downdate_applies(gpr, np.array([0]), np.array([loeo.DOWNDATE_MAX_ROWS])) is None


def test_unknown_route_and_unfitted_model_raise(no_library):
    with pytest.raises(ValueError):
        loeo.leave_event_out(_Gpr(), [(0, 10)], route="fast")
    gpr = _Gpr()
    gpr.models = []
    with pytest.raises(ValueError):
        loeo.leave_event_out(gpr, [(0, 10)])


# ---- scores ------------------------------------------------------------------------------------------------------------------------------
def test_event_scores_against_a_direct_evaluation():
    rng = np.random.default_rng(3)
    n, k = 50, 3
    y, mean, var = rng.standard_normal((n, k)), rng.standard_normal((n, k)), rng.uniform(0.1, 2.0, (n, k))
    ranges = [(0, 1), (1, 20), (25, 50)]
    rmse, nlpd = loeo.event_scores(y, mean, var, ranges)
    assert rmse.shape == nlpd.shape == (3, k)
    for e, (lo, hi) in enumerate(ranges):
        for j in range(k):
            r = y[lo:hi, j] - mean[lo:hi, j]
            assert rmse[e, j] == pytest.approx(np.sqrt(np.mean(r ** 2)), rel=1e-14)
            dens = np.exp(-0.5 * r ** 2 / var[lo:hi, j]) / np.sqrt(2 * np.pi * var[lo:hi, j])
            assert nlpd[e, j] == pytest.approx(-np.mean(np.log(dens)), rel=1e-12)
    with pytest.raises(ValueError):
        loeo.event_scores(y, mean[:, :2], var, ranges)
