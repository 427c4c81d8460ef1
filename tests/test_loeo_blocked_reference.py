"""The longdouble leave-one-event-out definition of loeo_blocked_reference.py against the float64 oracle on the reduced data, the recorded
bounds against their script, and the host side of the "blocked" route of gpras_amd/loeo.py: the argument checks, which raise before any
library call.  No GPU."""

import importlib.util
import os

import numpy as np
import pytest

import loeo_blocked_reference as br
from gpras_amd import _lib, loeo
from oracle import sgpr as osg

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("cid", list(br.CASES))
def test_longdouble_definition_is_the_oracle_on_the_reduced_data(cid):
    """Per event: oracle.sgpr.predict of the model on the rows outside the event, at the event's rows."""
    c = br.CASES[cid]
    x, y, zs = br.data(cid)
    form = "direct" if c.form == "difference" else "expanded"
    for cell in range(len(c.hypers)):
        v, ls, s = br.hyper(cid, cell)
        ref_mean, ref_var = br.loeo_ld(cid, cell)
        got_mean, got_var = np.full(c.n, np.nan), np.full(c.n, np.nan)
        for lo, hi in c.events:
            keep = br.kept_rows(c.n, lo, hi)
            got_mean[lo:hi], got_var[lo:hi] = osg.predict(c.kernel, x[keep], y[keep, cell], zs[cell], v, float(ls[0]), s, x[lo:hi], True, form=form)
        assert br.mean_err(cid, got_mean, ref_mean) <= 1e-9 and br.var_err(cid, got_var, ref_var) <= 1e-9
        inside = br.event_mask(cid)
        assert np.all(np.isnan(ref_mean[~inside].astype(np.float64))) and not np.any(np.isnan(ref_mean[inside].astype(np.float64)))


def test_the_cases_cover_what_they_claim():
    assert {c.mp for c in br.CASES.values()} == {64, 128, 192, 320}
    assert br.CASES["B65"].m == 65 and br.CASES["B130"].mp // 64 == 3 and br.CASES["B320"].m == loeo.BLOCKED_MAX_M
    lengths = {hi - lo for lo, hi in br.EV400}
    assert {1, 63, 64, 65, 199} <= lengths and any(lo % 2 == 1 for lo, _ in br.EV400)
    t = br.CASES["B70T"]
    assert t.events[1][1] - t.events[0][0] <= br.TILE < t.events[2][1] - t.events[0][0]  # two events share the first tile, the third does not fit
    assert br.CASES["BM32"].form == "expanded" and br.CASES["BM32"].kernel == "Matern32"
    for cid, c in br.CASES.items():
        assert len(c.hypers) == 2 and c.d == 3
        lo, hi = loeo.check_event_ranges(c.events, c.n)
        assert lo.size == len(c.events) and (cid == "B70T" or not br.event_mask(cid).all())  # (rows of no event, but in the two-tile case)


def test_recorded_bounds_are_what_the_script_writes():
    spec = importlib.util.spec_from_file_location("make_loeo_blocked_bounds", os.path.join(HERE, "golden", "make_loeo_blocked_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(br.BOUNDS_PATH) as fh:
        assert fh.read() == mod.render()
    b = br.bounds()
    expected = {f"{cid}/c{cell}/{route}/{q}" for cid, c in br.CASES.items() for cell in range(len(c.hypers)) for route in c.routes for q in ("mean", "var")}
    assert set(b) == expected and all(br.U <= r for r in b.values())


# ---- argument checks come before any library call ---------------------------------------------------------------------------------------
class _Untouchable:
    """A backend whose every use fails the test."""

    def __getattr__(self, name):
        if name in ("loeo_batch", "loeo_batch_blocked"):  # (hasattr: both downdates are offered)
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


def test_blocked_is_a_route_of_its_own():
    assert loeo.ROUTES == ("auto", "downdate", "refactor", "blocked") and loeo.BLOCKED_MAX_M == 320 and loeo.DOWNDATE_MAX_M == 64


@pytest.mark.parametrize("kw, why", [(dict(m=None), "exact"), (dict(m=321), "inducing"), (dict(d=65), "features")])
def test_blocked_on_a_model_it_does_not_take_raises_before_any_library_call(no_library, kw, why):
    with pytest.raises(ValueError, match=why):
        loeo.leave_event_out(_Gpr(**kw), [(0, 10), (10, 40)], route="blocked")


@pytest.mark.parametrize("events", [[(0, 5), (3, 8)], [(5, 8), (0, 3)], [(0, 3), (3, 3)], [0] * 10 + [1] * 10 + [0] * 20])
def test_bad_events_raise_before_any_library_call(no_library, events):
    with pytest.raises(ValueError):
        loeo.leave_event_out(_Gpr(m=100), events, route="blocked")


def test_an_event_longer_than_a_tile_is_not_for_the_blocked_route(no_library):
    gpr = _Gpr(n=loeo.DOWNDATE_MAX_ROWS + 2, d=1, m=320, k=1)
    with pytest.raises(ValueError, match="rows"):
        loeo.leave_event_out(gpr, [(0, loeo.DOWNDATE_MAX_ROWS + 1)], route="blocked")
    assert loeo.blocked_applies(gpr, np.array([0]), np.array([loeo.DOWNDATE_MAX_ROWS])) is None


def test_the_downdate_still_refuses_more_than_64_inducing_points(no_library):
    gpr = _Gpr(m=70)
    assert "inducing" in loeo.downdate_applies(gpr, np.array([0]), np.array([10]))
    assert loeo.blocked_applies(gpr, np.array([0]), np.array([10])) is None
    with pytest.raises(ValueError, match="inducing"):
        loeo.leave_event_out(gpr, [(0, 10)], route="downdate")
