"""The blocked leave-one-event-out route (gprx_loeo_batch_blocked, gpras_amd/loeo.py route "blocked": sparse models with M <= 320) against
the longdouble definition of tests/loeo_blocked_reference.py: every case within 8 x what a float64 restatement of the route reaches on
the same data (tests/golden/loeo_blocked_bounds.json), the route told apart from the refactor route and from the one-workgroup
downdate, bit-identity across batch, event list, group size and repeated calls, include_noise, the arguments the C entry point refuses,
and GPRAS.leave_event_out after a fit.  Every comparison prints its figures first."""

import ctypes as C

import numpy as np
import pytest

import loeo_blocked_reference as br
from gpras_amd import _lib, loeo
from gpras_amd.engine import Engine
from gpras_amd.gpr import GPRAS

pytestmark = pytest.mark.gpu

REFACTOR_TOO = ("B65", "B130", "B70T")  # cases that also run the refactor route (an Engine per event)


class Fitted:
    """What gpras_amd.loeo reads of a fitted GPRAS, with a case's stated hyperparameters in the place of an optimiser's."""

    class Mode:
        def __init__(self, backend, unit, theta, z):
            self.backend, self.unit, self._theta, self.Z = backend, unit, theta, z

        def theta(self):
            return self._theta

    def __init__(self, cid):
        c = br.CASES[cid]
        x, y, zs = br.data(cid)
        self.kernel_str, self.ard, self.distance_form, self.device = c.kernel, False, c.form, 0
        self.x, self.y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        self.engine = Engine(c.kernel, self.x, self.y, c.m, ard=False, distance_form=c.form)
        th = br.thetas(cid)
        self.models = [self.Mode(self.engine, cell, th[cell], zs[cell]) for cell in range(len(c.hypers))]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.engine.close()


@pytest.fixture(scope="module")
def results():
    """{(cid, route): (mean, var)} of every case, each (n, cells): computed once, read-only."""
    out = {}
    for cid, c in br.CASES.items():
        with Fitted(cid) as f:
            for route in ("blocked",) + (("refactor",) if cid in REFACTOR_TOO else ()):
                mean, var = loeo.leave_event_out(f, c.events, route=route)
                assert f.last_loeo_route == route
                if route == "blocked":
                    ran, groups, stages = f.engine.last_loeo_blocked()
                    assert ran and groups >= 1 and set(stages) == {"factorize_ms", "head_ms", "gram_ms", "chol_inverse_ms", "apply_ms", "total_ms"}
                    assert not f.engine.last_loeo()[0]  # the reporter of the other entry point keeps to its own calls
                mean.setflags(write=False)
                var.setflags(write=False)
                out[cid, route] = (mean, var)
    return out


def hold(mean, var, cid, cell, route, what):
    ref_mean, ref_var = br.loeo_ld(cid, cell)
    inside = br.event_mask(cid)
    assert not np.any(np.isnan(mean[inside])) and not np.any(np.isnan(var[inside])), f"{what}: NaN at the rows of an event"
    assert np.all(np.isnan(mean[~inside])) and np.all(np.isnan(var[~inside])), f"{what}: a row of no event is not NaN"
    em, ev = br.mean_err(cid, mean, ref_mean), br.var_err(cid, var, ref_var)
    am, av = br.allowed(cid, cell, route, "mean"), br.allowed(cid, cell, route, "var")
    print(f"{what} [{cid}/c{cell}/{route}]: mean {em:.3e} = {em / am * br.MARGIN:.2f} x ratio, var {ev:.3e} = {ev / av * br.MARGIN:.2f} x ratio")
    assert em <= am, f"{what}: mean off by {em:.3e}, allowed {am:.3e}"
    assert ev <= av, f"{what}: var off by {ev:.3e}, allowed {av:.3e}"


@pytest.mark.parametrize("cid", list(br.CASES))
def test_the_blocked_route_against_the_longdouble_definition(results, cid):
    c = br.CASES[cid]
    for route in ("blocked", "refactor"):
        if (cid, route) not in results or (route == "refactor" and cid != "B70T"):
            continue
        mean, var = results[cid, route]
        assert mean.shape == var.shape == (c.n, len(c.hypers))
        for cell in range(len(c.hypers)):
            hold(mean[:, cell], var[:, cell], cid, cell, route, "leave_event_out")


@pytest.mark.parametrize("cid", ["B65", "B130"])
def test_the_blocked_route_is_not_the_refactor_route(results, cid):
    """Both are within rounding of the definition, by different arithmetic: equal bits would mean one route ran twice."""
    blk, ref = results[cid, "blocked"], results[cid, "refactor"]
    assert not np.array_equal(blk[0], ref[0], equal_nan=True) and not np.array_equal(blk[1], ref[1], equal_nan=True)


def test_one_band_through_both_downdates(results):
    """B50 (mp = 64): the blocked route and the one-workgroup kernel on the same fitted object, each inside its own bound, each reporter
    telling of its own call only."""
    cid = "B50"
    c = br.CASES[cid]
    with Fitted(cid) as f:
        assert not f.engine.last_loeo()[0] and not f.engine.last_loeo_blocked()[0]
        mean, var = loeo.leave_event_out(f, c.events, route="downdate")
        assert f.last_loeo_route == "downdate" and f.engine.last_loeo()[0] and not f.engine.last_loeo_blocked()[0]
        for cell in range(len(c.hypers)):
            hold(mean[:, cell], var[:, cell], cid, cell, "downdate", "downdate on the blocked case")
        bmean, bvar = loeo.leave_event_out(f, c.events, route="blocked")
        assert f.last_loeo_route == "blocked" and f.engine.last_loeo_blocked()[0]
        assert np.array_equal(bmean, results[cid, "blocked"][0], equal_nan=True) and np.array_equal(bvar, results[cid, "blocked"][1], equal_nan=True)
        for cell in range(len(c.hypers)):
            hold(bmean[:, cell], bvar[:, cell], cid, cell, "blocked", "blocked beside the downdate")
        assert f.engine.last_loeo()[0]  # (the blocked call did not reset the other reporter)


@pytest.mark.parametrize("cid", ["B130", "B320"])
def test_batch_event_list_groups_and_repeats_give_the_same_bits(results, cid):
    c = br.CASES[cid]
    full_mean, full_var = results[cid, "blocked"]
    th, zs = br.thetas(cid), br.data(cid)[2]
    cells = list(range(len(c.hypers)))
    with Fitted(cid) as f:
        eng = f.engine
        for cell in cells:  # a mode alone against the same mode inside the batch of two
            mean, var, status = eng.loeo_batch_blocked([cell], th[cell : cell + 1], zs[cell : cell + 1], c.events)
            assert not status.any()
            assert np.array_equal(mean[0], full_mean[:, cell], equal_nan=True) and np.array_equal(var[0], full_var[:, cell], equal_nan=True)
        # every second event, and the last one alone: other columns of the tile, other slots, the same bits at the rows that remain
        for subset in (c.events[1::2], c.events[-1:]):
            mean, var, status = eng.loeo_batch_blocked(cells, th, zs, subset)
            assert status.shape == (len(cells), len(subset)) and not status.any()
            inside = np.zeros(c.n, dtype=bool)
            for lo, hi in subset:
                inside[lo:hi] = True
                assert np.array_equal(mean[:, lo:hi].T, full_mean[lo:hi]) and np.array_equal(var[:, lo:hi].T, full_var[lo:hi])
            assert np.all(np.isnan(mean[:, ~inside])) and np.all(np.isnan(var[:, ~inside]))
        # one event per group against the default (every event of the tile in one group)
        mean, var, status = eng.loeo_batch_blocked(cells, th, zs, c.events, max_slots=len(cells))
        ran, groups, _ = eng.last_loeo_blocked()
        assert ran and groups == len(c.events) > 1 and not status.any()
        assert np.array_equal(mean.T, full_mean, equal_nan=True) and np.array_equal(var.T, full_var, equal_nan=True)
        # fewer slots than cells: a group still holds one event
        mean, var, status = eng.loeo_batch_blocked(cells, th, zs, c.events, max_slots=1)
        assert eng.last_loeo_blocked()[1] == len(c.events)
        assert np.array_equal(mean.T, full_mean, equal_nan=True) and np.array_equal(var.T, full_var, equal_nan=True)
        # the default again: one group, and the same bits as the first call
        mean, var, status = eng.loeo_batch_blocked(cells, th, zs, c.events)
        assert eng.last_loeo_blocked()[:2] == (True, 1)
        assert np.array_equal(mean.T, full_mean, equal_nan=True) and np.array_equal(var.T, full_var, equal_nan=True)


def test_include_noise_adds_exactly_the_noise(results):
    cid = "B130"
    c = br.CASES[cid]
    with Fitted(cid) as f:
        mean, var = loeo.leave_event_out(f, c.events, route="blocked", include_noise=False)
    inside = br.event_mask(cid)
    assert np.array_equal(mean, results[cid, "blocked"][0], equal_nan=True)
    for cell in range(len(c.hypers)):
        _, _, s = br.hyper(cid, cell)
        # the kernel adds the noise last: var_y IS var_f + s, to the bit, at the library's own s (the longdouble softplus rounded to
        # double, or the double beside it)
        var_y, var_f = results[cid, "blocked"][1][inside, cell], var[inside, cell]
        assert any(np.array_equal(var_y, var_f + sd) for sd in (s, np.nextafter(s, 0.0), np.nextafter(s, 1.0))), np.max(np.abs(var_y - var_f - s))
    assert np.all(np.isnan(var[~inside]))


def _refused(lib, eng, n, m, d, ranges):
    """gprx_loeo_batch_blocked straight through ctypes on one cell: (return code, `ran` afterwards, outputs untouched)."""
    rng = np.random.default_rng(5)
    units = np.zeros(1, dtype=np.int32)
    th = np.zeros((1, 3))
    zs = None if m == 0 else np.ascontiguousarray(rng.standard_normal((1, m, d)))
    lo = np.array([r[0] for r in ranges], dtype=np.int64)
    hi = np.array([r[1] for r in ranges], dtype=np.int64)
    mean, var = np.zeros((1, n)), np.zeros((1, n))
    status = np.zeros((1, len(ranges)), dtype=np.int32)
    rc = lib.gprx_loeo_batch_blocked(eng._h, 1, _lib.ptr(units), _lib.ptr(th), None if zs is None else _lib.ptr(zs), len(ranges), _lib.ptr(lo),
                                     _lib.ptr(hi), _lib.ptr(mean), _lib.ptr(var), 1, 0, _lib.ptr(status))
    ran, groups = C.c_int(1), C.c_int(1)
    assert lib.gprx_last_loeo_blocked(eng._h, C.byref(ran), C.byref(groups), None) == _lib.GPRX_OK
    return rc, ran.value, groups.value, not mean.any() and not var.any() and not status.any()


@pytest.mark.parametrize("what, m, d", [("exact", 0, 3), ("mp = 384", 330, 3), ("d = 65", 8, 65)])
def test_the_c_abi_refuses_models_it_does_not_take_before_any_device_work(lib, what, m, d):
    n = 400
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal((n, d)), rng.standard_normal((n, 1))
    eng = Engine("RBF", x, y, m)
    try:
        rc, ran, groups, untouched = _refused(lib, eng, n, m, d, [(0, 100), (100, 250)])
        assert rc == _lib.GPRX_EINVAL and ran == 0 and groups == 0 and untouched, (what, rc)
    finally:
        eng.close()


def test_the_c_abi_refuses_bad_ranges_before_any_device_work(lib):
    cid = "B70T"  # (4200 rows: an event of 4097 fits the data)
    c = br.CASES[cid]
    with Fitted(cid) as f:
        for ranges in ([(10, 20), (15, 30)], [(30, 40), (10, 20)], [(10, 10)], [(0, c.n + 1)], [(-1, 5)], [(0, br.TILE + 1)]):
            rc, ran, groups, untouched = _refused(lib, f.engine, c.n, c.m, c.d, ranges)
            assert rc == _lib.GPRX_EINVAL and ran == 0 and groups == 0 and untouched, (ranges, rc)


def test_fit_then_leave_event_out_equals_the_engine_call():
    x, y, _ = br.data("B130")
    n = 400
    events = [(100 * e, 100 * e + 100) for e in range(4)]
    gpr = GPRAS("RBF")
    gpr.fit(x[:n], y[:n], 100, optimization_method="adam", max_iter=5)
    try:
        mean, var = gpr.leave_event_out(np.repeat(np.arange(4), 100), route="blocked")
        assert gpr.last_loeo_route == "blocked"
        assert mean.shape == var.shape == (n, y.shape[1]) and np.all(np.isfinite(mean)) and np.all(var > 0)
        units = [m.unit for m in gpr.models]
        thetas, zs = np.stack([m.theta() for m in gpr.models]), np.stack([m.Z for m in gpr.models])
        em, ev, status = gpr.engine.loeo_batch_blocked(units, thetas, zs, events)
        assert not status.any() and np.array_equal(mean, em.T) and np.array_equal(var, ev.T)
        # "auto" keeps to the refactor route for more than 64 inducing points (figures of the two routes side by side, not a check:
        # the bounds of the cases above are the check)
        amean, avar = gpr.leave_event_out(events)
        assert gpr.last_loeo_route == "refactor" and amean.shape == mean.shape
        print(f"blocked against refactor after a fit: mean {np.max(np.abs(amean - mean)):.3e}, var {np.max(np.abs(avar - var) / avar):.3e}")
    finally:
        for eng in gpr.engines:
            eng.close()
