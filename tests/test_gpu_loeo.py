"""Leave-one-event-out predictions (gprx_loeo_batch, gpras_amd/loeo.py) against their longdouble definition of tests/loeo_reference.py:
the downdate kernel and the refactor route on every case, the routes told apart, bit-identity across batch and event list,
include_noise, the models the kernel does not take, and GPRAS.leave_event_out after a fit.  A result may be off by 8 x what a float64
restatement of its route reaches on the same data (tests/golden/loeo_bounds.json); every comparison prints its figures first."""

import numpy as np
import pytest

import loeo_reference as lr
from gpras_amd import _lib, loeo
from gpras_amd.engine import Engine
from gpras_amd.gpr import GPRAS

pytestmark = pytest.mark.gpu


class Fitted:
    """What gpras_amd.loeo reads of a fitted GPRAS, with a case's stated hyperparameters in the place of an optimiser's."""

    class Mode:
        def __init__(self, backend, unit, theta, z):
            self.backend, self.unit, self._theta, self.Z = backend, unit, theta, z

        def theta(self):
            return self._theta

    def __init__(self, cid, cells=None):
        c = lr.CASES[cid]
        x, y, zs = lr.data(cid)
        self.kernel_str, self.ard, self.distance_form, self.device = c.kernel, c.ard, c.form, 0
        self.x, self.y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        self.engine = Engine(c.kernel, self.x, self.y, c.m, ard=c.ard, distance_form=c.form)
        th = lr.thetas(cid)
        cells = range(len(c.hypers)) if cells is None else cells
        self.models = [self.Mode(self.engine, cell, th[cell], None if zs is None else zs[cell]) for cell in cells]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.engine.close()


@pytest.fixture(scope="module")
def results():
    """{(cid, route): (mean, var)} of every case, each (n, cells): computed once, read-only."""
    out = {}
    for cid, c in lr.CASES.items():
        with Fitted(cid) as f:
            for route in c.routes:
                mean, var = loeo.leave_event_out(f, c.events, route=route)
                assert f.last_loeo_route == route
                if route == "downdate":
                    assert f.engine.last_loeo()[0]
                mean.setflags(write=False)
                var.setflags(write=False)
                out[cid, route] = (mean, var)
    return out


def hold(mean, var, cid, cell, route, what):
    ref_mean, ref_var = lr.loeo_ld(cid, cell)
    inside = lr.event_mask(cid)
    assert not np.any(np.isnan(mean[inside])) and not np.any(np.isnan(var[inside])), f"{what}: NaN at the rows of an event"
    assert np.all(np.isnan(mean[~inside])) and np.all(np.isnan(var[~inside])), f"{what}: a row of no event is not NaN"
    em, ev = lr.mean_err(cid, mean, ref_mean), lr.var_err(cid, var, ref_var)
    am, av = lr.allowed(cid, cell, route, "mean"), lr.allowed(cid, cell, route, "var")
    print(f"{what} [{cid}/c{cell}/{route}]: mean {em:.3e} = {em / am * lr.MARGIN:.2f} x ratio, var {ev:.3e} = {ev / av * lr.MARGIN:.2f} x ratio")
    assert em <= am, f"{what}: mean off by {em:.3e}, allowed {am:.3e}"
    assert ev <= av, f"{what}: var off by {ev:.3e}, allowed {av:.3e}"


@pytest.mark.parametrize("cid", list(lr.CASES))
def test_both_routes_against_the_longdouble_definition(results, cid):
    c = lr.CASES[cid]
    for route in c.routes:
        mean, var = results[cid, route]
        assert mean.shape == var.shape == (c.n, len(c.hypers))
        for cell in range(len(c.hypers)):
            hold(mean[:, cell], var[:, cell], cid, cell, route, "leave_event_out")


@pytest.mark.parametrize("cid", lr.DOWNDATE_CASES)
def test_the_downdate_is_not_the_refactor_route(results, cid):
    """Both are within rounding of the definition, by different arithmetic: equal bits would mean one route ran twice."""
    down, ref = results[cid, "downdate"], results[cid, "refactor"]
    assert not np.array_equal(down[0], ref[0], equal_nan=True) and not np.array_equal(down[1], ref[1], equal_nan=True)


@pytest.mark.parametrize("cid", ["M70", "EXACT"])
def test_auto_takes_the_refactor_route_where_the_kernel_does_not_apply(results, cid):
    c = lr.CASES[cid]
    with Fitted(cid) as f:
        mean, var = loeo.leave_event_out(f, c.events, route="auto")
        assert f.last_loeo_route == "refactor" and not f.engine.last_loeo()[0]
        assert np.array_equal(mean, results[cid, "refactor"][0], equal_nan=True) and np.array_equal(var, results[cid, "refactor"][1], equal_nan=True)
        with pytest.raises(ValueError):
            loeo.leave_event_out(f, c.events, route="downdate")
        # the C ABI refuses the same models itself
        th, zs = lr.thetas(cid), lr.data(cid)[2]
        with pytest.raises(ValueError):
            f.engine.loeo_batch([0], th[:1], None if zs is None else zs[:1], c.events)
        assert not f.engine.last_loeo()[0]


def test_auto_takes_the_downdate_where_it_applies(results):
    c = lr.CASES["M5"]
    with Fitted("M5") as f:
        mean, var = loeo.leave_event_out(f, c.events)
        assert f.last_loeo_route == "downdate" and f.engine.last_loeo()[0]
        assert np.array_equal(mean, results["M5", "downdate"][0], equal_nan=True) and np.array_equal(var, results["M5", "downdate"][1], equal_nan=True)


@pytest.mark.parametrize("cid", ["M50", "TILE"])
def test_a_mode_alone_and_an_event_in_a_shorter_list_give_the_same_bits(results, cid):
    c = lr.CASES[cid]
    full_mean, full_var = results[cid, "downdate"]
    th, zs = lr.thetas(cid), lr.data(cid)[2]
    with Fitted(cid) as f:
        for cell in (0, len(c.hypers) - 1):  # a mode alone against the same mode inside the batch
            mean, var, status = f.engine.loeo_batch([cell], th[cell : cell + 1], zs[cell : cell + 1], c.events)
            assert not status.any()
            assert np.array_equal(mean[0], full_mean[:, cell], equal_nan=True) and np.array_equal(var[0], full_var[:, cell], equal_nan=True)
        # every second event, and the last one alone: other tiles, other columns of a tile, the same bits at the rows that remain
        for subset in (c.events[1::2], c.events[-1:]):
            mean, var, status = f.engine.loeo_batch(list(range(len(c.hypers))), th, zs, subset)
            assert status.shape == (len(c.hypers), len(subset)) and not status.any()
            inside = np.zeros(c.n, dtype=bool)
            for lo, hi in subset:
                inside[lo:hi] = True
                assert np.array_equal(mean[:, lo:hi].T, full_mean[lo:hi]) and np.array_equal(var[:, lo:hi].T, full_var[lo:hi])
            assert np.all(np.isnan(mean[:, ~inside])) and np.all(np.isnan(var[:, ~inside]))


def test_include_noise_adds_exactly_the_noise(results):
    cid = "M50"
    c = lr.CASES[cid]
    with Fitted(cid) as f:
        mean, var = loeo.leave_event_out(f, c.events, route="downdate", include_noise=False)
    inside = lr.event_mask(cid)
    assert np.array_equal(mean, results[cid, "downdate"][0], equal_nan=True)
    for cell in range(len(c.hypers)):
        v, _, s = lr.hyper(cid, cell)
        # the kernel adds the noise last: var_y IS var_f + s, to the bit, at the library's own s (the softplus of theta as the library
        # evaluates it: the longdouble one rounded to double, or the double beside it)
        var_y, var_f = results[cid, "downdate"][1][inside, cell], var[inside, cell]
        assert any(np.array_equal(var_y, var_f + sd) for sd in (s, np.nextafter(s, 0.0), np.nextafter(s, 1.0))), np.max(np.abs(var_y - var_f - s))
    assert np.all(np.isnan(var[~inside]))


def test_the_c_abi_refuses_bad_ranges_before_any_device_work(lib):
    """Straight through ctypes (Engine.loeo_batch checks the ranges itself before it calls)."""
    import ctypes as C

    cid = "M5"
    c = lr.CASES[cid]
    th, zs = lr.thetas(cid), lr.data(cid)[2]
    units = np.zeros(1, dtype=np.int32)
    with Fitted(cid) as f:
        h = f.engine._h
        mean, var = np.zeros((1, c.n)), np.zeros((1, c.n))
        for ranges in ([(10, 20), (15, 30)], [(30, 40), (10, 20)], [(10, 10)], [(0, c.n + 1)], [(-1, 5)], [(0, lr.TILE + 1)]):
            lo = np.array([r[0] for r in ranges], dtype=np.int64)
            hi = np.array([r[1] for r in ranges], dtype=np.int64)
            status = np.zeros((1, len(ranges)), dtype=np.int32)
            rc = lib.gprx_loeo_batch(h, 1, _lib.ptr(units), _lib.ptr(th[:1]), _lib.ptr(zs[:1]), len(ranges), _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(mean),
                                     _lib.ptr(var), 1, _lib.ptr(status))
            assert rc == _lib.GPRX_EINVAL, (ranges, rc)
            ran = C.c_int(1)
            assert lib.gprx_last_loeo(h, C.byref(ran), None) == _lib.GPRX_OK and ran.value == 0
        assert not mean.any() and not var.any()


def test_fit_then_leave_event_out_equals_the_engine_call():
    cid = "M5"
    c = lr.CASES[cid]
    x, y, _ = lr.data(cid)
    n = 260
    labels = np.repeat(np.arange(4), 65)
    gpr = GPRAS("RBF")
    gpr.fit(x[:n], y[:n], 5, optimization_method="adam", max_iter=5)
    mean, var = gpr.leave_event_out(labels)
    assert gpr.last_loeo_route == "downdate"
    assert mean.shape == var.shape == (n, y.shape[1]) and np.all(np.isfinite(mean)) and np.all(var > 0)
    units = [m.unit for m in gpr.models]
    thetas, zs = np.stack([m.theta() for m in gpr.models]), np.stack([m.Z for m in gpr.models])
    em, ev, status = gpr.engine.loeo_batch(units, thetas, zs, [(65 * e, 65 * e + 65) for e in range(4)])
    assert not status.any() and np.array_equal(mean, em.T) and np.array_equal(var, ev.T)
    rmse, nlpd = loeo.event_scores(gpr.y, mean, var, [(65 * e, 65 * e + 65) for e in range(4)])
    assert rmse.shape == nlpd.shape == (4, y.shape[1]) and np.all(np.isfinite(rmse)) and np.all(np.isfinite(nlpd))
    for eng in gpr.engines:
        eng.close()
