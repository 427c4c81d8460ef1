"""What the batched and single GP entry points do with ONE bad per-cell argument (gp_ctx.h decode_cells): the status code and the
message, the caller's output buffers, and the handle's state afterwards.

Shapes: n = 70 (np = 128 is ragged), d = 3, two units, kernels RBF and Matern32, ard 0 and 1 (ntheta 3 and 5: the faulty theta element
is the last lengthscale or the noise), exact (m = 0), sparse m = 5 (fused five-launch route) and m = 70 (general sequence, mp = 128);
three cells with the faulty one LAST.  One fault per call: unit -1, unit n_units, NaN theta, +inf theta, z null and NaN in the last
element of z (sparse handles).

Every refused call returns GPRX_EINVAL with the message of its fault and leaves its output buffers at the canary they were filled
with; the same valid call made before and after it returns the same bits.

Recorded as it is, not asserted (include/gprx.h): the optimiser entry points clear n_evals, batches and losses before they look at
the cells, and the host-stepped route counts the refused evaluation, so of their buffers only theta and z (in/out) are held to
"untouched"."""

import ctypes as C

import blocks_reference as br
import numpy as np
import pytest

from gpras_amd import _lib
from gpras_amd._lib import DeviceBuffer, check, ptr
from gpras_amd.synth import make_regression
from oracle import kernels as okn

pytestmark = pytest.mark.gpu

N, D, N_UNITS, CELLS, NS = 70, 3, 2, 3, 9
ALL = _lib.TRAIN_VARIANCE | _lib.TRAIN_LENGTHSCALE | _lib.TRAIN_NOISE | _lib.TRAIN_Z
UNITS = np.array([1, 0, 1], dtype=np.int32)

# fault -> (what the message must contain, needs a sparse handle)
FAULTS = {
    "unit_negative": ("unit out of range", False),
    "unit_n_units": ("unit out of range", False),
    "theta_nan": ("theta is not finite", False),
    "theta_inf": ("theta is not finite", False),
    "z_null": ("is null", True),
    "z_nan": ("z is not finite", True),
}


class Args:
    """The per-cell arguments of one call: units, theta (cells, ntheta), z (cells, m, d) or None."""

    def __init__(self, units, theta, z):
        self.units, self.theta, self.z = units, theta, z

    def first(self):
        return Args(self.units[:1].copy(), self.theta[:1].copy(), None if self.z is None else self.z[:1].copy())


def good_args(m, ard):
    rng = np.random.default_rng(5)
    theta = np.ascontiguousarray(rng.normal(0.2, 0.3, size=(CELLS, 2 + (D if ard else 1))))
    z = None
    if m:
        z = np.ascontiguousarray(rng.standard_normal((CELLS, m, D)))
    return Args(UNITS.copy(), theta, z)


def faulty(good, fault, cell):
    """`good` with one fault in cell `cell`: the LAST lengthscale (NaN) or the noise (+inf) of theta, the last element of z."""
    a = Args(good.units.copy(), good.theta.copy(), None if good.z is None else good.z.copy())
    if fault == "unit_negative":
        a.units[cell] = -1
    elif fault == "unit_n_units":
        a.units[cell] = N_UNITS
    elif fault == "theta_nan":
        a.theta[cell, -2] = np.nan
    elif fault == "theta_inf":
        a.theta[cell, -1] = np.inf
    elif fault == "z_null":
        a.z = None
    elif fault == "z_nan":
        a.z[cell, -1, -1] = np.nan
    return a


def zptr(a):
    return None if a.z is None else ptr(a.z)


def bits(*arrays):
    return [np.ascontiguousarray(a).view(np.uint8).copy() for a in arrays]


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b))


class Case:
    """One handle family: `CELLS` handles on the same data (gprx_factorize_many takes one handle per cell; the rest use the first)."""

    def __init__(self, lib, kernel, ard, m):
        self.lib, self.m, self.ard = lib, m, ard
        x, y, xs = make_regression(N, D, n_outputs=N_UNITS, n_test=NS, config=3, unit=11)
        self.xs = xs
        self.handles = (C.c_void_p * CELLS)()
        for c in range(CELLS if m == 0 else 1):
            h = C.c_void_p()
            check(lib.gprx_create(0, N, D, m, okn.KERNEL_IDS[kernel], ard, C.byref(h)))
            check(lib.gprx_set_data(h, ptr(x), ptr(y), N_UNITS), h)
            self.handles[c] = h
        self.h = C.c_void_p(self.handles[0])
        self.good = good_args(m, ard)
        self.gw = self.good.theta.shape[1] + m * D
        self.xs_dev = DeviceBuffer.from_array(xs)

    def close(self):
        self.xs_dev.free()
        for h in self.handles:
            if h:
                self.lib.gprx_destroy(C.c_void_p(h))

    # ---- entry points: each returns (status, handle of the message, output buffers, in/out buffers) ----
    def objective(self, a, grad=True):
        a = a.first() if a.units.size > 1 else a
        loss, g = br.canary(1), br.canary(self.gw)
        rc = self.lib.gprx_objective(self.h, int(a.units[0]), ptr(a.theta), zptr(a), ALL, loss.ctypes.data_as(C.POINTER(C.c_double)),
                                     ptr(g) if grad else None)
        return rc, self.h, [loss] + ([g] if grad else []), []

    def factorize(self, a):
        a = a.first() if a.units.size > 1 else a
        loss = br.canary(1)
        rc = self.lib.gprx_factorize(self.h, int(a.units[0]), ptr(a.theta), zptr(a), ALL, ptr(loss))
        return rc, self.h, [loss], []

    def factorize_many(self, a):
        losses = br.canary(CELLS)
        rc = self.lib.gprx_factorize_many(CELLS, self.handles, ptr(a.units), ptr(a.theta), ALL, ptr(losses))
        return rc, C.c_void_p(self.handles[CELLS - 1]), [losses], []

    def factorize_batch(self, a):
        losses, status = br.canary(CELLS), np.full(CELLS, -77, dtype=np.int32)
        rc = self.lib.gprx_factorize_batch(self.h, CELLS, ptr(a.units), ptr(a.theta), ALL, ptr(losses), ptr(status))
        return rc, self.h, [losses, status], []

    def objective_batch(self, a, grad=True):
        losses, grads = br.canary(CELLS), br.canary(CELLS * self.gw)
        rc = self.lib.gprx_objective_batch(self.h, CELLS, ptr(a.units), ptr(a.theta), zptr(a), ALL, ptr(losses), ptr(grads) if grad else None)
        return rc, self.h, [losses] + ([grads] if grad else []), []

    def optimizer(self, a, adam, max_iter=2, mask=ALL):
        theta, z = a.theta.copy(), None if a.z is None else a.z.copy()
        n_evals, batches = np.full(CELLS, -77, dtype=np.int32), C.c_int(-77)
        if adam:
            rc = self.lib.gprx_adam_batch(self.h, CELLS, ptr(a.units), ptr(theta), None if z is None else ptr(z), mask, max_iter, ptr(n_evals),
                                          C.byref(batches))
        else:
            losses = br.canary(CELLS)
            rc = self.lib.gprx_adadelta_batch(self.h, CELLS, ptr(a.units), ptr(theta), None if z is None else ptr(z), mask, max_iter, ptr(losses),
                                              ptr(n_evals), C.byref(batches))
        self.n_evals = n_evals
        return rc, self.h, [], [(theta, a.theta)] + ([] if z is None else [(z, a.z)])

    def predict_batch(self, a, which):
        fn = {"host": self.lib.gprx_predict_batch, "t": self.lib.gprx_predict_batch_t, "dev": self.lib.gprx_predict_batch_dev}[which]
        means, vars_ = br.canary(CELLS * NS), br.canary(CELLS * NS)
        if which == "dev":
            dm, dv = DeviceBuffer.from_array(means), DeviceBuffer.from_array(vars_)
            rc = fn(self.h, CELLS, ptr(a.units), ptr(a.theta), zptr(a), self.xs_dev.ptr, NS, dm.ptr, dv.ptr, 1)
            check(self.lib.gprx_synchronize(self.h), self.h)
            means, vars_ = dm.to_array(CELLS * NS), dv.to_array(CELLS * NS)
            dm.free()
            dv.free()
        else:
            rc = fn(self.h, CELLS, ptr(a.units), ptr(a.theta), zptr(a), ptr(self.xs), NS, ptr(means), ptr(vars_), 1)
        return rc, self.h, [means, vars_], []

    def predict_current(self):
        mean, var = np.zeros(NS), np.zeros(NS)
        check(self.lib.gprx_predict(self.h, ptr(self.xs), NS, ptr(mean), ptr(var), 1), self.h)
        return bits(mean, var)

    def entries(self):
        e = {
            "objective": lambda a: self.objective(a),
            "factorize": self.factorize,
            "objective_batch_grad": lambda a: self.objective_batch(a, True),
            "objective_batch_loss": lambda a: self.objective_batch(a, False),
            "adam_batch": lambda a: self.optimizer(a, True),
            "adadelta_batch": lambda a: self.optimizer(a, False),
            "predict_batch": lambda a: self.predict_batch(a, "host"),
            "predict_batch_dev": lambda a: self.predict_batch(a, "dev"),
            "predict_batch_t": lambda a: self.predict_batch(a, "t"),
        }
        if self.m == 0:
            e["factorize_many"] = self.factorize_many
            e["factorize_batch"] = self.factorize_batch
        return e


def results(out):
    _, _, outputs, inout = out
    return bits(*outputs, *[now for now, _ in inout])


def check_refused(case, name, call, fault):
    """One refused call between two identical valid ones."""
    what, sparse_only = FAULTS[fault]
    if sparse_only and case.m == 0:
        return
    single = name in ("objective", "factorize")
    before = call(case.good)
    assert before[0] == _lib.GPRX_OK, (name, case.lib.gprx_last_error(before[1]))
    rc, h, outputs, inout = call(faulty(case.good, fault, 0 if single else CELLS - 1))
    msg = case.lib.gprx_last_error(h).decode()
    assert rc == _lib.GPRX_EINVAL, (name, fault, rc, msg)
    assert what in msg and (fault != "z_null" or msg.startswith("z ")), (name, fault, msg)
    for o in outputs:
        untouched = br.is_canary(o) if o.dtype == np.float64 else o == -77
        assert np.all(untouched), f"{name}, {fault}: an output buffer of the refused call was written"
    for now, given in inout:
        assert same_bits(bits(now), bits(given)), f"{name}, {fault}: theta / z of the refused call were changed"
    after = call(case.good)
    assert after[0] == _lib.GPRX_OK, (name, fault, case.lib.gprx_last_error(after[1]))
    assert same_bits(results(before), results(after)), f"{name}, {fault}: the same valid call gives other bits after the refused one"


CASES = [(k, a, m) for k in ("RBF", "Matern32") for a in (0, 1) for m in (0, 5, 70)]


def case_id(p):
    return f"{p[0]}-ard{p[1]}-m{p[2]}"


@pytest.fixture
def case(lib, request):
    c = Case(lib, *request.param)
    yield c
    c.close()


@pytest.mark.parametrize("case", CASES, indirect=True, ids=case_id)
def test_one_bad_cell_is_refused_and_changes_nothing(case):
    for resident in (1, 0):
        check(case.lib.gprx_set_handle_tuning(case.h, b"sgpr_resident", resident), case.h)
        for name, call in case.entries().items():
            if resident == 0 and name not in ("adam_batch", "adadelta_batch"):
                continue  # (the key routes the optimiser loops only)
            for fault in FAULTS:
                check_refused(case, name, call, fault)


@pytest.mark.parametrize("case", CASES, indirect=True, ids=case_id)
def test_optimizers_with_nothing_to_do_do_not_look_at_the_cells(case):
    """max_iter = 0, or a mask with nothing trainable: GPRX_OK and no evaluation, whatever the units are."""
    for resident in (1, 0):
        check(case.lib.gprx_set_handle_tuning(case.h, b"sgpr_resident", resident), case.h)
        for fault in ("unit_negative", "unit_n_units"):
            bad = faulty(case.good, fault, CELLS - 1)
            for adam in (True, False):
                for max_iter, mask in ((0, ALL), (3, 0)):
                    rc, h, _, inout = case.optimizer(bad, adam, max_iter, mask)
                    assert rc == _lib.GPRX_OK, (fault, adam, max_iter, mask, case.lib.gprx_last_error(h))
                    assert np.all(case.n_evals == 0)
                    for now, given in inout:
                        assert same_bits(bits(now), bits(given))


def test_batched_potrf_probe_refuses_what_no_route_takes(lib):
    """gprx_potrf_batched, by return code only: nothing of this reaches a kernel, and info keeps what the caller put there."""
    buf = DeviceBuffer(8 * 65536)
    p, off = buf.ptr, buf.at(1)
    info = np.full(4, -77, dtype=np.int32)
    ip = info.ctypes.data_as(C.POINTER(C.c_int))

    def call(a=p, lda=128, n=128, extra=0, inv=p, stage=p, y=None, batch=1, cs=0, route=0, outer=0, tile=0, lookahead=0, col_base=0, out=ip):
        return lib.gprx_potrf_batched(0, a, lda, n, extra, inv, stage, y, batch, cs, route, outer, tile, lookahead, col_base, out)

    refused = {
        "a null": call(a=None), "inv_diag null": call(inv=None), "stage null": call(stage=None), "info null": call(out=None),
        "np 0": call(n=0), "np negative": call(n=-64), "np % 64": call(n=96), "extra negative": call(extra=-1),
        "odd lda": call(lda=129), "lda < np": call(lda=126), "odd cs": call(batch=2, cs=32769), "negative cs": call(batch=2, cs=-2),
        "cs 0 with cells": call(batch=2, cs=0), "cs shorter than a cell": call(batch=2, cs=128 * 128 - 2),
        "cs shorter than a cell with its right-hand-side rows": call(batch=2, cs=128 * 128, extra=64),
        "a off 16 bytes": call(a=off), "inv_diag off 16 bytes": call(inv=off), "stage off 16 bytes": call(stage=off),
        "yvec off 16 bytes": call(y=off, batch=2, cs=32768, route=1),
        "batch 0": call(batch=0), "route 3": call(route=3), "route -1": call(route=-1), "col_base negative": call(col_base=-1),
        "yvec on the fused panel": call(y=p, batch=2, cs=32768, route=0), "yvec on the cell kernel": call(y=p, batch=2, cs=32768, route=2),
        "yvec with one matrix": call(y=p, batch=1, route=1), "yvec with right-hand-side rows": call(y=p, batch=2, cs=32768, route=1, extra=64),
        "cell kernel with ragged rows": call(route=2, extra=40), "look-ahead with cells": call(batch=2, cs=32768, lookahead=1),
        "look-ahead on the cell kernel": call(route=2, lookahead=1), "lookahead 2": call(lookahead=2),
        "outer_block 96": call(outer=96), "outer_block negative": call(outer=-64), "update_tile 32": call(tile=32),
    }
    assert {k: v for k, v in refused.items() if v != _lib.GPRX_EINVAL} == {}
    assert np.all(info == -77)
    buf.free()


@pytest.mark.parametrize("which", ["host", "dev", "t"])
@pytest.mark.parametrize("case", [c for c in CASES if c[2] != 0], indirect=True, ids=case_id)
def test_batched_sparse_predict_refuses_before_it_factorises(case, which):
    """A non-finite z: the handle still holds the model it held, and predicts it with the same bits."""
    rc, h, _, _ = case.objective(case.good, grad=False)
    assert rc == _lib.GPRX_OK, case.lib.gprx_last_error(h)
    before = case.predict_current()
    rc, h, outputs, _ = case.predict_batch(faulty(case.good, "z_nan", CELLS - 1), which)
    assert rc == _lib.GPRX_EINVAL and "z is not finite" in case.lib.gprx_last_error(h).decode()
    assert all(np.all(br.is_canary(o)) for o in outputs)
    assert same_bits(before, case.predict_current())
