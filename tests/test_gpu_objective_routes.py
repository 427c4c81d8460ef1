"""Every route of the exact-model loss and gradient (csrc/gp_objective.h, gp_exact.h, grad.h, potrf*.h, solve.h) through the C ABI against
the longdouble objective of tests/objective_reference.py: the schedules of a lone fit, both ways of forming alpha, the eight masks, the
distance forms, d beyond the staging chunk and beyond the parameter table, coincident inputs, gprx_objective_batch under every panel and
right-hand-side form, gprx_factorize_many's graph replay.  Every error is measured on the natural scale of its own number (the loss's
terms, each gradient component's own sum of magnitudes) and may be 8 x what a float64 restatement of the route reaches on the same data
(tests/golden/objective_bounds.json); every comparison prints `error / recorded ratio` first."""

import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import objective_reference as orf
from gpras_amd import _lib
from gpras_amd._lib import check, ptr

pytestmark = pytest.mark.gpu

ALL = orf.ALL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)
SUBSTITUTION, FROM_INVERSE = orf.ROUTES


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
class Model:
    """A handle on one case's data with the case's distance form and the given tuning; destroyed on exit."""

    def __init__(self, lib, cid, profiling=False, **tuning):
        c = orf.CASES[cid]
        x, y = orf.data(cid)
        self.lib, self.cid, self.x, self.y = lib, cid, np.ascontiguousarray(x), np.ascontiguousarray(y)
        self.ntheta = (c.d if c.ard else 1) + 2
        self.h = C.c_void_p()
        check(lib.gprx_create(0, c.n, c.d, 0, orf.KERNEL_IDS[c.kernel], int(c.ard), C.byref(self.h)))
        check(lib.gprx_set_distance_form(self.h, _lib.DISTANCE_FORMS[c.form]), self.h)
        check(lib.gprx_set_data(self.h, ptr(self.x), ptr(self.y), self.y.shape[1]), self.h)
        for key, value in tuning.items():
            check(lib.gprx_set_handle_tuning(self.h, key.encode(), value), self.h)
        if profiling:
            check(lib.gprx_set_profiling(self.h, 1), self.h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.gprx_destroy(self.h)

    def objective(self, theta, unit=0, mask=ALL):
        """(loss, grad), both written into canary-filled buffers."""
        theta = np.ascontiguousarray(theta)
        loss, grad = orf.canary(1), orf.canary(self.ntheta)
        check(self.lib.gprx_objective(self.h, unit, ptr(theta), None, mask, loss.ctypes.data_as(DP), ptr(grad)), self.h)
        return loss[0], grad

    def factorize(self, theta, unit=0, mask=ALL):
        theta = np.ascontiguousarray(theta)
        loss = orf.canary(1)
        check(self.lib.gprx_factorize(self.h, unit, ptr(theta), None, mask, ptr(loss)), self.h)
        return loss[0]

    def objective_batch(self, units, thetas, mask=ALL):
        units, thetas = np.ascontiguousarray(units, dtype=np.int32), np.ascontiguousarray(thetas)
        losses, grads = orf.canary(len(units)), orf.canary((len(units), self.ntheta))
        check(self.lib.gprx_objective_batch(self.h, len(units), ptr(units), ptr(thetas), None, mask, ptr(losses), ptr(grads)), self.h)
        return losses, grads

    def factorize_batch(self, units, thetas, mask=ALL):
        units, thetas = np.ascontiguousarray(units, dtype=np.int32), np.ascontiguousarray(thetas)
        losses = orf.canary(len(units))
        check(self.lib.gprx_factorize_batch(self.h, len(units), ptr(units), ptr(thetas), mask, ptr(losses), None), self.h)
        return losses


def hold(loss, grad, cid, cell, route, what, mask=ALL):
    """Loss and every gradient component of one cell against the longdouble reference, each on its natural scale under 8 x the recorded
    ratio of its route; untrained components exactly 0."""
    grad = np.asarray(grad)
    assert not np.any(orf.is_canary(np.array([loss]))) and not np.any(orf.is_canary(grad)), f"{what}: an output nobody wrote"
    assert not np.isnan(loss) and not np.any(np.isnan(grad)), f"{what}: NaN"
    on = orf.trained(mask, grad.size - 2)
    assert np.all(grad[~on] == 0.0), f"{what}: an untrained component is not exactly 0: {grad[~on]}"
    el, eg = orf.errors(loss, grad, orf.reference(cid, cell, mask))
    rl = orf.recorded(cid, cell, route, mask, "loss")
    xg = {int(k): eg[k] / orf.recorded(cid, cell, route, mask, f"g{k}") for k in np.flatnonzero(on)}
    worst = max(xg, key=xg.get) if xg else None
    print(f"{what} [{cid}/c{cell}/{route}/m{mask}]: loss {el:.3e} = {el / rl:.2f} x ratio"
          + (f", gradient worst g{worst} {eg[worst]:.3e} = {xg[worst]:.2f} x ratio" if xg else "")
          + "".join(f" g{k}={v:.2f}" for k, v in xg.items() if len(xg) <= 20))
    assert el <= orf.MARGIN * rl, f"{what}: loss off by {el:.3e} of its scale, allowed {orf.MARGIN * rl:.3e}"
    for k, v in xg.items():
        assert v <= orf.MARGIN, f"{what}: gradient component {k} off by {eg[k]:.3e} of its scale, allowed {orf.MARGIN * eg[k] / v:.3e}"


def hold_batch(losses, grads, cid, route, what, mask=ALL):
    assert not np.any(orf.is_canary(losses)) and not np.any(orf.is_canary(grads)), f"{what}: an output nobody wrote"
    for cell in range(len(orf.CASES[cid].units)):
        hold(losses[cell], grads[cell], cid, cell, route, f"{what}, cell {cell}", mask)


def bits(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist() for a in arrays]


def same_bits(a, b):
    return bits(*a) == bits(*b)


# ---- a single model ----------------------------------------------------------------------------------------------------------------
# name -> (profiling, tuning, how alpha is formed)
SINGLE_ROUTES = {
    "default": (False, {}, FROM_INVERSE),                  # the fused evaluation: alpha = X^T beta
    "profiling": (True, {}, SUBSTITUTION),                 # the unfused path: backward substitution, then exact_gradient
    "dag": (False, {"dag": 1}, FROM_INVERSE),
    "no_lookahead": (False, {"no_lookahead": 1}, FROM_INVERSE),
    "update_tile_128": (False, {"update_tile": 128}, FROM_INVERSE),
    "poison_workspace": (False, {"poison_workspace": 1}, FROM_INVERSE),
    "outer_block_128": (False, {"outer_block": 128}, FROM_INVERSE),  # HEAD / TAIL outer blocks wherever np > 128
    "outer_block_128_update_tile_128": (False, {"outer_block": 128, "update_tile": 128}, FROM_INVERSE),
}
SAME_LOSS_BITS = ("default", "profiling", "no_lookahead", "update_tile_128", "poison_workspace")  # (one outer block: the same sums)


@pytest.mark.parametrize("cid", [c.id for c in orf.SINGLE])
def test_single_model_every_route_against_longdouble(lib, cid):
    """Each schedule of a lone fit forced on a fresh handle and held to the bound of its way of forming alpha.  The loss is the same bits
    on every schedule but the tile DAG and the 128-column outer blocks (other groupings of the updates of a tile: to their bounds), and
    gprx_factorize -- no gradient -- gives the bits of gprx_objective."""
    theta = orf.thetas(cid)[0]
    losses = {}
    for name, (profiling, tuning, route) in SINGLE_ROUTES.items():
        with Model(lib, cid, profiling, **tuning) as m:
            loss, grad = m.objective(theta)
            hold(loss, grad, cid, 0, route, name)
            losses[name] = loss
            assert same_bits([m.factorize(theta)], [loss]), name
    for name in SAME_LOSS_BITS:
        assert same_bits([losses[name]], [losses["default"]]), name


def test_the_eight_masks(lib):
    """A9 (ARD, d = 9) under every mask, against objective_ld(mask): the prior terms enter the loss and the gradient for trained parameters
    only, untrained components are exactly 0.0 (hold() asserts it); both ways of forming alpha."""
    theta = orf.thetas("A9")[0]
    for profiling, route in ((False, FROM_INVERSE), (True, SUBSTITUTION)):
        with Model(lib, "A9", profiling) as m:
            for mask in orf.CASES["A9"].masks:
                hold(*m.objective(theta, 0, mask), "A9", 0, route, f"mask {mask}", mask)


UNFUSED_CASES = ("K-Matern12", "A9", "N385")
UNFUSED = r"""
import json, sys
sys.path[:0] = [{root!r}, {tests!r}]
import objective_reference as orf
import test_gpu_objective_routes as t
from gpras_amd import _lib
lib = _lib.load()
out = {{}}
for cid in {cases!r}:
    with t.Model(lib, cid) as m:
        loss, grad = m.objective(orf.thetas(cid)[0])
    out[cid] = [float.hex(float(loss)), [float.hex(float(v)) for v in grad]]
print(json.dumps(out))
"""


def test_unfused_evaluation_by_environment_switch(lib):
    """GPRX_FUSED_EVAL=0 (a process-wide static, hence ONE child for three cases): the evaluation waits for the factorisation, alpha comes
    from the backward substitution -- the substitution bounds -- and the loss is the parent's fused one bit for bit."""
    env = dict(os.environ, GPRX_FUSED_EVAL="0")
    code = UNFUSED.format(root=ROOT, tests=os.path.join(ROOT, "tests"), cases=UNFUSED_CASES)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    for cid in UNFUSED_CASES:
        loss, grad = float.fromhex(out[cid][0]), np.array([float.fromhex(v) for v in out[cid][1]])
        hold(loss, grad, cid, 0, SUBSTITUTION, "GPRX_FUSED_EVAL=0")
        with Model(lib, cid) as m:
            fused_loss, fused_grad = m.objective(orf.thetas(cid)[0])
        assert same_bits([loss], [fused_loss])
        assert not same_bits([grad], [fused_grad])  # (alpha formed another way: the child did take the other path)


def test_second_theta_on_the_same_handle_and_back(lib):
    """D70 (d = 70: the lengthscales leave the pinned staging area of upload_inv_ls), then D70b's hyperparameters on the same handle to their
    own bound, then the first ones again: the first bits."""
    a, b = orf.thetas("D70")[0], orf.thetas("D70b")[0]
    with Model(lib, "D70") as m:
        first = m.objective(a)
        hold(*first, "D70", 0, FROM_INVERSE, "first theta")
        hold(*m.objective(b), "D70b", 0, FROM_INVERSE, "second theta")
        assert same_bits(m.objective(a), first)


# ---- gprx_objective_batch ----------------------------------------------------------------------------------------------------------
# name -> tuning; every one forms alpha from the inverse
BATCH_ROUTES = {
    "default": {},
    "split_vector": {"split_panel": 1, "rhs_vector": 0},   # potrf_rows_kernel<..., YVEC>
    "split_tile": {"split_panel": 1, "rhs_vector": -1},
    "fused_panel": {"split_panel": -1},
    "cell_kernel": {"cell_kernel": 1},
    "update_tile_128": {"update_tile": 128},                # the 128-wide tile of the batched trtri_lower
}


@pytest.mark.parametrize("cid", ["B3", "B26", "B5"])
def test_batch_every_route_per_cell_against_longdouble(lib, cid):
    """B3 (mixed units and thetas), B26 (26 cells of np = 128: the split panel and the vector right-hand side by default), B5 (ARD, d = 9):
    every cell of gprx_objective_batch to its own reference under each setting, and the repository's stated equalities: the fused panel
    and the split panel with the right-hand side as a tile agree bit for bit, and are the bits of gprx_objective on each cell; the vector
    right-hand side and the one-workgroup-per-cell kernel are held to their bounds; gprx_factorize_batch gives the batch's losses."""
    c = orf.CASES[cid]
    th = orf.thetas(cid)
    got = {}
    for name, tuning in BATCH_ROUTES.items():
        with Model(lib, cid, **tuning) as m:
            got[name] = m.objective_batch(c.units, th)
            hold_batch(*got[name], cid, FROM_INVERSE, name)
            assert same_bits([m.factorize_batch(c.units, th)], [got[name][0]]), name
    assert same_bits(got["fused_panel"], got["split_tile"])
    with Model(lib, cid) as m:
        singles = [m.objective(th[cell], c.units[cell]) for cell in range(len(c.units))]
    assert same_bits(got["fused_panel"], (np.array([s[0] for s in singles]), np.stack([s[1] for s in singles])))
    default_is = "split_vector" if len(c.units) >= 24 else "fused_panel"
    assert same_bits(got["default"], got[default_is])


def test_batch_wider_than_the_parameter_table_is_its_single_calls(lib):
    """B4, d = 66: the lengthscales do not fit a row of the cell-parameter table, gprx_objective_batch evaluates one cell after the other --
    each to its reference, and the bits of gprx_objective."""
    c = orf.CASES["B4"]
    th = orf.thetas("B4")
    with Model(lib, "B4") as m:
        losses, grads = m.objective_batch(c.units, th)
        hold_batch(losses, grads, "B4", FROM_INVERSE, "per-cell loop")
        singles = [m.objective(th[cell], c.units[cell]) for cell in range(len(c.units))]
    assert same_bits((losses, grads), (np.array([s[0] for s in singles]), np.stack([s[1] for s in singles])))


def test_factorize_many_eager_then_replayed(lib):
    """Two handles (K-Matern52: np = 128 with 65 rows; H-2: n = np = 192), three calls: the first runs eagerly, the second captures the
    graph and replays it, the third replays.  The losses meet the reference and are the same bits every time.  (The one test here that
    replays a captured graph.)"""
    cids = ("K-Matern52", "H-2")
    thetas = np.ascontiguousarray(np.stack([orf.thetas(cid)[0] for cid in cids]))
    units = np.zeros(2, dtype=np.int32)
    with Model(lib, cids[0]) as m0, Model(lib, cids[1]) as m1:
        handles = (C.c_void_p * 2)(m0.h, m1.h)
        seen = []
        for rep in range(3):
            losses = orf.canary(2)
            check(lib.gprx_factorize_many(2, handles, ptr(units), ptr(thetas), ALL, ptr(losses)))
            assert not np.any(orf.is_canary(losses))
            for i, cid in enumerate(cids):
                ref_loss, _, loss_scale, _ = orf.reference(cid, 0)
                el = float(abs(orf.LD(losses[i]) - ref_loss) / loss_scale)
                rl = orf.recorded(cid, 0, SUBSTITUTION, ALL, "loss")
                print(f"call {rep} [{cid}/c0/{SUBSTITUTION}/m{ALL}]: loss {el:.3e} = {el / rl:.2f} x ratio")
                assert el <= orf.MARGIN * rl, (rep, cid, el)
            seen.append(losses)
        assert same_bits(seen[1:], [seen[0], seen[0]])
        for m, theta, loss in zip((m0, m1), thetas, seen[0]):
            assert same_bits([m.factorize(theta)], [loss])
