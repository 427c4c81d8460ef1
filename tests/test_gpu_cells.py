"""The one-workgroup-per-cell Cholesky for many small matrices (gpras_amd/csrc/potrf_cell.h; "cell_kernel" = 1 forces it, -1
forbids it, default: N <= 256 from 32 cells, N <= 512 from 160, N <= 1024 from 256) through gprx_factorize_batch /
gprx_objective_batch: against the batched launch sequence (same tile products, another summation grouping: equal to rounding),
against the oracle, with a failing cell, and the forms of the kernel that remain against each other: the right-hand side as tile rows
(GPRX_CELL_BETA_ROWS=1; also with K evaluated inside the kernel, GPRX_CELL_BUILD_K=1) bit for bit, the default vector form to rounding."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from gpras_amd import _lib
from gpras_amd._lib import check, ptr
from gpras_amd.synth import make_regression
from oracle import exact as oex
from oracle import kernels as okn
from oracle import transforms as otr

pytestmark = pytest.mark.gpu
ALL = _lib.TRAIN_VARIANCE | _lib.TRAIN_LENGTHSCALE | _lib.TRAIN_NOISE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def handle(lib, n, d, kernel, x, y, cell_kernel):
    h = C.c_void_p()
    check(lib.gprx_create(0, n, d, 0, okn.KERNEL_IDS[kernel], 0, C.byref(h)))
    check(lib.gprx_set_handle_tuning(h, b"cell_kernel", cell_kernel), h)
    check(lib.gprx_set_data(h, ptr(x), ptr(y), y.shape[1]), h)
    return h


def thetas_for(x, cells, seed):
    base = np.array(otr.unconstrain(1.0, float(np.mean(np.abs(x))), 0.5), dtype=np.float64)
    return np.ascontiguousarray(base[None, :] + np.random.default_rng(seed).uniform(-0.2, 0.2, size=(cells, 3)))


@pytest.mark.parametrize("kernel,n,d,cells", [("RBF", 64, 2, 5), ("RBF", 200, 3, 40), ("Matern52", 333, 4, 12), ("Matern12", 512, 8, 9), ("RBF", 1000, 5, 6),
                                              ("Matern32", 1024, 8, 4), ("RBF", 1088, 3, 3)])  # (1088: 17 block columns, the forced kernel's tile-row form)
def test_cell_kernel_against_launch_sequence_and_oracle(lib, kernel, n, d, cells):
    ns = 40
    x, y, xs = make_regression(n, d, n_outputs=cells, n_test=ns, config=2, unit=n)
    thetas = thetas_for(x, cells, n)
    units = np.arange(cells, dtype=np.int32)
    got = {}
    for mode in (-1, 1):
        h = handle(lib, n, d, kernel, x, y, mode)
        try:
            losses, status = np.zeros(cells), np.zeros(cells, dtype=np.int32)
            check(lib.gprx_factorize_batch(h, cells, ptr(units), ptr(thetas), ALL, ptr(losses), ptr(status)), h)
            assert not status.any()
            preds = []
            for c in (0, cells - 1):
                check(lib.gprx_select_slot(h, c), h)
                mean, var = np.zeros(ns), np.zeros(ns)
                check(lib.gprx_predict(h, ptr(xs), ns, ptr(mean), ptr(var), 1), h)
                preds.append((mean, var))
            glosses, grads = np.zeros(cells), np.zeros((cells, 3))
            check(lib.gprx_objective_batch(h, cells, ptr(units), ptr(thetas), None, ALL, ptr(glosses), ptr(grads)), h)
            got[mode] = (losses, preds, glosses, grads)
        finally:
            lib.gprx_destroy(h)
    (l0, p0, gl0, g0), (l1, p1, gl1, g1) = got[-1], got[1]
    assert np.max(np.abs(l1 - l0) / np.abs(l0)) <= 1e-13
    assert np.array_equal(gl1, l1) or np.max(np.abs(gl1 - l1) / np.abs(l1)) <= 1e-15  # (objective = factorisation + prior of nothing)
    assert np.max(np.abs(g1 - g0)) <= 1e-9 * np.max(np.abs(g0))
    for (m0, v0), (m1, v1) in zip(p0, p1):
        assert np.max(np.abs(m1 - m0)) <= 1e-11 * np.max(np.abs(m0)) and np.max(np.abs(v1 - v0) / v0) <= 1e-11
    for c, (mean, var) in zip((0, cells - 1), p1):
        ref = oex.loss(kernel, x, y[:, c], float(thetas[c, 0]), float(thetas[c, 1]), float(thetas[c, 2]))
        assert abs(l1[c] - ref) <= 1e-9 * abs(ref)
        v, l, s = otr.constrain(thetas[c, 0], thetas[c, 1], thetas[c, 2])
        rm, rv = oex.predict(kernel, x, y[:, c], float(v), float(l), float(s), xs)
        assert np.max(np.abs(mean - rm)) <= 1e-8 * np.max(np.abs(rm)) and np.max(np.abs(var - rv) / rv) <= 1e-8


NON_PD_VARIANCE = 2.0**40  # with noise 1e-6 the diagonal v + s rounds to v, and sqrt / rsqrt of a power of four are exact: on rows that
                            # duplicate their predecessor the second pivot is v - (v / sqrt(v))^2 = 0 EXACTLY, on the host and on the device


@pytest.mark.parametrize("cell_kernel", [1, -1])
def test_a_non_positive_definite_cell_is_reported_alone(lib, cell_kernel):
    """a cell that IS not positive definite in fp64 -- scipy's Cholesky of the oracle's K raises, checked first -- must
    come back as GPRX_ENOTPD with its own status entry and a NaN loss, from the one-workgroup-per-cell kernel (1) and from the
    launch sequence (-1), while its neighbours finish with the values they have alone."""
    n, d = 256, 3
    x, y, _ = make_regression(n, d, config=1, unit=1)
    x[1::2] = x[0::2]  # duplicated inputs: singular without the noise term
    good = np.array([float(v) for v in otr.unconstrain(1.0, 0.9, 0.1)])
    bad = np.array([NON_PD_VARIANCE, float(otr.unconstrain(1.0, 0.9, 0.1)[1]), -800.0])
    with pytest.raises(np.linalg.LinAlgError, match="2-th leading minor"):
        oex.loss("RBF", x, y[:, 0], bad[0], bad[1], bad[2])
    h = handle(lib, n, d, "RBF", x, y, 1)
    try:
        check(lib.gprx_set_handle_tuning(h, b"cell_kernel", cell_kernel), h)
        thetas = np.ascontiguousarray(np.stack([good, bad, good, good]))
        units = np.zeros(4, dtype=np.int32)
        losses, status = np.zeros(4), np.zeros(4, dtype=np.int32)
        rc = lib.gprx_factorize_batch(h, 4, ptr(units), ptr(thetas), ALL, ptr(losses), ptr(status))
        assert rc == _lib.GPRX_ENOTPD
        assert status[1] == _lib.GPRX_ENOTPD and not status[[0, 2, 3]].any() and np.isnan(losses[1])
        ref = oex.loss("RBF", x, y[:, 0], float(good[0]), float(good[1]), float(good[2]))
        assert abs(losses[0] - ref) <= 1e-9 * abs(ref) and losses[2] == losses[0] and losses[3] == losses[0]
        assert lib.gprx_select_slot(h, 1) == _lib.GPRX_ESTATE  # nothing to predict from
        assert lib.gprx_select_slot(h, 2) == _lib.GPRX_OK
        single = C.c_double()  # the lone call names the same pivot as LAPACK (1-based)
        assert lib.gprx_factorize(h, 0, ptr(bad), None, ALL, C.byref(single)) == _lib.GPRX_ENOTPD
        assert lib.gprx_last_error(h).endswith(b"pivot 2")
    finally:
        lib.gprx_destroy(h)


FORMS = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, {root!r})
from gpras_amd import _lib
from gpras_amd._lib import check, ptr
from gpras_amd.synth import make_regression
from oracle import transforms as otr
lib = _lib.load()
out = []
for n, d, cells in ((700, 4, 10), (1024, 8, 6), (64, 2, 3), (130, 3, 7), (960, 5, 4)):  # 11, 16, 1, 3 and 15 block columns
    x, y, _ = make_regression(n, d, n_outputs=cells, n_test=4, config=2, unit=n)
    base = np.array(otr.unconstrain(1.0, float(np.mean(np.abs(x))), 0.5), dtype=np.float64)
    thetas = np.ascontiguousarray(base[None, :] + np.random.default_rng(1).uniform(-0.2, 0.2, size=(cells, 3)))
    units = np.arange(cells, dtype=np.int32)
    h = C.c_void_p()
    check(lib.gprx_create(0, n, d, 0, 0, 0, C.byref(h)))
    check(lib.gprx_set_handle_tuning(h, b"cell_kernel", 1), h)
    check(lib.gprx_set_data(h, ptr(x), ptr(y), cells), h)
    losses, status = np.zeros(cells), np.zeros(cells, dtype=np.int32)
    check(lib.gprx_factorize_batch(h, cells, ptr(units), ptr(thetas), 7, ptr(losses), ptr(status)), h)
    lib.gprx_destroy(h)
    out += [float.hex(v) for v in losses]
print(json.dumps(out))
"""


def test_cell_kernel_forms_agree_bit_for_bit():
    """The forms of the column-pair kernel (two block columns per pass on LDS-DMA operand panels, potrf_cell.h cell2_rows) that carry the
    right-hand side as tile rows -- K read from memory, and K evaluated inside the kernel (GPRX_CELL_BUILD_K=1) -- perform the same tile
    products on the same operands in the same accumulation order: the losses are equal to the last bit.  (Round 3's two-pass and
    single-column kernels were part of this comparison until they were retired; they agreed to the last bit.)"""
    import json

    outs = []
    # (GPRX_CELL_BUILD_K applies to even block-column counts only; the odd cases of that run take the plain kernel, pinned to the tile form too)
    for env in ({"GPRX_CELL_BETA_ROWS": "1"}, {"GPRX_CELL_BUILD_K": "1", "GPRX_CELL_BETA_ROWS": "1"}, {}):
        base = {k: v for k, v in os.environ.items() if not k.startswith("GPRX_CELL")}
        res = subprocess.run([sys.executable, "-c", FORMS.format(root=ROOT)], capture_output=True, text=True, timeout=600, env=dict(base, **env))
        assert res.returncode == 0, res.stderr[-2000:]
        outs.append(res.stdout.strip().splitlines()[-1])
    assert outs[0] == outs[1]
    # the default form carries the right-hand side as a VECTOR (cell2_beta_*: beta = L^-1 y by matrix-vector products on the same factor,
    # no tile row): the factor and log det are those bits, y^T K^-1 y = |beta|^2 is summed in another order -- equal to rounding
    tiles = np.array([float.fromhex(v) for v in json.loads(outs[0])])
    vector = np.array([float.fromhex(v) for v in json.loads(outs[2])])
    assert np.max(np.abs(vector - tiles) / np.abs(tiles)) <= 1e-14


FULL_LOAD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, {root!r})
from gpras_amd import _lib
from gpras_amd._lib import check, ptr
from gpras_amd.synth import make_regression
from oracle import transforms as otr
lib = _lib.load()
n, d, cells = 1024, 8, 512
x, y, _ = make_regression(n, d, n_outputs=cells, n_test=4, config=2, unit=n)
base = np.array(otr.unconstrain(1.0, float(np.mean(np.abs(x))), 0.5), dtype=np.float64)
thetas = np.ascontiguousarray(base[None, :] + np.random.default_rng(1).uniform(-0.2, 0.2, size=(cells, 3)))
units = np.arange(cells, dtype=np.int32)
h = C.c_void_p()
check(lib.gprx_create(0, n, d, 0, 0, 0, C.byref(h)))
check(lib.gprx_set_handle_tuning(h, b"cell_kernel", int(sys.argv[1])), h)
check(lib.gprx_set_data(h, ptr(x), ptr(y), cells), h)
out = []
for rep in range(3):
    losses, status = np.zeros(cells), np.zeros(cells, dtype=np.int32)
    check(lib.gprx_factorize_batch(h, cells, ptr(units), ptr(thetas), 7, ptr(losses), ptr(status)), h)
    out.append([float.hex(v) for v in losses])
lib.gprx_destroy(h)
print(json.dumps(out))
"""


def test_cell_kernels_at_full_load_two_workgroups_per_cu():
    """Round 4: every remaining form of the one-workgroup-per-cell kernel (tile rows, tile rows with K built inside, vector) at FULL load -- 512 cells of N = 1024, two workgroups on every CU --, three
    repetitions each: the same bits every time, the same bits in every form, and the launch sequence's values to rounding.  (A store
    whose data registers were reused too early corrupted the low dword of a few entries of L(j,j)^-1 in 7-50 % of the cells of the
    workgroups that became resident second, differently on every run, and only in some builds; the small cases above never showed it.)"""
    import json

    def run(knob, env):
        base = {k: v for k, v in os.environ.items() if not k.startswith("GPRX_CELL")}
        res = subprocess.run([sys.executable, "-c", FULL_LOAD.format(root=ROOT), str(knob)], capture_output=True, text=True, timeout=600, env=dict(base, **env))
        assert res.returncode == 0, res.stderr[-2000:]
        return json.loads(res.stdout.strip().splitlines()[-1])

    seq = run(-1, {})
    assert seq[0] == seq[1] == seq[2]
    ref = np.array([float.fromhex(v) for v in seq[0]])
    first = None
    for env in ({"GPRX_CELL_BETA_ROWS": "1"}, {"GPRX_CELL_BUILD_K": "1", "GPRX_CELL_BETA_ROWS": "1"}, {}):
        got = run(1, env)
        assert got[0] == got[1] == got[2], env
        first = first or got[0]
        if env:  # (the default form's right-hand side is a vector: same factor, another summation order -- equal to rounding, checked below)
            assert got[0] == first, env
        vals = np.array([float.fromhex(v) for v in got[0]])
        assert np.max(np.abs(vals - ref) / np.abs(ref)) <= 1e-13, env
