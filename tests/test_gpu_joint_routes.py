"""Every route of the joint sparse prediction (csrc/gp_joint.h, gprx_predict_joint_batch_dev) through the C ABI against the longdouble
definition of tests/joint_reference.py: who produced L, LB and c (the five fused launches, the launch sequence at M <= 64 and above, two
row chunks at mp = 320), every kernel build (kernel x class, d = 17 and 64), every event length at which a launch changes shape up to the
1024-row limit, every Cholesky route (fused and split panel, one rows launch per panel and per pair, one workgroup per cell, the picker's
own choice at 24 cells), a reused workspace, the two ENOTPD paths and the chunking of PeakEnsemble.joint_dev.  A result may be off by
8 x what a float64 restatement of the call reaches on the same data (tests/golden/joint_bounds.json) in three measures -- the mean,
Lc Lc^T entry by entry on the entry's natural scale, Lc entry by entry on the norm of its row --; every comparison prints
`error / recorded ratio` first, and every test closes with the largest share of the 8 x it used."""

import ctypes as C

import numpy as np
import pytest

import joint_reference as jr
from gpras_amd import _lib
from gpras_amd._lib import DeviceBuffer, check, ptr

pytestmark = pytest.mark.gpu

GUARD = 256  # canaries behind each output
USED = {}    # group -> the largest error / recorded ratio seen
LAUNCHES, SPLIT_PER_PANEL, SPLIT_PAIR, CELL = "fused panel", "split panel, rows per panel", "split panel, rows pair", "cell kernel"
ROUTE_TUNING = {
    LAUNCHES: dict(cell_kernel=-1, split_panel=-1, rows_pair=1),
    SPLIT_PER_PANEL: dict(cell_kernel=-1, split_panel=1, rows_pair=0),
    SPLIT_PAIR: dict(cell_kernel=-1, split_panel=1, rows_pair=1),
    CELL: dict(cell_kernel=1, split_panel=-1, rows_pair=1),
}


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
class Joint:
    """A handle on one case's data with the case's distance form and the given tuning; destroyed on exit."""

    def __init__(self, lib, cid, **tuning):
        c = jr.CASES[cid]
        x, y, zs, xs = jr.data(cid)
        self.lib, self.cid, self.case = lib, cid, c
        self.x, self.y, self.zs, self.xs = (np.ascontiguousarray(a) for a in (x, y, zs, xs))
        self.thetas, self.units = np.ascontiguousarray(jr.thetas(cid)), jr.units(cid)
        self.h = C.c_void_p()
        check(lib.gprx_create(0, jr.N_TRAIN, c.d, c.m, jr.KERNEL_IDS[c.kernel], int(c.ard), C.byref(self.h)))
        check(lib.gprx_set_data(self.h, ptr(self.x), ptr(self.y), self.y.shape[1]), self.h)
        check(lib.gprx_set_distance_form(self.h, _lib.DISTANCE_FORMS[c.form]), self.h)
        self.tune(**tuning)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.gprx_destroy(self.h)

    def tune(self, **tuning):
        for key, value in tuning.items():
            check(self.lib.gprx_set_handle_tuning(self.h, key.encode(), value), self.h)

    def call(self, cells=None, include_noise=1, xs=None, thetas=None, expect=_lib.GPRX_OK):
        """gprx_predict_joint_batch_dev on the given cells (default all) into canary-filled buffers, then gprx_predict_batch_dev on the
        same arguments.  Asserts what holds for every call -- the canaries behind both outputs untouched and none left inside, the mean
        the batched predict's bit for bit, Lc lower triangular with the exact identity on the padding -- and returns
        (mean (count, ns), Lc (count, Tp, Tp)); with an expected error status: the status's message."""
        cells = list(range(self.case.cells)) if cells is None else list(cells)
        xs = self.xs if xs is None else np.ascontiguousarray(xs)
        units, zs = np.ascontiguousarray(self.units[cells]), np.ascontiguousarray(self.zs[cells])
        thetas = np.ascontiguousarray((self.thetas if thetas is None else thetas)[cells])
        count, ns = len(cells), xs.shape[0]
        tp = -(-ns // jr.NB) * jr.NB
        bufs = [DeviceBuffer.from_array(xs), DeviceBuffer.from_array(jr.canary(count * ns + GUARD)),
                DeviceBuffer.from_array(jr.canary(count * tp * tp + GUARD)), DeviceBuffer.from_array(jr.canary(count * ns + GUARD)),
                DeviceBuffer.from_array(jr.canary(count * ns + GUARD))]
        dxs, dmean, dlc, dmean2, dvar = bufs
        try:
            rc = self.lib.gprx_predict_joint_batch_dev(self.h, count, ptr(units), ptr(thetas), ptr(zs), dxs.ptr, ns, dmean.ptr, dlc.ptr, include_noise)
            assert rc == expect, (rc, _lib.last_error(self.h))
            if expect != _lib.GPRX_OK:
                return _lib.last_error(self.h)
            check(self.lib.gprx_predict_batch_dev(self.h, count, ptr(units), ptr(thetas), ptr(zs), dxs.ptr, ns, dmean2.ptr, dvar.ptr, include_noise), self.h)
            check(self.lib.gprx_synchronize(self.h), self.h)
            mean, lc, mean2 = dmean.to_array(count * ns + GUARD), dlc.to_array(count * tp * tp + GUARD), dmean2.to_array(count * ns + GUARD)
        finally:
            for b in bufs:
                b.free()
        what = f"{self.cid}, {count} cells, ns = {ns}, include_noise = {include_noise}"
        assert np.all(jr.is_canary(mean[count * ns:])) and np.all(jr.is_canary(lc[count * tp * tp:])), f"{what}: written past the end of an output"
        mean, lc, mean2 = mean[:count * ns].reshape(count, ns), lc[:count * tp * tp].reshape(count, tp, tp), mean2[:count * ns].reshape(count, ns)
        assert not np.any(jr.is_canary(mean)) and not np.any(jr.is_canary(lc)), f"{what}: an output element nobody wrote"
        assert same_bits(mean, mean2), f"{what}: the mean is not gprx_predict_batch_dev's"
        for c in range(count):
            assert np.array_equal(lc[c], np.tril(lc[c])), f"{what}, cell {c}: not lower triangular"
            assert np.array_equal(lc[c, ns:, ns:], np.eye(tp - ns)) and not np.any(lc[c, ns:, :ns]), f"{what}, cell {c}: the padding is not the identity"
        return mean, lc


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def hold(group, mean, lc, cid, cell, include_noise, what):
    """Mean and factor of one cell (lc: its (Tp, Tp) block) against the longdouble reference: the three measures within 8 x recorded."""
    ns = jr.CASES[cid].ns
    assert not np.any(np.isnan(mean)) and not np.any(np.isnan(lc)), f"{what}: NaN"
    got = jr.errors(mean, lc[:ns, :ns], cid, cell, include_noise)
    used = {q: val / jr.recorded(cid, cell, include_noise, q) for q, val in got.items()}
    print(f"{what} [{jr.key(cid, cell, include_noise, '')}]: " + ", ".join(f"{q} {got[q]:.3e} = {used[q]:.2f} x ratio" for q in jr.QUANTITIES))
    USED[group] = max(USED.get(group, 0.0), max(used.values()))
    for q, val in used.items():
        assert val <= jr.MARGIN, f"{what}: {q} off by {got[q]:.3e}, allowed {jr.MARGIN * jr.recorded(cid, cell, include_noise, q):.3e}"


def hold_call(group, mean, lc, cid, include_noise, what, cells=None):
    for i, cell in enumerate(range(jr.CASES[cid].cells) if cells is None else cells):
        hold(group, mean[i], lc[i], cid, cell, include_noise, f"{what}, cell {cell}")


def report(group):
    print(f"group {group}: used {USED.get(group, 0.0):.2f} of {jr.MARGIN:.0f} x recorded")


def whole_and_alone(lib, group, cid, **tuning):
    """All cells in one call against the reference, both include_noise values; every cell called alone gives the batch's bits (one
    cell and three take the same Cholesky route: the launch sequence with the fused panel).  Returns the include_noise = 1 result."""
    with Joint(lib, cid, **tuning) as m:
        for include_noise in (1, 0):
            mean, lc = m.call(include_noise=include_noise)
            hold_call(group, mean, lc, cid, include_noise, f"{m.case.cells} cells")
            for cell in range(m.case.cells):
                m1, l1 = m.call([cell], include_noise)
                assert same_bits(m1[0], mean[cell]) and same_bits(l1[0], lc[cell]), (cid, cell, include_noise)
            if include_noise:
                first = (mean, lc)
    return first


# ---- who produced L, LB and c ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", jr.GROUPS["factors"])
def test_factors_from_every_producer(lib, cid):
    """M = 1, 50, 64 (the five fused launches), 65 (mp = 128, nearly all padding), 192, 300 and 320 (mp = 320: two row chunks of the
    mean's column reduce), 65 and 130 event rows."""
    whole_and_alone(lib, "factors", cid)
    report("factors")


@pytest.mark.parametrize("cid", jr.UNFUSED)
def test_factors_from_the_launch_sequence_at_64_or_fewer_inducing_points(lib, cid):
    """"sgpr_fused" = 0 at M = 50: the launch sequence of gp_sparse.h leaves L, LB and c where the joint call reads them -- within the
    bounds, and not the bits of the fused producer (the other producer ran)."""
    fused = whole_and_alone(lib, "factors", cid)
    unfused = whole_and_alone(lib, "factors", cid, sgpr_fused=0)
    assert not same_bits(fused[0], unfused[0]) or not same_bits(fused[1], unfused[1])
    report("factors")


# ---- kernel builds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", jr.GROUPS["build"])
def test_every_kernel_build(lib, cid):
    """Five kernels x (iso, ARD, expanded) at d = 3, then d = 17 ARD (three staging passes of the build), d = 64 ARD and d = 64
    isotropic in the expanded form: the rectangle Kus and the symmetric mode of launch_kmat for Kss."""
    whole_and_alone(lib, "build", cid)
    report("build")


# ---- event lengths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", jr.GROUPS["rows"])
def test_every_event_length(lib, cid):
    """1, 64, 65, 256, 257 (both sides of a block of colreduce and of joint_diag_kernel), 300 and the limit, 1024 rows (Tp = 1024: tmp1
    beside tmp2 in the cell's tile)."""
    whole_and_alone(lib, "rows", cid)
    report("rows")


# ---- Cholesky routes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", jr.ROUTE_CASES)
def test_every_cholesky_route(lib, cid):
    """Tp = 320 (3 cells) and Tp = 1024 (2 cells) through the fused panel, the split panel with one rows launch per panel and per pair of
    panels, and one workgroup per cell.  The three launch sequences give the same bits (csrc/potrf.h); the cell kernel is another
    summation order, within the bounds."""
    got = {}
    with Joint(lib, cid) as m:
        for route, tuning in ROUTE_TUNING.items():
            m.tune(**tuning)
            got[route] = m.call(include_noise=1)
    for route in (SPLIT_PER_PANEL, SPLIT_PAIR):
        assert same_bits(got[route][0], got[LAUNCHES][0]) and same_bits(got[route][1], got[LAUNCHES][1]), route
    assert same_bits(got[CELL][0], got[LAUNCHES][0]) and not same_bits(got[CELL][1], got[LAUNCHES][1])
    for route in (LAUNCHES, CELL):
        hold_call("routes", *got[route], cid, 1, route)
    report("routes")


def test_24_cells_take_the_split_panel_by_the_pickers_choice(lib):
    """Untouched tuning at Tp = 320 with 24 cells, 8 hyperparameter sets x 3 units: the first count at which potrf_lower takes the split
    panel (and the rows-pair kernel), on the workspace layout of the joint call.  Every cell against the reference of its (set, unit);
    the first and the last cell called alone (the fused panel) give the batch's bits."""
    with Joint(lib, "C24") as m:
        mean, lc = m.call(include_noise=1)
        hold_call("routes", mean, lc, "C24", 1, "24 cells")
        for cell in (0, 23):
            m1, l1 = m.call([cell], 1)
            assert same_bits(m1[0], mean[cell]) and same_bits(l1[0], lc[cell]), cell
    report("routes")


# ---- a reused workspace ----------------------------------------------------------------------------------------------------------------
def test_a_short_event_after_a_long_one_on_the_same_handle(lib):
    """h->joint_ws is reused: 1024 rows, then 65, then 300, then one cell, then three -- each the bits of the same call on a fresh handle
    (the symmetric launch_kmat rewrites the identity padding; nothing of the longer event is read)."""
    cid = "R-RBF-ns300"
    c = jr.CASES[cid]
    rows = jr._points(c.d, c.seed)[2]
    calls = [((0, 1), rows[:1024]), ((0, 1, 2), rows[:65]), ((0, 1, 2), rows[:300]), ((1,), rows[:300]), ((0, 1, 2), rows[:300])]
    with Joint(lib, cid) as reused:
        for cells, xs in calls:
            for include_noise in (1, 0):
                got = reused.call(cells, include_noise, xs=xs)
                with Joint(lib, cid) as fresh:
                    want = fresh.call(cells, include_noise, xs=xs)
                assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (cells, xs.shape[0], include_noise)


# ---- the error paths -----------------------------------------------------------------------------------------------------------------
def test_a_nan_test_point_is_enotpd_at_its_pivot_and_the_handle_lives_on(lib):
    """Row 70 of a 130-row event has a NaN coordinate: row and column 70 of the covariance are NaN, the rows before it never read them,
    and the pivot test !(s > 0) fails first at pivot 71 (counted from 1) of the first cell.  A status code read back from the info words
    of the workspace, not a device fault; the same call with clean rows then gives the bits it gave before."""
    cid, row = "F-m50-ns130", 70
    with Joint(lib, cid) as m:
        before = m.call(include_noise=1)
        xs = m.xs.copy()
        xs[row, 0] = np.nan
        msg = m.call(include_noise=1, xs=xs, expect=_lib.GPRX_ENOTPD)
        assert "cell 0" in msg and f"pivot {row + 1}" in msg and "not positive definite" in msg, msg
        after = m.call(include_noise=1)
    assert same_bits(after[0], before[0]) and same_bits(after[1], before[1])


def test_a_cell_whose_kuu_is_singular_is_the_factorisations_enotpd(lib):
    """Variance 1e12 with lengthscale 1e6 in the second cell (test_gpu_sgpr.py's failing cell): every entry of Kuu rounds to v, the jitter
    drowns.  The joint call answers with the factorisation's GPRX_ENOTPD naming the cell; the next call on the handle is clean."""
    cid = "F-m50-ns65"
    with Joint(lib, cid) as m:
        before = m.call(include_noise=1)
        bad = m.thetas.copy()
        bad[1] = [1e12, 1e6, 0.0]
        msg = m.call(include_noise=1, thetas=bad, expect=_lib.GPRX_ENOTPD)
        assert "cell 1" in msg, msg
        after = m.call(include_noise=1)
    assert same_bits(after[0], before[0]) and same_bits(after[1], before[1])


# ---- PeakEnsemble.joint_dev --------------------------------------------------------------------------------------------------------------
class _Device:
    """What PeakEnsemble reads of a projector when only joint_dev is exercised."""
    device = 0

    def __init__(self, k):
        self.spatial_mode_count = k


def test_joint_dev_sends_the_modes_in_runs_of_the_engines_batch_size(lib):
    """Five modes with eng.max_cells standing in at 2 go out as runs of 2, 2 and 1 cells into the (K, rows) and (K, Tp, Tp) buffers at
    their offsets: mean and Lc are the one-run call's bit for bit (5, 2 and 1 cells at Tp = 128 all take the launch sequence with the
    fused panel -- no run here changes the Cholesky route, so nothing is left to a bound)."""
    from gpras_amd.ensemble import PeakEnsemble, padded_rows
    from gpras_amd.gpr import GPRAS
    from gpras_amd.synth import make_regression

    k, rows = 5, 70
    x, y, xs = make_regression(200, 4, n_outputs=k, n_test=rows, config=53, unit=99)
    gpr = GPRAS("Matern32")
    gpr.fit(x, y, 10, "kmeans", "adam", max_iter=3)
    ens = PeakEnsemble(gpr, _Device(k))
    tp = padded_rows(rows)

    def run():
        sizes = []
        engines = {id(mod.backend): mod.backend for mod in gpr.models}
        originals = {}
        for key, eng in engines.items():
            originals[key] = eng.predict_joint_batch_dev
            eng.predict_joint_batch_dev = lambda units, *a, _f=originals[key], **kw: (sizes.append(len(units)), _f(units, *a, **kw))[1]
        try:
            mean_dev, lc_dev, _ = ens.joint_dev(xs)
        finally:
            for key, eng in engines.items():
                eng.predict_joint_batch_dev = originals[key]
        try:
            return sizes, mean_dev.to_array((k, rows)), lc_dev.to_array((k, tp, tp))
        finally:
            mean_dev.free()
            lc_dev.free()

    sizes, mean, lc = run()
    assert sizes == [k]
    for eng in {id(mod.backend): mod.backend for mod in gpr.models}.values():
        eng.max_cells = lambda want_grad=False, reserve=0.15: 2  # pretend only two cells fit
    sizes2, mean2, lc2 = run()
    assert sizes2 == [2, 2, 1]
    assert same_bits(mean2, mean) and same_bits(lc2, lc)
    assert not np.any(np.isnan(lc)) and all(np.array_equal(lc[i, rows:, rows:], np.eye(tp - rows)) for i in range(k))
