"""Per-event temporal clipping on the device (gpras_amd/csrc/align.h, gpras_amd/align.py) against the reference's own outputs
(tests/golden/align_ref_golden.npz) and the numpy restatement in the device's summation order (tests/align_numpy.py).

Bounds.  The cutoffs are integers: equal to the fixture's.  The curve equals the restatement's BIT FOR BIT (differences, divisions
and sums are the same IEEE operations in the same order, contraction off) and lies within 4 x max(eps_curve, 2^-52) of the
reference's, eps_curve being the fixture's record of how far the restatement is from the reference.  The shapes are the smallest at
which the kernels can go wrong: columns around a wave (64) and a strip (256), rows around a row tile (32 difference rows) and the
finish kernel's chunk (1024).  aligned_features against the host chain of existing entries: bit for bit, the slabs agreeing.
"""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import align_numpy
from gpras_amd._lib import GPRX_EINVAL, GPRX_OK, DeviceBuffer, ptr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_align_ref import ALIGN_PRESET, HF_COLS, align_plans, align_ref_cases, hydrograph  # noqa: E402
from make_golden_resample_ref import N_HF, N_HF_FULL, N_LF, resample_ref_cases  # noqa: E402

FIX = np.load(os.path.join(GOLDEN, "align_ref_golden.npz"))
CASES = align_ref_cases()
EPS = float(FIX["eps_curve"])
BOUND = 4.0 * max(EPS, 2.0**-52)
GRID = [n for n in CASES if n.startswith("grid/")]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64)[~np.isnan(b)], b.view(np.int64)[~np.isnan(b)]) and np.array_equal(np.isnan(a), np.isnan(b))


@pytest.fixture(scope="module")
def handle(lib):
    h = C.c_void_p()
    assert lib.gprx_al_create(0, C.byref(h)) == GPRX_OK
    yield h
    assert lib.gprx_al_destroy(h) == GPRX_OK


def cutoff_dev(lib, h, combo, threshold=0.95, splits=(), pad=0):
    """The cutoff over `combo` cut into device blocks at the columns `splits`, every block with `pad` columns of NaN padding.
    -> (status, start, stop, rows_used, curve)."""
    T, Ctot = combo.shape
    edges = [0, *splits, Ctot]
    bufs = []
    try:
        for a, b in zip(edges[:-1], edges[1:]):
            block = np.full((T, b - a + pad), np.nan)
            block[:, : b - a] = combo[:, a:b]
            bufs.append(DeviceBuffer.from_array(block))
        n = len(bufs)
        start, stop, used = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
        curve = np.full(T - 1, -7.0)
        rc = lib.gprx_al_cutoff_dev(h, n, (C.c_void_p * n)(*[b.ptr for b in bufs]), (C.c_int64 * n)(*[b - a for a, b in zip(edges[:-1], edges[1:])]),
                                    (C.c_int64 * n)(*[b - a + pad for a, b in zip(edges[:-1], edges[1:])]), T, threshold, C.byref(start),
                                    C.byref(stop), C.byref(used), ptr(curve))
        return rc, start.value, stop.value, used.value, curve[: max(used.value - 1, 0)]
    finally:
        for b in bufs:
            b.free()


def check_case(lib, h, name, **how):
    c = CASES[name]
    rc, start, stop, used, curve = cutoff_dev(lib, h, c["combo"], c["threshold"], **how)
    assert rc == GPRX_OK, lib.gprx_al_last_error(h)
    want, used_want = align_numpy.curve(c["combo"])
    ref = FIX[f"{name}/curve"]
    assert (start, stop) == tuple(FIX[f"{name}/cutoff"]) and used == used_want
    assert same_bits(curve, want), (name, how)
    if not np.all(np.isnan(ref)):
        diff = float(np.max(np.abs(curve - ref)))
        print(f"{name}: max |curve - reference| {diff:.3e}, bound {BOUND:.3e}")
        assert diff <= BOUND
    return curve


# ---- the grid of shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRID)
def test_cutoffs_and_curve_on_every_shape(lib, handle, name):
    check_case(lib, handle, name)


def test_host_matrix_form_and_two_calls_give_the_same_bits(lib):
    from gpras_amd.align import EventAligner

    al = EventAligner()
    for name in ("grid/C549_T130", "grid/C65_T1100", "grid/C1_T2", "nan/second_block"):
        c = CASES[name]
        curve = al.cutoff_curve(c["combo"])
        assert same_bits(curve, align_numpy.curve(c["combo"])[0]) and same_bits(al.cutoff_curve(c["combo"]), curve)
        assert al.get_cutoff(c["combo"]) == tuple(FIX[f"{name}/cutoff"])
    ms = al.stage_timings_ms()
    assert set(ms) == {"scan", "normalisers", "row_sums", "finish"} and all(v > 0.0 for v in ms.values())
    al.close()


# ---- the blocks the columns arrive in -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid/C549_T130", "grid/C257_T34", "const/some"])
def test_the_cut_into_blocks_and_nan_padding_do_not_change_a_bit(lib, handle, name):
    Ctot = CASES[name]["combo"].shape[1]
    one = check_case(lib, handle, name)
    for splits in ((101,), (1, 65, Ctot - 3), (63, 64, 191)):
        assert same_bits(check_case(lib, handle, name, splits=splits), one), splits
    assert same_bits(check_case(lib, handle, name, pad=5), one)
    assert same_bits(check_case(lib, handle, name, splits=(129,), pad=3), one)


# ---- NaN ------------------------------------------------------------------------------------------------------------------------------
def test_nan_trim(lib, handle):
    check_case(lib, handle, "nan/row2")
    check_case(lib, handle, "nan/last_row")
    check_case(lib, handle, "nan/tail", splits=(HF_COLS,))
    curve = check_case(lib, handle, "nan/second_block", splits=(HF_COLS,))  # the NaN lie in the second block only
    assert len(curve) == 28 and same_bits(check_case(lib, handle, "nan/second_block"), curve)
    for row in (0, 1):
        rc, start, stop, used, _ = cutoff_dev(lib, handle, CASES[f"nan/row{row}"]["combo"], splits=(HF_COLS,))
        assert rc == GPRX_EINVAL and used == row and (start, stop) == (-7, -7)
        assert b"NaN trim" in lib.gprx_al_last_error(handle) and f"row {row}".encode() in lib.gprx_al_last_error(handle)
    check_case(lib, handle, "nan/last_row")  # the handle still computes


def test_nan_trim_raises_through_the_class(lib):
    from gpras_amd.align import EventAligner

    al = EventAligner()
    for row in (0, 1):
        with pytest.raises(ValueError, match="NaN trim"):
            al.get_cutoff(CASES[f"nan/row{row}"]["combo"])
    assert al.get_cutoff(CASES["nan/row2"]["combo"]) == (0, 0)
    al.close()


# ---- constant columns, thresholds -----------------------------------------------------------------------------------------------------
def test_constant_columns_and_thresholds(lib, handle):
    check_case(lib, handle, "const/some")
    rc, start, stop, used, curve = cutoff_dev(lib, handle, CASES["const/all"]["combo"])
    assert rc == GPRX_OK and (start, stop, used) == (0, 0, 40) and np.all(np.isnan(curve)) and len(curve) == 39
    low = check_case(lib, handle, "thr/0.5")
    assert same_bits(check_case(lib, handle, "thr/0.999"), low)  # the same field: the threshold moves stop alone
    assert FIX["thr/0.5/cutoff"][1] != FIX["thr/0.999/cutoff"][1]


# ---- clip -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,lds,ldd", [(101, 101, 112), (101, 112, 101), (300, 304, 304), (1, 3, 16)])
def test_clip_rows_and_padding(lib, handle, cols, lds, ldd):
    T, start, stop = 29, 3, 21
    rng = np.random.default_rng(cols + ldd)
    src = np.full((T, lds), np.nan)
    src[:, :cols] = rng.standard_normal((T, cols))
    n = stop - start
    sdev, ddev = DeviceBuffer.from_array(src), DeviceBuffer.from_array(np.full(n * ldd + 7, np.nan))
    try:
        assert lib.gprx_al_clip_dev(handle, sdev.ptr, lds, cols, start, start, ddev.ptr, ldd) == GPRX_OK  # start == stop: nothing
        assert lib.gprx_al_clip_dev(handle, sdev.ptr, lds, cols, stop, start, ddev.ptr, ldd) == GPRX_OK  # numpy's empty slice
        assert lib.gprx_al_synchronize(handle) == GPRX_OK
        assert np.all(np.isnan(ddev.to_array((n * ldd + 7,))))
        assert lib.gprx_al_clip_dev(handle, sdev.ptr, lds, cols, start, stop, ddev.ptr, ldd) == GPRX_OK
        assert lib.gprx_al_synchronize(handle) == GPRX_OK
        flat = ddev.to_array((n * ldd + 7,))
        got = flat[: n * ldd].reshape(n, ldd)
        assert same_bits(got[:, :cols], src[start:stop, :cols])
        assert np.all(got[:, cols:] == 0.0) and not np.any(np.signbit(got[:, cols:]))
        assert np.all(np.isnan(flat[n * ldd :]))  # nothing past the last row
    finally:
        sdev.free()
        ddev.free()


# ---- error codes ----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_handle_usable(lib, handle):
    c = CASES["grid/C65_T34"]
    dev = DeviceBuffer.from_array(c["combo"])
    start, stop = C.c_int64(), C.c_int64()

    def call(n_blocks=1, cols=65, ld=65, rows=34, thr=0.95, block=dev.ptr.value, h=handle):
        return lib.gprx_al_cutoff_dev(h, n_blocks, (C.c_void_p * 4)(block, block, block, block), (C.c_int64 * 4)(cols, 1, 1, 1),
                                      (C.c_int64 * 4)(ld, 1, 1, 1), rows, thr, C.byref(start), C.byref(stop), None, None)

    try:
        for kwargs, word in ((dict(n_blocks=0), b"n_blocks"), (dict(n_blocks=5), b"n_blocks"), (dict(cols=0), b"cols"), (dict(ld=64), b"ld"),
                             (dict(rows=0), b"rows"), (dict(rows=1), b"fewer than 2 rows"), (dict(thr=float("nan")), b"threshold"),
                             (dict(thr=float("-inf")), b"threshold"), (dict(block=None), b"null")):
            assert call(**kwargs) == GPRX_EINVAL and word in lib.gprx_al_last_error(handle), kwargs
        assert call(h=None) == GPRX_EINVAL
        out = DeviceBuffer(8 * 34 * 80)
        assert lib.gprx_al_clip_dev(handle, dev.ptr, 64, 65, 0, 3, out.ptr, 80) == GPRX_EINVAL and b"lds" in lib.gprx_al_last_error(handle)
        assert lib.gprx_al_clip_dev(handle, dev.ptr, 65, 65, 0, 3, out.ptr, 64) == GPRX_EINVAL and b"ldd" in lib.gprx_al_last_error(handle)
        assert lib.gprx_al_clip_dev(handle, dev.ptr, 65, 65, -1, 3, out.ptr, 80) == GPRX_EINVAL
        assert lib.gprx_al_clip_dev(handle, None, 65, 65, 0, 3, out.ptr, 80) == GPRX_EINVAL
        out.free()
        assert call() == GPRX_OK and (start.value, stop.value) == tuple(FIX["grid/C65_T34/cutoff"])
    finally:
        dev.free()


# ---- _align_datasets ------------------------------------------------------------------------------------------------------------------
def test_align_against_the_reference(lib):
    from gpras_amd.align import EventAligner

    al = EventAligner(0.95, ALIGN_PRESET)
    plans = align_plans()
    hf, lf, runs, t = al.align(plans)
    assert same_bits(hf, FIX["align/hf"]) and same_bits(lf, FIX["align/lf"])
    assert list(runs) == list(FIX["align/runs"]) and np.array_equal(t, FIX["align/t"])
    assert [al.cutoffs[p] for p, _, _ in plans] == [tuple(c) for c in FIX["align/cutoffs"]] and al.cutoffs["p2"] == ALIGN_PRESET["p2"]
    # a zero-length event: start == stop, no rows
    flat = np.broadcast_to(100.0 + np.arange(20.0), (9, 20)).copy()
    hf0, lf0, runs0, t0 = al.align([("flat", flat[:, :12], flat[:, 12:])])
    assert al.cutoffs["flat"] == (0, 0) and hf0.shape == (0, 12) and lf0.shape == (0, 8) and len(runs0) == len(t0) == 0
    al.close()


# ---- plan blocks to features ----------------------------------------------------------------------------------------------------------
def _projector(rng, k):
    from gpras_amd.preprocess import EOFProjector

    dry = np.zeros(N_HF, dtype=bool)
    dry[[3, 17, 100]] = True
    n_wet = N_HF - 3
    return EOFProjector(dry, 100.0 + 5.0 * rng.random(N_HF), 102.0 + rng.normal(size=n_wet), rng.uniform(0.5, 1.5, size=n_wet),
                        rng.normal(size=(k, n_wet)) / np.sqrt(k), rng.normal(size=k), rng.uniform(0.5, 2, size=k), "wse")


def _check_features(rows):
    """aligned_features against the host chain gather / resample -> align -> transform, for plans of `rows` rows each."""
    from gpras_amd._lib import load
    from gpras_amd.align import EventAligner
    from gpras_amd.resample import MeshResampler

    geo = resample_ref_cases()["geometry"]["g"]
    rng = np.random.default_rng(11)
    hf_proj, lf_proj = _projector(rng, 6), _projector(rng, 4)
    elev = np.where(np.isnan(geo["cell_elevations"]), 101.0, geo["cell_elevations"]) - 3.0  # below the water: the floor seldom wins
    gather = MeshResampler.nearest(geo["hf_resampler"], N_HF_FULL)
    total = 0
    for lf_rs in (MeshResampler.linear(geo["lf_xy"], geo["hf_xy"], elev, geo["lf_cell_ids"], n_lf=N_LF), MeshResampler.nearest(geo["lf_resampler"], N_LF, elev)):
        plans = [(f"p{i}", hydrograph(rng, T, N_HF_FULL), hydrograph(rng, T, N_LF)) for i, T in enumerate(rows)]
        plans[-1][2][rows[-1] - 3 :, 7] = np.nan  # the LF plan ends in NaN rows: they fall to the trim
        preset = {"p1": (2, rows[1] - 5)} if len(rows) > 1 else {}
        host = EventAligner(0.95, preset)
        hf_al, lf_al, runs_want, t_want = host.align([(p, gather.hf_plan_data(hf), lf_rs.lf_plan_data(lf)) for p, hf, lf in plans])
        assert np.all(np.isfinite(hf_al)) and np.all(np.isfinite(lf_al))
        x_want, y_want = lf_proj.transform(lf_al), hf_proj.transform(hf_al)
        dev = EventAligner(0.95, preset)
        x, y, runs, t = dev.aligned_features(plans, gather, lf_rs, hf_proj, lf_proj)
        assert dev.cutoffs == host.cutoffs and list(runs) == list(runs_want) and np.array_equal(t, t_want)
        assert x.shape == (len(t), 4) and y.shape == (len(t), 6)
        assert same_bits(x, x_want) and same_bits(y, y_want), (float(np.max(np.abs(x - x_want))), float(np.max(np.abs(y - y_want))))
        computed = len(rows) - len(preset)
        assert dev.last_timings_ms["host_link_bytes"] == 8 * (sum(rows) * (N_HF_FULL + N_LF) + len(t) * 10) + 16 * computed
        total = len(t)
        for a in (host, dev, lf_rs):
            a.close()
    slab = C.c_int64()
    assert load().gprx_pca_slab_rows(hf_proj.handle, C.byref(slab)) == GPRX_OK
    return total, int(slab.value)


def test_aligned_features_equal_the_host_chain_inside_one_slab(lib):
    total, slab = _check_features((37, 20, 45))
    assert 0 < total <= slab


def test_aligned_features_equal_the_host_chain_over_several_slabs(lib):
    """GPRX_PCA_CHUNK_DOUBLES = 64 x 112 in a child process: slabs of 64 rows; the first plan alone keeps more rows than one slab
    holds, and the slabs run across the plans' boundaries."""
    code = "import sys; sys.path.insert(0, 'tests'); import test_gpu_align as t; n, slab = t._check_features((150, 40, 90)); print('slabs ok', n > 2 * slab, slab)"
    env = dict(os.environ, GPRX_PCA_CHUNK_DOUBLES=str(64 * 112))
    res = subprocess.run([sys.executable, "-c", code], env=env, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0 and "slabs ok True 64" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
