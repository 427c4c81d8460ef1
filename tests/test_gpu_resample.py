"""LF-to-HF mesh resampling on the device (gpras_amd/csrc/resample.h, gpras_amd/resample.py) against the reference's own outputs
(tests/golden/resample_ref_golden.npz) and the numpy restatement (tests/resample_numpy.py).

Bounds.  The fixture records eps_interp, the largest relative difference between the restatement and the reference
(RasUpskillDataBuilder / RasInterpolaterBuilder.get_lf_plan_data, i.e. scipy's LinearNDInterpolator row by row).  It records 0: a
gather, a comparison, one correctly rounded square root and the three products and sums of the interpolation in scipy's order are the
same IEEE operations on the device (contraction off), so every instantiation is held to the reference bit for bit, NaN positions
equal.  Were eps_interp not 0 the bound would be 4 x eps_interp x max|z| per element.  lf_features against the host chain of
existing entries: bit for bit, the row slabs agreeing.
"""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import resample_numpy
from gpras_amd._lib import GPRX_EINVAL, GPRX_OK, DeviceBuffer, ptr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_resample_ref import N_HF, N_HF_FULL, N_LF, ROWS, resample_ref_cases  # noqa: E402

FIX = np.load(os.path.join(GOLDEN, "resample_ref_golden.npz"))
CASES = resample_ref_cases()
GEO = CASES["geometry"]["g"]
EPS = float(FIX["eps_interp"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64)[~np.isnan(b)], b.view(np.int64)[~np.isnan(b)]) and np.array_equal(np.isnan(a), np.isnan(b))


def within(got, want, zmax, what):
    """Bit for bit when the fixture records eps_interp = 0, else 4 x eps_interp x max|z| per element with NaN positions equal."""
    fin = np.isfinite(want)
    diff = float(np.max(np.abs(got[fin] - want[fin]))) if fin.any() and got.shape == want.shape else np.inf
    print(f"{what}: max |difference| {diff:.3e}, eps_interp {EPS:.3e}")
    if EPS == 0.0:
        return same_bits(got, want)
    return np.array_equal(got[~fin], want[~fin], equal_nan=True) and diff <= 4.0 * EPS * zmax


def resamplers():
    from gpras_amd.resample import MeshResampler

    elev = GEO["cell_elevations"]
    return dict(
        nearest=MeshResampler.nearest(GEO["lf_resampler"], N_LF, elev),
        velocity=MeshResampler.nearest(GEO["lf_resampler"], N_LF, elev, "velocity"),
        linear=MeshResampler.linear(GEO["lf_xy"], GEO["hf_xy"], elev, GEO["lf_cell_ids"], n_lf=N_LF),
        linear_raw=MeshResampler.linear(GEO["lf_xy"], GEO["hf_xy"], None, GEO["lf_cell_ids"], n_lf=N_LF),
        hf=MeshResampler.nearest(GEO["hf_resampler"], N_HF_FULL),
        hf_velocity=MeshResampler.nearest(GEO["hf_resampler"], N_HF_FULL, hydraulic_parameter="velocity"),
    )


def finite(a):
    return float(np.max(np.abs(a[np.isfinite(a)])))


# ---- every instantiation against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ROWS))
def test_every_instantiation_against_the_reference(lib, name):
    b = CASES["blocks"][name]
    rs = resamplers()
    zmax = finite(b["wse"])
    assert within(rs["nearest"].lf_plan_data(b["wse"]), FIX[f"nearest/{name}/lf_plan_data"], zmax, f"nearest {name}")
    assert within(rs["hf"].hf_plan_data(b["hf_wse"]), FIX[f"hf/{name}/wse"], finite(b["hf_wse"]), f"gather {name}")
    vmax = max(finite(b["vx"]), finite(b["vy"]))
    assert within(rs["velocity"].lf_plan_data(b["vx"], b["vy"]), FIX[f"velocity/{name}/lf_plan_data"], vmax, f"velocity {name}")
    assert within(rs["hf_velocity"].hf_plan_data(b["hf_wse"] - 102.0, 103.0 - b["hf_wse"]), FIX[f"hf/{name}/velocity"], 3.0, f"hf velocity {name}")
    lin = rs["linear"]
    got = lin.lf_plan_data(b["wse"])
    assert within(got, FIX[f"linear/{name}/lf_plan_data"], zmax, f"linear {name}")
    # without elevations the NaN of a point outside the hull and of a NaN vertex under any weight stays (scipy's own result)
    raw = rs["linear_raw"].lf_plan_data(b["wse"])
    assert same_bits(raw, resample_numpy.linear(b["wse"], lin.idx, lin.weights))
    assert np.all(np.isnan(raw[:, np.all(lin.idx == -1, axis=1)]))
    ms = np.zeros(1)
    assert lib.gprx_rs_timings(lin.handle, ms.ctypes.data_as(C.POINTER(C.c_double))) == GPRX_OK and ms[0] > 0.0
    for r in rs.values():
        r.close()


def test_first_rows_alone_and_two_runs_give_the_same_bits(lib):
    b = CASES["blocks"]["b"]
    rs = resamplers()
    for kind, args in (("nearest", (b["wse"],)), ("velocity", (b["vx"], b["vy"])), ("linear", (b["wse"],)), ("linear_raw", (b["wse"],))):
        full = rs[kind].lf_plan_data(*args)
        assert same_bits(rs[kind].lf_plan_data(*args), full), kind
        for n in (1, 5, 9, 33):  # inside one group of rows, one row more, and one row more than the linear form's tile of 32
            assert same_bits(rs[kind].lf_plan_data(*(a[:n] for a in args)), full[:n]), (kind, n)
    for r in rs.values():
        r.close()


# ---- device buffers: pitches, padding, bases --------------------------------------------------------------------------------------
def _synthetic(kind, n_src, n_out, seed):
    from gpras_amd.resample import MeshResampler

    rng = np.random.default_rng(seed)
    elev = 100.0 + 5.0 * rng.random(n_out)
    if kind == "linear":
        idx = rng.integers(0, n_src, (n_out, 3))
        w = rng.random((n_out, 3))
        outside = rng.random(n_out) < 0.1
        idx[outside] = -1
        w[outside] = 7.0  # the marker alone decides: these weights must not be used
        return MeshResampler(n_src, idx, w, elev)
    return MeshResampler.nearest(rng.integers(0, n_src, n_out), n_src, elev, "velocity" if kind == "velocity" else "wse")


def _expected(rs, z, z2=None):
    if rs.n_vert == 3:
        return resample_numpy.linear(z, rs.idx, np.where(rs.idx < 0, np.nan, rs.weights), rs.cell_elevations)
    return resample_numpy.velocity(z, z2, rs.idx) if z2 is not None else resample_numpy.nearest(z, rs.idx, rs.cell_elevations)


@pytest.mark.parametrize("kind", ["nearest", "velocity", "linear"])
@pytest.mark.parametrize("n_src,n_out,lds,ldo,shift", [(53, 101, 56, 112, 0), (53, 101, 53, 101, 0), (53, 102, 55, 104, 1), (9000, 20001, 9001, 20016, 0)])
def test_apply_dev_pitches_padding_and_unaligned_base(lib, kind, n_src, n_out, lds, ldo, shift):
    """Vector and scalar stores (even / odd pitch, a base 8 bytes off a 16-byte boundary), padded source rows, the zeroed padding of
    the output, more than one workgroup, and the rows of the host-array call."""
    T = 19
    rs = _synthetic(kind, n_src, n_out, n_src + ldo)
    rng = np.random.default_rng(ldo)
    z = np.full((T, lds), 1e300)  # the padding of the source rows must not be read
    z[:, :n_src] = 100.0 + 5.0 * rng.random((T, n_src))
    z[2, 1] = np.nan
    z2 = None
    if kind == "velocity":
        z2 = np.full((T, lds), 1e300)
        z2[:, :n_src] = rng.standard_normal((T, n_src))
    want = _expected(rs, z[:, :n_src], None if z2 is None else z2[:, :n_src])
    host = rs.lf_plan_data(np.ascontiguousarray(z[:, :n_src]), None if z2 is None else np.ascontiguousarray(z2[:, :n_src]))
    assert same_bits(host, want)
    sdev, s2dev = DeviceBuffer.from_array(z), None if z2 is None else DeviceBuffer.from_array(z2)
    odev = DeviceBuffer.from_array(np.full(T * ldo + shift, np.nan))
    try:
        assert lib.gprx_rs_apply_dev(rs.handle, T, sdev.ptr, lds, None if s2dev is None else s2dev.ptr, odev.at(shift), ldo) == GPRX_OK
        assert lib.gprx_rs_synchronize(rs.handle) == GPRX_OK
        flat = odev.to_array((T * ldo + shift,))
        got = flat[shift:].reshape(T, ldo)
        assert np.all(np.isnan(flat[:shift]))  # nothing before the base was written
        assert same_bits(got[:, :n_out], host)
        assert np.all(got[:, n_out:] == 0.0) and not np.any(np.signbit(got[:, n_out:]))
    finally:
        for b in (sdev, s2dev, odev):
            if b is not None:
                b.free()
        rs.close()


def test_kernel_indexes_past_two_to_the_31(lib):
    """T x n_hf = 2 200 x 1 000 002 > 2^31 elements: one 17.6 GB output of the linear kernel; rows on both sides of element 2^31."""
    T, n_out, n_src = 2200, 1_000_002, 1000
    assert T * n_out > 2**31
    rs = _synthetic("linear", n_src, n_out, 31)
    z = 100.0 + 5.0 * np.random.default_rng(32).random((T, n_src))
    src = DeviceBuffer.from_array(z)
    out = DeviceBuffer(8 * T * n_out)
    try:
        assert lib.gprx_rs_apply_dev(rs.handle, T, src.ptr, n_src, None, out.ptr, n_out) == GPRX_OK
        assert lib.gprx_rs_synchronize(rs.handle) == GPRX_OK
        first_past = 2**31 // n_out  # the row that holds element 2^31
        for t in (0, 1, 1100, first_past - 1, first_past, first_past + 1, T - 2, T - 1):
            row = np.empty(n_out)
            assert lib.gprx_memcpy_d2h(0, ptr(row), out.at(t * n_out), row.nbytes) == GPRX_OK
            assert same_bits(row, _expected(rs, z[t : t + 1])[0]), t
    finally:
        src.free()
        out.free()
        rs.close()


# ---- LF rows to features ----------------------------------------------------------------------------------------------------------
def _projector(rng, k=6):
    from gpras_amd.preprocess import EOFProjector

    dry = np.zeros(N_HF, dtype=bool)
    dry[[3, 17, 100]] = True
    n_wet = N_HF - 3
    return EOFProjector(dry, 100.0 + 5.0 * rng.random(N_HF), 102.0 + rng.normal(size=n_wet), rng.uniform(0.5, 1.5, size=n_wet),
                        rng.normal(size=(k, n_wet)) / np.sqrt(k), rng.normal(size=k), rng.uniform(0.5, 2, size=k), "wse")


def _check_features(T):
    from gpras_amd.resample import MeshResampler

    rng = np.random.default_rng(7)
    proj = _projector(rng)
    elev = np.where(np.isnan(GEO["cell_elevations"]), 101.0, GEO["cell_elevations"])
    z = 100.0 + 5.0 * rng.random((T, N_LF))
    vy = rng.standard_normal((T, N_LF))
    got = None
    for rs, args in ((MeshResampler.linear(GEO["lf_xy"], GEO["hf_xy"], elev, GEO["lf_cell_ids"], n_lf=N_LF), (z,)),
                     (MeshResampler.nearest(GEO["lf_resampler"], N_LF, elev), (z,)),
                     (MeshResampler.nearest(GEO["lf_resampler"], N_LF, hydraulic_parameter="velocity"), (z - 102.0, vy))):
        field = rs.lf_plan_data(*args)
        assert np.all(np.isfinite(field))
        want = proj.transform(field)
        got = rs.lf_features(args[0], proj, *args[1:])
        assert got.shape == (T, proj.spatial_mode_count) and same_bits(got, want), float(np.max(np.abs(got - want)))
        assert same_bits(rs.lf_features(args[0], proj, *args[1:]), got)
        assert rs.last_timings_ms["host_link_bytes"] == 8 * (T * N_LF * len(args) + T * proj.spatial_mode_count)
        rs.close()
    slab = C.c_int64()
    from gpras_amd._lib import load

    assert load().gprx_pca_slab_rows(proj.handle, C.byref(slab)) == GPRX_OK
    return got, int(slab.value)


def test_lf_features_equal_the_host_chain_inside_one_slab(lib):
    _, slab = _check_features(37)
    assert slab >= 37


def test_lf_features_equal_the_host_chain_over_three_slabs(lib):
    """GPRX_PCA_CHUNK_DOUBLES = 64 x 112 in a child process: slabs of 64 rows, T = 150 = 64 + 64 + 22."""
    code = "import sys; sys.path.insert(0, 'tests'); import test_gpu_resample as t; z, slab = t._check_features(150); print('slabs ok', z.shape, slab)"
    env = dict(os.environ, GPRX_PCA_CHUNK_DOUBLES=str(64 * 112))
    res = subprocess.run([sys.executable, "-c", code], env=env, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0 and "slabs ok (150, 6) 64" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


# ---- error codes ------------------------------------------------------------------------------------------------------------------
def test_error_codes_leave_the_handle_usable(lib):
    idx = np.ascontiguousarray(GEO["lf_resampler"], dtype=np.int32)
    elev = GEO["cell_elevations"]
    h = C.c_void_p()

    def create(n_vert, ix, w=None, el=elev, n_src=N_LF):
        return lib.gprx_rs_create(0, n_src, N_HF, n_vert, ptr(ix), None if w is None else ptr(w), None if el is None else ptr(el), C.byref(h))

    bad = idx.copy()
    bad[7] = N_LF
    assert create(1, bad) == GPRX_EINVAL and h.value is None  # an index out of range
    assert b"outside [0, n_src)" in lib.gprx_rs_last_error(None)
    bad[7] = -1
    assert create(1, bad) == GPRX_EINVAL  # the outside marker belongs to the linear form
    assert create(2, idx) == GPRX_EINVAL and create(0, idx) == GPRX_EINVAL  # a wrong n_vert
    idx3 = np.ascontiguousarray(np.stack([idx, idx, idx], axis=1))
    w3 = np.full((N_HF, 3), 1.0 / 3.0)
    assert create(3, idx3) == GPRX_EINVAL and create(1, idx, w3) == GPRX_EINVAL  # weights that do not go with n_vert
    part = idx3.copy()
    part[5] = [-1, 2, 3]
    assert create(3, part, w3) == GPRX_EINVAL  # neither three vertices nor the marker
    assert create(1, idx, n_src=2**28 + 1) == GPRX_EINVAL and create(1, idx, n_src=2**28) == GPRX_OK and lib.gprx_rs_destroy(h) == GPRX_OK
    assert create(1, idx, n_src=0) == GPRX_EINVAL and lib.gprx_rs_create(0, N_LF, N_HF, 1, None, None, None, C.byref(h)) == GPRX_EINVAL
    part[5] = -1
    h3 = C.c_void_p()
    assert lib.gprx_rs_create(0, N_LF, N_HF, 3, ptr(part), ptr(w3), ptr(elev), C.byref(h3)) == GPRX_OK
    assert create(1, idx) == GPRX_OK
    z = np.ascontiguousarray(CASES["blocks"]["a"]["wse"])
    T = z.shape[0]
    src, out = DeviceBuffer.from_array(z), DeviceBuffer(8 * T * 112)
    try:
        assert lib.gprx_rs_apply_dev(h, T, src.ptr, N_LF, None, out.ptr, N_HF - 1) == GPRX_EINVAL  # ldo < n_out
        assert b"ldo" in lib.gprx_rs_last_error(h)
        assert lib.gprx_rs_apply_dev(h, T, src.ptr, N_LF - 1, None, out.ptr, 112) == GPRX_EINVAL  # lds < n_src
        assert lib.gprx_rs_apply_dev(h, -1, src.ptr, N_LF, None, out.ptr, 112) == GPRX_EINVAL
        assert lib.gprx_rs_apply_dev(h, T, None, N_LF, None, out.ptr, 112) == GPRX_EINVAL
        assert lib.gprx_rs_apply_dev(h, T, src.ptr, N_LF, src.ptr, out.ptr, 112) == GPRX_EINVAL  # velocity on a handle with a floor
        assert lib.gprx_rs_apply_dev(h3, T, src.ptr, N_LF, src.ptr, out.ptr, 112) == GPRX_EINVAL  # velocity on a linear handle
        host = np.empty((T, N_HF))
        assert lib.gprx_rs_apply(h, ptr(z), ptr(z), T, ptr(host)) == GPRX_EINVAL and lib.gprx_rs_apply(h, None, None, T, ptr(host)) == GPRX_EINVAL
        assert lib.gprx_rs_apply_dev(h, 0, None, N_LF, None, None, 112) == GPRX_OK  # no rows: nothing to do
        # after every refusal the handles still compute
        assert lib.gprx_rs_apply_dev(h, T, src.ptr, N_LF, None, out.ptr, 112) == GPRX_OK and lib.gprx_rs_synchronize(h) == GPRX_OK
        assert same_bits(out.to_array((T, 112))[:, :N_HF], FIX["nearest/a/lf_plan_data"])
        assert lib.gprx_rs_apply(h3, ptr(z), None, T, ptr(host)) == GPRX_OK
        col5 = np.where(np.isnan(elev[5]), np.nan, elev[5])
        assert np.array_equal(host[:, 5], np.full(T, col5), equal_nan=True)  # the marked point: NaN, hence its elevation
    finally:
        src.free()
        out.free()
        lib.gprx_rs_destroy(h)
        lib.gprx_rs_destroy(h3)
