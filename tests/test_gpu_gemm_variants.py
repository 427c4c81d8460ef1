"""Every variant of the GEMM dispatcher (csrc/gemm_f64.h: launch_gemm_t / launch_gemm / launch_gemm_splitk), called directly
through gprx_gemm_batched / gprx_gemm_splitk and held to a DERIVED bound against a longdouble reference (blocks_reference.py):

    |got - ref| <= 2 (K + 2) 2^-53 (|alpha| |op(A)| |op(B)| + |beta| |C0|)      (split-K: K + nsplit + 2)

which holds for any order of the k sum.  Every output lives in a buffer larger than the result (ldc > N, rows below M, gaps
between batch entries and cells) that is pre-filled with one NaN bit pattern: afterwards every element outside the specified
result must hold those bits, and with beta == 0 the result region starts as that NaN too, so a tile nobody wrote shows.  The
padding of the INPUTS is NaN as well: an operand read past its rows or columns poisons the result.  Every batch entry and cell
has its own random data; all strides are even, all operands 16-byte aligned.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

import blocks_reference as br
from gpras_amd import _lib
from gpras_amd._lib import DeviceBuffer

pytestmark = pytest.mark.gpu

LD = br.LD
NT, NN, TN = (0, 1), (0, 0), (1, 0)
PAIRS = [NT, NN, TN]
TILES = [64, 128]
OK = _lib.GPRX_OK


def _operands(rng, ta, tb, m, n, k, flags):
    """Random A and B as stored; triangular where a flag promises zeros (the kernel skips those k ranges)."""
    oa, ob = rng.standard_normal((m, k)), rng.standard_normal((k, n))
    if flags & _lib.GEMM_A_LOWER:
        oa = np.tril(oa)
    if flags & _lib.GEMM_A_UPPER:
        oa = np.triu(oa)
    if flags & _lib.GEMM_B_LOWER:
        ob = np.tril(ob)
    if flags & _lib.GEMM_B_UPPER:
        ob = np.triu(ob)
    return (oa.T.copy() if ta else oa), (ob.T.copy() if tb else ob)


def _masks(m, n, flags, tile):
    """(written, checked): with C_LOWER the tiles on or below the block diagonal AT THE LAUNCHED TILE SIZE are stored whole, the
    elements with col <= row are specified."""
    i, j = np.arange(m)[:, None], np.arange(n)[None, :]
    if flags & _lib.GEMM_C_LOWER:
        return (j // tile <= i // tile), (j <= i) & np.ones((m, n), bool)
    full = np.ones((m, n), bool)
    return full, full


class Case:
    """One product per (cell, entry): operands, C0, reference and magnitude, built once and launched at any tile size."""

    def __init__(self, pair, m, n, k, alpha, beta, flags=0, batch=1, cells=1, alpha_tab=None, alpha_stride=0, seed=0, ldb=None, ldc=None):
        self.ta, self.tb = pair
        self.m, self.n, self.k, self.alpha, self.beta, self.flags = m, n, k, alpha, beta, flags
        self.batch, self.cells, self.alpha_tab, self.alpha_stride = batch, cells, alpha_tab, alpha_stride
        self.ldb, self.ldc = ldb, ldc
        rng = np.random.default_rng([m, n, k, flags, batch, cells, seed, 2 * self.ta + self.tb])
        self.ops, self.c0, self.ref, self.mag = {}, {}, {}, {}
        for c in range(cells):
            al = alpha if alpha_tab is None else float(alpha_tab[c * alpha_stride])
            for e in range(batch):
                a, b = _operands(rng, self.ta, self.tb, m, n, k, flags)
                c0 = rng.standard_normal((m, n))
                self.ops[c, e], self.c0[c, e] = (a, b), c0
                self.ref[c, e], self.mag[c, e] = br.gemm_ref(self.ta, self.tb, al, a, b, beta, c0)

    def images(self, tile):
        a0, b0 = self.ops[0, 0]
        pad = dict(cells=self.cells, batch=self.batch, extra_rows=3)
        pa = br.Image(fill=np.nan, gap=10, cell_gap=14, A=(*a0.shape, a0.shape[1] + 6), **pad)
        pb = br.Image(fill=np.nan, gap=10, cell_gap=14, B=(*b0.shape, self.ldb or b0.shape[1] + 6), **pad)
        pc = br.Image(gap=12, cell_gap=18, C=(self.m, self.n, self.ldc or self.n + 6), **pad)  # (strides unlike those of B)
        written, checked = _masks(self.m, self.n, self.flags, tile)
        for (c, e), (a, b) in self.ops.items():
            pa.view("A", c, None, e)[...] = a
            pb.view("B", c, None, e)[...] = b
            if self.beta != 0.0:
                pc.set_result("C", self.c0[c, e], c, e, written)
            else:
                pc.mark_result("C", c, e, written)  # (stays NaN: a tile that is never written shows)
        return pa, pb, pc, checked

    def check(self, pc, got_flat, checked, what, nsplit=0):
        pc.assert_unchanged_except(got_flat, [], what)
        with np.errstate(invalid="ignore"):
            for key in self.ref:
                br.assert_gemm(pc.view("C", key[0], got_flat, key[1]), self.ref[key], self.mag[key], self.k, checked, nsplit, f"{what} cell/entry {key}")

    def run(self, lib, tile, what=""):
        pa, pb, pc, checked = self.images(tile)
        da, db, dc = DeviceBuffer.from_array(pa.flat), DeviceBuffer.from_array(pb.flat), DeviceBuffer.from_array(pc.flat)
        dt = DeviceBuffer.from_array(self.alpha_tab) if self.alpha_tab is not None else None
        two_level = self.cells > 1 or dt is not None
        rc = lib.gprx_gemm_batched(0, self.ta, self.tb, self.m, self.n, self.k, self.alpha, da.ptr, pa.ld("A"), db.ptr, pb.ld("B"), self.beta, dc.ptr, pc.ld("C"),
                                   self.flags, tile, self.batch, pa.stride["A"], pb.stride["B"], pc.stride["C"], self.cells, pa.cs if two_level else 0,
                                   pb.cs if two_level else 0, pc.cs if two_level else 0, dt.ptr if dt else None, self.alpha_stride, None, 0)
        assert rc == OK, _lib.last_error()
        got = dc.to_array(pc.flat.shape)
        for d in (da, db, dc, dt):
            if d is not None:
                d.free()
        self.check(pc, got, checked, f"{what} tile {tile}")

    def run_splitk(self, lib, kchunk, what=""):
        pa, pb, pc, checked = self.images(64)
        nsplit = -(-self.k // kchunk)
        ws_cell = nsplit * self.m * self.n + 22  # larger than needed
        ws = br.canary(self.cells * ws_cell)
        da, db, dc, dw = (DeviceBuffer.from_array(x) for x in (pa.flat, pb.flat, pc.flat, ws))
        dt = DeviceBuffer.from_array(self.alpha_tab) if self.alpha_tab is not None else None
        rc = lib.gprx_gemm_splitk(0, self.ta, self.tb, self.m, self.n, self.k, self.alpha, da.ptr, pa.ld("A"), db.ptr, pb.ld("B"), self.beta, dc.ptr, pc.ld("C"),
                                  dw.ptr, kchunk, self.cells, pa.cs, pb.cs, pc.cs, ws_cell, dt.ptr if dt else None, self.alpha_stride)
        assert rc == OK, _lib.last_error()
        got, gws = dc.to_array(pc.flat.shape), dw.to_array(ws.shape).reshape(self.cells, ws_cell)
        for d in (da, db, dc, dw, dt):
            if d is not None:
                d.free()
        self.check(pc, got, checked, what, nsplit)
        assert np.all(br.is_canary(gws[:, nsplit * self.m * self.n:])), f"{what}: the workspace was written past the slabs of a cell"
        assert not np.any(np.isnan(gws[:, : nsplit * self.m * self.n])), f"{what}: a slab of the workspace was not written"


# ---- C_LOWER without operand flags: the Cholesky update --------------------------------------------------------------------------------
@pytest.mark.parametrize("k,beta", [(64, 1.0), (192, 1.0), (64, 0.0)])
def test_lower_trapezoid(lib, k, beta):
    """M = 704, N = 320: 11 x 5 tiles of 64 -- the triangle, then bands of 4 + 2 tile rows below it (the `bid >= tri` branch), 45
    workgroups (the XCD remap with nwg % 8 != 0).  K = 64 with beta: LDS-DMA operands and prefetched C; K = 192: no prefetch."""
    case = Case(NT, 704, 320, k, -1.0, beta, _lib.GEMM_C_LOWER)
    for tile in TILES:
        case.run(lib, tile, f"lower trapezoid K={k} beta={beta}")


def test_lower_square_many_bands(lib):
    """M = N = 640: ten tile rows, so the band decode S(b) runs past two bands."""
    case = Case(NT, 640, 640, 32, -1.0, 1.0, _lib.GEMM_C_LOWER)
    for tile in TILES:
        case.run(lib, tile, "lower square")


@pytest.mark.parametrize("batch", [8, 16, 3, 12])
def test_lower_cell_xcd(lib, batch):
    """batch 8 and 16 switch the (workgroup, entry) remap on, 3 and 12 leave it off; six workgroups per entry."""
    case = Case(NT, 192, 192, 64, -1.0, 1.0, _lib.GEMM_C_LOWER, batch=batch)
    for tile in TILES:
        case.run(lib, tile, f"cell_xcd lower batch {batch}")


@pytest.mark.parametrize("batch", [8, 16, 3, 12])
def test_dense_cell_xcd(lib, batch):
    case = Case(NT, 128, 192, 64, 0.7, 0.0, 0, batch=batch)
    for tile in TILES:
        case.run(lib, tile, f"cell_xcd dense batch {batch}")


# ---- dense products ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("k", [144, 48])
def test_dense_ragged_general_path(lib, pair, k):
    """(200, 136, K) with beta == 0: the register-staged kernels, K above and below 128, at the dispatcher's own tile choice too."""
    case = Case(pair, 200, 136, k, 0.7, 0.0)
    for tile in (0, 64, 128):
        case.run(lib, tile, f"ragged {pair} K={k}")


@pytest.mark.parametrize("pair", PAIRS)
def test_dense_full_tiles_beta0(lib, pair):
    """(128, 192, 256) on full 64 x 64 tiles: the LDS-DMA kernels of all three transpose pairs, no C prefetch."""
    Case(pair, 128, 192, 256, 0.7, 0.0).run(lib, 64, f"full tiles {pair}")


# ---- two-level batches -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES)
def test_two_level_batches_as_trtri_lower_launches_them(lib, tile):
    """The two calls of trtri_lower's level s = 128 with a ragged pair (n1 = 128, n2 = 64): T21 = L21 X11 with B_LOWER, then
    X21 = alpha X22 T21 with A_LOWER; 2 entries in each of 3 cells, per-cell alpha at stride 5, all three cell strides different."""
    tab = np.zeros(11)
    tab[[0, 5, 10]] = [1.0, -0.6, 1.7]
    for m, n, k, flag in [(64, 128, 128, _lib.GEMM_B_LOWER), (64, 128, 64, _lib.GEMM_A_LOWER)]:
        case = Case(NN, m, n, k, 0.0, 0.0, flag, batch=2, cells=3, alpha_tab=tab, alpha_stride=5)
        pa, pb, pc, _ = case.images(tile)
        assert len({pa.cs, pb.cs, pc.cs}) == 3
        case.run(lib, tile, f"two-level flag {flag}")


# ---- rowsq: the product is not stored ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [100, 256])
@pytest.mark.parametrize("n", [128, 320])
def test_rowsq_epilogue_and_final_sum(lib, m, n):
    """The launch of the predictive variance (NT, tile 64, K = N, op(B) upper triangular): C keeps its canary, the 2 * tiles_n slabs
    add up to the row sums of squares of alpha op(A) op(B); then rowsq_final_kernel on those slabs.

    Bound of a row sum: v_ij = alpha acc_ij is off by d_ij <= (K + 2) u mag_ij (as above), so sum_j v_ij^2 is off by at most
    sum_j (2 |ref_ij| d_ij + d_ij^2), plus (N + 1) u sum_j v_ij^2 for the N squarings and additions in any order (16 per lane, 4 shuffle
    steps, 2 * tiles_n slabs: fewer than N), all times 2 for the rounding of the reference."""
    k, alpha, tile = n, 0.7, 64
    for flags in (_lib.GEMM_B_UPPER, 0):
        case = Case(NT, m, n, k, alpha, 0.0, flags, seed=1)
        pa, pb, pc, _ = case.images(tile)
        pc.result[:] = False  # nothing of C is part of the result
        nparts = 2 * (-(-n // tile))
        ldr = m + 10
        slabs = br.canary(nparts * ldr + 6)
        da, db, dc, dr = (DeviceBuffer.from_array(x) for x in (pa.flat, pb.flat, pc.flat, slabs))
        rc = lib.gprx_gemm_batched(0, 0, 1, m, n, k, alpha, da.ptr, pa.ld("A"), db.ptr, pb.ld("B"), 0.0, dc.ptr, pc.ld("C"), flags, tile, 1, 0, 0, 0, 1, 0, 0, 0, None, 0,
                                   dr.ptr, ldr)
        assert rc == OK, _lib.last_error()
        pc.assert_unchanged_except(dc.to_array(pc.flat.shape), [], "rowsq: C")
        got = dr.to_array(slabs.shape)
        body = got[: nparts * ldr].reshape(nparts, ldr)
        assert np.all(br.is_canary(body[:, m:])) and np.all(br.is_canary(got[nparts * ldr:])), "rowsq: slabs written past row M"
        assert not np.any(np.isnan(body[:, :m])), "rowsq: a slab entry was not written"
        assert np.all(body[:, :m] >= 0.0)
        ref, mag = case.ref[0, 0], case.mag[0, 0]
        d = (k + 2) * br.U * mag
        ref_rows = np.sum(ref * ref, axis=1)
        bound = 2.0 * (np.sum(2.0 * np.abs(ref) * d + d * d, axis=1) + (n + 1) * br.U * ref_rows)
        err = np.abs(np.sum(body[:, :m].astype(LD), axis=0) - ref_rows)
        assert np.all(err <= bound), f"rowsq flags {flags}: worst err / bound {float(np.max(err / bound)):.3e}"
        # rowsq_final_kernel: out[row] = base - sum of the slabs, in slab order
        base = 2.5
        out = br.canary(m + 5)
        do = DeviceBuffer.from_array(out)
        rc = lib.gprx_reduce_probe(0, _lib.REDUCE_ROWSQ_FINAL, dr.ptr, ldr, None, m, nparts, base, 0.0, 0, None, 0, do.ptr, 1, 0, 0, 0, 0, None, None, 0)
        assert rc == OK, _lib.last_error()
        res = do.to_array(out.shape)
        assert np.all(br.is_canary(res[m:]))
        tot = np.sum(body[:, :m].astype(LD), axis=0)
        assert np.all(np.abs(res[:m].astype(LD) - (LD(base) - tot)) <= 2.0 * (nparts + 1) * br.U * (abs(base) + tot))
        for dbuf in (da, db, dc, dr, do):
            dbuf.free()


# ---- split-K ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("cells", [1, 3])
def test_splitk_ragged_last_slice(lib, pair, beta, cells):
    """K = 416 in slices of 128: four slabs, the last 32 wide; per-cell alpha from a table with alpha = 0.0 passed, as the sparse path calls it."""
    tab = np.zeros(2 * cells + 1)
    tab[::2][:cells] = [0.7, -1.1, 0.4][:cells]
    Case(pair, 128, 96, 416, 0.0, beta, cells=cells, alpha_tab=tab, alpha_stride=2).run_splitk(lib, 128, f"split-K {pair} beta {beta} cells {cells}")


def test_splitk_full_tiles_and_plain_alpha(lib):
    """NT on full 64 x 64 tiles takes the LDS-DMA kernel with K slices (the A A^T of the sparse path); no alpha table (the EOF fit)."""
    Case(NT, 128, 128, 416, 0.7, 1.0).run_splitk(lib, 128, "split-K NT full tiles")
    Case(NT, 128, 96, 416, 1.0, 0.0).run_splitk(lib, 128, "split-K NT plain alpha")


@pytest.mark.parametrize("cells", [1, 3])
def test_splitk_vector_form(lib, cells):
    """NN with N = 1, ldb = 1, ldc = 1: the matrix-vector product of the sparse path."""
    tab = np.zeros(2 * cells + 1)
    tab[::2][:cells] = [0.7, -1.1, 0.4][:cells]
    Case(NN, 128, 1, 416, 0.0, 0.0, cells=cells, alpha_tab=tab, alpha_stride=2, ldb=1, ldc=1).run_splitk(lib, 128, f"split-K vector cells {cells}")


# ---- what the probes refuse --------------------------------------------------------------------------------------------------------------
def test_probes_reject_what_the_kernels_cannot_take(lib):
    """By return code only: nothing of this reaches a kernel."""
    buf = DeviceBuffer(8 * 4096)
    p, off = buf.ptr, buf.at(1)

    def batched(m=64, n=64, k=64, a=p, lda=64, b=p, ldb=64, c=p, ldc=64, sa=0, sb=0, sc=0, ca=0, cb=0, cc=0, tile=64, pair=NT):
        return lib.gprx_gemm_batched(0, pair[0], pair[1], m, n, k, 1.0, a, lda, b, ldb, 0.0, c, ldc, 0, tile, 1, sa, sb, sc, 1, ca, cb, cc, None, 0, None, 0)

    def rowsq(tile=64, batch=1, cells=1, ld=64):
        return lib.gprx_gemm_batched(0, 0, 1, 64, 64, 64, 1.0, p, 64, p, 64, 0.0, p, 64, 0, tile, batch, 0, 0, 0, cells, 0, 0, 0, None, 0, p, ld)

    def splitk(k=64, kchunk=32, a=p, lda=64, ws=p, ca=0, ws_cell=0, cells=1):
        return lib.gprx_gemm_splitk(0, 0, 1, 32, 32, k, 1.0, a, lda, p, 64, 0.0, p, 32, ws, kchunk, cells, ca, 0, 0, ws_cell, None, 0)

    bad = [batched(lda=65), batched(ldb=65), batched(k=40), batched(a=off), batched(b=off), batched(c=off), batched(sa=1), batched(sb=3),
           batched(sc=5), batched(ca=7), batched(cb=9), batched(cc=11), batched(tile=32), batched(pair=(1, 1)), batched(lda=32), batched(a=None),
           rowsq(tile=0), rowsq(batch=2), rowsq(cells=2), rowsq(ld=32),
           splitk(k=40), splitk(kchunk=24), splitk(lda=65), splitk(a=off), splitk(ws=off), splitk(ca=3), splitk(ws=None),
           splitk(cells=2, ws_cell=64)]
    assert bad == [_lib.GPRX_EINVAL] * len(bad)
    # C is read and written element by element: an odd ldc is taken (the vector form of the sparse path has ldc = 1, tested above)
    buf.free()


# ---- the switches that are read once per process ------------------------------------------------------------------------------------------
def test_register_staged_kernels_in_a_fresh_process():
    """GPRX_GEMM_DMA* = 0 and GPRX_CELL_XCD = 0 are read at the first launch of a process: one child re-runs the dense and lower cases
    of this file with them, where the register-staged kernels must meet the same bound."""
    env = dict(os.environ, GPRX_GEMM_DMA="0", GPRX_GEMM_DMA_NN="0", GPRX_GEMM_DMA_TN="0", GPRX_CELL_XCD="0")
    res = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "test_lower or test_dense"],
                         env=env, capture_output=True, text=True, timeout=240, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-2000:]
    assert " passed" in res.stdout and "skipped" not in res.stdout and "failed" not in res.stdout, res.stdout[-2000:]
