"""Every host driver and reduction of csrc/solve.h, called directly through the probe entry points, against longdouble references
(blocks_reference.py).  The inputs are built on the host -- L is the longdouble Cholesky factor of an RBF matrix rounded to double,
inv_diag the longdouble inverses of its 64 x 64 diagonal blocks rounded to double -- so nothing here depends on the device
factorisation.  Two matrices per size (noise 1e-2 and 1e-6), a third and fourth per cell of a batched call.

Bounds: the kernels use explicit block inverses, so the constant of their backward error is not derivable; golden/blocks_bounds.json
records what a float64 numpy restatement of the same block algorithm reaches on these very matrices (golden/make_blocks_bounds.py),
as a componentwise ratio, and the kernels get 8 x that (another summation order, FMA contraction).  On the noise-1e-2 matrices every
solve and inverse is also within 1e-11 relative of the reference, the factorisation tolerance of test_gpu_blocks.py.  All outputs
live in canary-filled buffers (see test_gpu_gemm_variants.py); inputs must come back unchanged bit for bit.
"""

import functools
import os
import re

import numpy as np
import pytest

import blocks_reference as br
from gpras_amd import _lib
from gpras_amd._lib import DeviceBuffer

pytestmark = pytest.mark.gpu

LD, NB, OK = br.LD, br.NB, _lib.GPRX_OK
SLACK = 8.0
SIZES_NOISES = [(n, noise) for n in br.SIZES for noise in br.NOISES]


Image = br.Image


def _limit(key):
    return SLACK * br.bounds()[key]


def _key(kind, n, noise, seed):
    return f"{kind}/n{n}/{br.tag(noise)}/seed{seed}"


@functools.lru_cache(maxsize=None)
def _trsv_ref(n, noise, seed, transpose):
    return br.solve_lower_ld(br.solve_inputs(n, noise, seed)[0], br.rhs(n, 0, seed), transpose)


@functools.lru_cache(maxsize=None)
def _trsm_ref(n, noise, seed, ncols):
    return br.solve_lower_ld(br.solve_inputs(n, noise, seed)[0], br.rhs(n, ncols, seed))


def _factor_image(cells, n, noise, **more):
    img = Image(cells, L=(n, n, n + 6), inv=(n, NB, NB), **more)
    for c in range(cells):
        low, inv = br.solve_inputs(n, noise, c)
        img.view("L", c)[...] = low
        img.view("inv", c)[...] = inv.reshape(n, NB)
    return img


def _check_solution(got, ref, low, b, n, noise, key, transpose=False):
    assert not np.any(np.isnan(got)), f"{key}: part of the solution was not written"
    ratio = br.solve_ratio(low, got, b, transpose)
    assert ratio <= _limit(key), f"{key}: residual ratio {ratio:.3e}, allowed {_limit(key):.3e}"
    if noise == br.NOISES[0]:
        assert br.rel_err(got, ref) < 1e-11, f"{key}: {br.rel_err(got, ref):.3e} from the reference"


# ---- vector right-hand sides -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,noise", SIZES_NOISES)
def test_trsv_lower_in_place(lib, n, noise):
    """Forward and backward, one system and three (their cell stride larger than needed), block counts 1 to 5."""
    for batch in (1, 3):
        for transpose in (0, 1):
            img = _factor_image(batch, n, noise, b=(n, 1, 1))
            for c in range(batch):
                img.view("b", c)[:, 0] = br.rhs(n, 0, c)
            img.upload()
            rc = lib.gprx_trsv_lower(0, img.ptr("L"), n + 6, img.ptr("inv"), img.ptr("b"), n, transpose, batch, img.cs, None)
            assert rc == OK, _lib.last_error()
            got = img.download()
            img.assert_unchanged_except(got, ["b"], f"trsv n={n} batch={batch} transpose={transpose}")
            for c in range(batch):
                _check_solution(img.view("b", c, got)[:, 0], _trsv_ref(n, noise, c, bool(transpose)), br.solve_inputs(n, noise, c)[0], br.rhs(n, 0, c),
                                n, noise, _key("trsv_bwd" if transpose else "trsv_fwd", n, noise, c), bool(transpose))


@pytest.mark.parametrize("n,noise", SIZES_NOISES)
def test_trsv_lower_backward_with_work_vector(lib, n, noise):
    """The two-steps-per-launch path (the pair loop leaves 0 or 1 single steps by the parity of the block count): b only receives the
    solution, `work` is used up, L and inv_diag are untouched; the solution is the in-place one bit for bit, as solve.h promises."""
    outs = []
    for with_work in (True, False):
        img = _factor_image(1, n, noise, b=(n, 1, 1), work=(n, 1, 1))
        img.view("work" if with_work else "b")[:, 0] = br.rhs(n, 0, 0)
        img.upload()
        rc = lib.gprx_trsv_lower(0, img.ptr("L"), n + 6, img.ptr("inv"), img.ptr("b"), n, 1, 1, 0, img.ptr("work") if with_work else None)
        assert rc == OK, _lib.last_error()
        got = img.download()
        img.assert_unchanged_except(got, ["b", "work"] if with_work else ["b"], f"trsv work={with_work} n={n}")
        outs.append(img.view("b", 0, got)[:, 0].copy())
    _check_solution(outs[0], _trsv_ref(n, noise, 0, True), br.solve_inputs(n, noise)[0], br.rhs(n, 0, 0), n, noise, _key("trsv_bwd", n, noise, 0), True)
    assert np.array_equal(outs[0], outs[1])


# ---- matrix right-hand sides -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,noise", SIZES_NOISES)
def test_trsm_lower_left(lib, n, noise):
    """64 columns (full tiles: LDS-DMA NN kernel), 40 and 200 (ragged), ldb > ncols, one cell and three."""
    for cells in (1, 3):
        for ncols in br.TRSM_NCOLS:
            img = _factor_image(cells, n, noise, B=(n, ncols, ncols + 6))
            for c in range(cells):
                img.view("B", c)[...] = br.rhs(n, ncols, c)
            img.upload()
            rc = lib.gprx_trsm_lower_left(0, img.ptr("L"), n + 6, img.ptr("inv"), img.ptr("B"), ncols + 6, n, ncols, cells, img.cs, None)
            assert rc == OK, _lib.last_error()
            got = img.download()
            img.assert_unchanged_except(got, ["B"], f"trsm n={n} ncols={ncols} cells={cells}")
            for c in range(cells):
                _check_solution(img.view("B", c, got), _trsm_ref(n, noise, c, ncols), br.solve_inputs(n, noise, c)[0], br.rhs(n, ncols, c), n, noise,
                                f"trsm/c{ncols}/n{n}/{br.tag(noise)}/seed{c}")


@pytest.mark.parametrize("noise", br.NOISES)
@pytest.mark.parametrize("cells", [1, 3])
def test_trsm_lower_left_src_form(lib, noise, cells):
    """n == 64 with the right-hand side read from `src`: B (NaN on entry) only receives the solution, src is unchanged."""
    n, ncols = 64, 200
    img = _factor_image(cells, n, noise, B=(n, ncols, ncols + 6), src=(n, ncols, ncols + 6))
    for c in range(cells):
        img.view("src", c)[...] = br.rhs(n, ncols, c)
    img.upload()
    rc = lib.gprx_trsm_lower_left(0, img.ptr("L"), n + 6, img.ptr("inv"), img.ptr("B"), ncols + 6, n, ncols, cells, img.cs, img.ptr("src"))
    assert rc == OK, _lib.last_error()
    got = img.download()
    img.assert_unchanged_except(got, ["B"], f"trsm src cells={cells}")
    for c in range(cells):
        _check_solution(img.view("B", c, got), _trsm_ref(n, noise, c, ncols), br.solve_inputs(n, noise, c)[0], br.rhs(n, ncols, c), n, noise,
                        f"trsm/c{ncols}/n{n}/{br.tag(noise)}/seed{c}")


# ---- the inverse ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,noise", SIZES_NOISES)
@pytest.mark.parametrize("cells", [1, 3])
def test_trtri_lower(lib, n, noise, cells):
    """Block counts 1 to 5: a ragged last pair at 192 and 320, none at 128 and 256.  X starts as NaN everywhere.  Afterwards the blocks on
    and below the block diagonal hold L^-1 (zeros above the diagonal inside the diagonal blocks); the block to the right of every even
    diagonal block is ZERO (a 128 x 128 tile of the products reads it as part of a triangular operand, so the routine writes it);
    every other block above the diagonal, the padding and the gaps keep the canary.  T is scratch."""
    nb = n // NB
    for tile in (0, 64, 128):
        fac = _factor_image(cells, n, noise)
        xt = Image(cells, X=(n, n, n + 6), T=(n, n, n + 4))
        fac.upload(), xt.upload()
        rc = lib.gprx_trtri_lower(0, fac.ptr("L"), n + 6, fac.ptr("inv"), xt.ptr("X"), n + 6, xt.ptr("T"), n + 4, n, cells, fac.cs, xt.cs, tile)
        assert rc == OK, _lib.last_error()
        fac.assert_unchanged_except(fac.download(), [], f"trtri n={n} tile={tile}: L / inv_diag")
        got = xt.download()
        xt.assert_unchanged_except(got, ["X", "T"], f"trtri n={n} tile={tile}")
        for c in range(cells):
            x = xt.view("X", c, got)
            low = br.solve_inputs(n, noise, c)[0]
            for bi in range(nb):
                for bj in range(nb):
                    blk = x[NB * bi:NB * bi + NB, NB * bj:NB * bj + NB]
                    if bj > bi and bi % 2 == 0 and bj == bi + 1:
                        assert np.all(blk.view(np.uint64) == 0), f"block {bi, bj} must be zero"
                    elif bj > bi:
                        assert np.all(br.is_canary(blk)), f"block {bi, bj} above the diagonal was written"
                    else:
                        assert not np.any(np.isnan(blk)), f"block {bi, bj} holds NaN (tile {tile})"
                    if bi == bj:
                        assert np.all(np.triu(blk, 1) == 0.0)
            key = _key("trtri", n, noise, c)
            xl = np.tril(x)
            ratio = br.inverse_ratio(low, xl)
            assert ratio <= _limit(key), f"{key} tile {tile}: residual ratio {ratio:.3e}, allowed {_limit(key):.3e}"
            if noise == br.NOISES[0]:
                assert br.rel_err(xl, br.inverse_input(n, noise, c)) < 1e-11


@pytest.mark.parametrize("n", [256, 320])
def test_inverse_gram_from_a_nan_workspace(lib, n):
    """The gradient's sequence on a workspace that starts as NaN: X = L^-1 (trtri_lower), transposed in place, K^-1 = Xt Xt^T on the
    lower tiles with both triangular flags -- at 64 x 64 and at 128 x 128 tiles, whose K ranges reach one block across the diagonal."""
    flags = _lib.GEMM_C_LOWER | _lib.GEMM_A_UPPER | _lib.GEMM_B_LOWER
    for tile in (64, 128):
        fac = _factor_image(1, n, br.NOISES[0])
        xt = Image(1, X=(n, n, n + 6), T=(n, n, n + 4))
        fac.upload(), xt.upload()
        assert lib.gprx_trtri_lower(0, fac.ptr("L"), n + 6, fac.ptr("inv"), xt.ptr("X"), n + 6, xt.ptr("T"), n + 4, n, 1, 0, 0, tile) == OK, _lib.last_error()
        assert lib.gprx_transpose_inplace(0, xt.ptr("X"), n + 6, n, 1, 0) == OK, _lib.last_error()
        out = Image(1, G=(n, n, n + 6))
        out.upload()
        rc = lib.gprx_gemm_batched(0, 0, 1, n, n, n, 1.0, xt.ptr("X"), n + 6, xt.ptr("X"), n + 6, 0.0, out.ptr("G"), n + 6, flags, tile, 1, 0, 0, 0, 1, 0, 0, 0,
                                   None, 0, None, 0)
        assert rc == OK, _lib.last_error()
        fac.dev.free()
        up = np.triu(xt.view("X", 0, xt.download()))  # L^-T as the device left it
        assert not np.any(np.isnan(up))
        got = out.download()
        out.assert_unchanged_except(got, ["G"], f"K^-1 n={n} tile={tile}")
        g = out.view("G", 0, got)
        i, j = np.arange(n)[:, None], np.arange(n)[None, :]
        assert np.all(br.is_canary(g[j // tile > i // tile])), "a tile above the block diagonal was written"
        ref, mag = br.gemm_ref(0, 1, 1.0, up, up, 0.0, None)
        br.assert_gemm(g, ref, mag, n, j <= i, what=f"K^-1 n={n} tile={tile}")


@pytest.mark.parametrize("n", [64, 192])
@pytest.mark.parametrize("cells", [1, 3])
def test_transpose_inplace(lib, n, cells):
    img = Image(cells, X=(n, n, n + 6))
    rng = np.random.default_rng([n, cells])
    for c in range(cells):
        img.view("X", c)[...] = rng.standard_normal((n, n))
    img.upload()
    assert lib.gprx_transpose_inplace(0, img.ptr("X"), n + 6, n, cells, img.cs) == OK, _lib.last_error()
    got = img.download()
    img.assert_unchanged_except(got, ["X"], f"transpose n={n}")
    for c in range(cells):
        assert np.array_equal(img.view("X", c, got), img.view("X", c).T)


def test_alpha_from_inverse(lib):
    """alpha = X^T beta on both sides of ALPHA_CHUNK rows (one partial sum per column, or two); the tiles of X above the diagonal hold NaN."""
    header = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "solve.h")).read()
    chunk = int(re.search(r"constexpr int ALPHA_CHUNK = (\d+);", header).group(1))
    assert min(br.ALPHA_N) < chunk and chunk in br.ALPHA_N and chunk < max(br.ALPHA_N) <= 2 * chunk
    for n in br.ALPHA_N:
        chunks = -(-n // chunk)
        for cells in (1, 3):
            xi = Image(cells, X=(n, n, n + 6))
            vi = Image(cells, beta=(n, 1, 1), alpha=(n, 1, 1))
            i, j = np.arange(n)[:, None] // NB, np.arange(n)[None, :] // NB
            for c in range(cells):
                np.copyto(xi.view("X", c), br.alpha_input(n, c), where=j <= i)
                vi.view("beta", c)[:, 0] = br.vec(n, c)
            xi.upload(), vi.upload()
            # (part: cells * chunks * np doubles, contiguous -- the driver strides it itself)
            part = DeviceBuffer.from_array(br.canary(cells * chunks * n + 8))
            rc = lib.gprx_alpha_from_inverse(0, xi.ptr("X"), n + 6, vi.ptr("beta"), part.ptr, vi.ptr("alpha"), n, cells, xi.cs, vi.cs, vi.cs)
            assert rc == OK, _lib.last_error()
            xi.assert_unchanged_except(xi.download(), [], "alpha_from_inverse: X")
            gp = part.to_array((cells * chunks * n + 8,))
            part.free()
            assert np.all(br.is_canary(gp[cells * chunks * n:])) and not np.any(np.isnan(gp[: cells * chunks * n]))
            got = vi.download()
            vi.assert_unchanged_except(got, ["alpha"], f"alpha_from_inverse n={n} cells={cells}")
            for c in range(cells):
                x, beta = br.alpha_input(n, c).astype(LD), br.vec(n, c).astype(LD)
                ratio = br.sum_ratio(vi.view("alpha", c, got)[:, 0], x.T @ beta, np.abs(x).T @ np.abs(beta))
                key = f"alpha/n{n}/seed{c}"
                assert ratio <= _limit(key), f"{key}: {ratio:.3e}, allowed {_limit(key):.3e}"


# ---- reductions ------------------------------------------------------------------------------------------------------------------------------
# The recorded ratios are those of the bare sums, relative to the sum of the magnitudes of the terms and never below u.  A kernel that
# goes on to form base + scale * sum adds two roundings, each at most u (|base| + |scale| sum |terms|): the same ratio is taken against
# that magnitude, and 8 x (at least u) leaves room for them.
def _reduce(lib, op, m, ldm, w, nrows, ncols, base, scale, acc, partial, rpc, out, cells=1, m_cell=0, w_cell=0, p_cell=0, out_cell=0, tab=None, tab2=None,
            tab_stride=0):
    rc = lib.gprx_reduce_probe(0, op, m, ldm, w, nrows, ncols, base, scale, acc, partial, rpc, out, cells, m_cell, w_cell, p_cell, out_cell, tab, tab2,
                               tab_stride)
    assert rc == OK, _lib.last_error()


@pytest.mark.parametrize("n", br.LOGDET_N)
def test_logdet_quad(lib, n):
    """sum log L[i][i] and sum v[i]^2 for one factor and for three (cell stride, output stride), with and without v."""
    big = max(br.SIZES)
    for cells in (1, 3):
        img = Image(cells, L=(n, n, big + 6), v=(n, 1, 1))
        for c in range(cells):
            img.view("L", c)[...] = br.solve_inputs(big, br.NOISES[0], c)[0][:n, :n]
            img.view("v", c)[:, 0] = br.vec(n, c)
        img.upload()
        for with_v in (True, False):
            ostride = 4
            out = DeviceBuffer.from_array(br.canary(cells * ostride + 2))
            _reduce(lib, _lib.REDUCE_LOGDET_QUAD, img.ptr("L"), big + 6, img.ptr("v") if with_v else None, n, n, 0.0, 0.0, 0, None, 0, out.ptr, cells,
                    img.cs, 0, 0, ostride)
            res = out.to_array((cells * ostride + 2,))
            out.free()
            for c in range(cells):
                d, v = np.diag(br.solve_inputs(big, br.NOISES[0], c)[0])[:n].astype(LD), br.vec(n, c).astype(LD)
                lg = np.log(d)
                r0 = br.sum_ratio(res[c * ostride], np.sum(lg), np.sum(np.abs(lg)))
                assert r0 <= _limit(f"logdet/n{n}/seed{c}"), (n, c, r0)
                if with_v:
                    r1 = br.sum_ratio(res[c * ostride + 1], np.sum(v * v), np.sum(v * v))
                    assert r1 <= _limit(f"quad/n{n}/seed{c}"), (n, c, r1)
                else:
                    assert res[c * ostride + 1] == 0.0
                assert np.all(br.is_canary(res[c * ostride + 2:(c + 1) * ostride]))
            assert np.all(br.is_canary(res[cells * ostride:]))
        img.assert_unchanged_except(img.download(), [], "logdet_quad inputs")


@pytest.mark.parametrize("nrows,ncols", br.COLREDUCE_SHAPES)
def test_colreduce(lib, nrows, ncols):
    """colreduce_partial + colreduce_final: weighted sums and sums of squares down the columns, three cells, chunks of 48 rows (a ragged
    last chunk), accumulate on and off, the base from the argument or from one or two per-cell tables."""
    cells, rpc = 3, br.ROWS_PER_CHUNK
    nchunks = -(-nrows // rpc)
    img = Image(cells, M=(nrows, ncols, ncols + 5), w=(nrows, 1, 1))
    for c in range(cells):
        img.view("M", c)[...] = br.reduce_matrix(nrows, ncols, c)
        img.view("w", c)[:, 0] = br.vec(nrows, c)
    img.upload()
    tab = np.arange(1.0, 1.0 + 7 * cells) * 0.37
    tab2 = -np.arange(1.0, 1.0 + 7 * cells) * 0.11
    dtab, dtab2 = DeviceBuffer.from_array(tab), DeviceBuffer.from_array(tab2)
    prev = np.random.default_rng([nrows, ncols]).standard_normal((cells, ncols))
    for weighted in (True, False):
        for acc, tabs in [(0, 0), (1, 0), (0, 1), (0, 2)]:
            oi = Image(cells, out=(ncols, 1, 1), part=(nchunks * ncols, 1, 1))
            for c in range(cells):
                if acc:
                    oi.view("out", c)[:, 0] = prev[c]
            oi.upload()
            base, scale = 1.25, -0.75
            _reduce(lib, _lib.REDUCE_COL, img.ptr("M"), ncols + 5, img.ptr("w") if weighted else None, nrows, ncols, base, scale, acc, oi.ptr("part"), rpc,
                    oi.ptr("out"), cells, img.cs, img.cs, oi.cs, oi.cs, dtab.ptr if tabs else None, dtab2.ptr if tabs == 2 else None, 7)
            got = oi.download()
            oi.assert_unchanged_except(got, ["out", "part"], f"colreduce {nrows}x{ncols}")
            for c in range(cells):
                m, w = br.reduce_matrix(nrows, ncols, c).astype(LD), br.vec(nrows, c).astype(LD)
                s, mag = (w @ m, np.abs(w) @ np.abs(m)) if weighted else (np.sum(m * m, 0), np.sum(m * m, 0))
                b0 = prev[c].astype(LD) if acc else LD(base if not tabs else tab[7 * c] + (tab2[7 * c] if tabs == 2 else 0.0))
                ratio = br.sum_ratio(oi.view("out", c, got)[:, 0], b0 + LD(scale) * s, np.abs(b0) + abs(scale) * mag)
                key = f"colreduce_{'w' if weighted else 'sq'}/r{nrows}c{ncols}/seed{c}"
                assert ratio <= _limit(key), f"{key} acc={acc} tabs={tabs}: {ratio:.3e}, allowed {_limit(key):.3e}"
    img.assert_unchanged_except(img.download(), [], "colreduce inputs")
    dtab.free(), dtab2.free()


@pytest.mark.parametrize("nrows,ncols", br.ROWREDUCE_SHAPES)
def test_rowreduce(lib, nrows, ncols):
    """One wave per row, 16-byte loads along it: weighted sums and sums of squares, rows that do not fill the last workgroup."""
    img = Image(1, M=(nrows, ncols, ncols + 6), w=(ncols, 1, 1))
    m, w = br.reduce_matrix(nrows, ncols, 0), br.vec(ncols, 0)
    img.view("M")[...] = m
    img.view("w")[:, 0] = w
    img.upload()
    ml, wl = m.astype(LD), w.astype(LD)
    for weighted in (True, False):
        out = DeviceBuffer.from_array(br.canary(nrows + 6))
        base, scale = 0.5, -2.0
        _reduce(lib, _lib.REDUCE_ROW, img.ptr("M"), ncols + 6, img.ptr("w") if weighted else None, nrows, ncols, base, scale, 0, None, 0, out.ptr)
        res = out.to_array((nrows + 6,))
        out.free()
        assert np.all(br.is_canary(res[nrows:]))
        s, mag = (ml @ wl, np.abs(ml) @ np.abs(wl)) if weighted else (np.sum(ml * ml, 1), np.sum(ml * ml, 1))
        ratio = br.sum_ratio(res[:nrows], LD(base) + LD(scale) * s, abs(base) + abs(scale) * mag)
        key = f"rowreduce_{'w' if weighted else 'sq'}/r{nrows}c{ncols}"
        assert ratio <= _limit(key), f"{key}: {ratio:.3e}, allowed {_limit(key):.3e}"
    img.assert_unchanged_except(img.download(), [], "rowreduce inputs")


# ---- what the probes refuse --------------------------------------------------------------------------------------------------------------------
def test_solve_probes_reject_what_the_kernels_cannot_take(lib):
    """By return code only: nothing of this reaches a kernel."""
    buf = DeviceBuffer(8 * 4096)
    p, off = buf.ptr, buf.at(1)
    e = _lib.GPRX_EINVAL
    assert lib.gprx_trsv_lower(0, p, 64, p, p, 96, 0, 1, 0, None) == e  # np % 64
    assert lib.gprx_trsv_lower(0, p, 65, p, p, 64, 0, 1, 0, None) == e  # odd lda
    assert lib.gprx_trsv_lower(0, off, 64, p, p, 64, 0, 1, 0, None) == e  # L not 16-byte aligned
    assert lib.gprx_trsv_lower(0, p, 64, off, p, 64, 0, 1, 0, None) == e
    assert lib.gprx_trsv_lower(0, p, 64, p, p, 64, 0, 3, 4097, None) == e  # odd cell stride
    assert lib.gprx_trsv_lower(0, p, 64, p, p, 64, 0, 1, 0, p) == e  # work without transpose
    assert lib.gprx_trsm_lower_left(0, p, 64, p, p, 41, 64, 40, 1, 0, None) == e  # odd ldb
    assert lib.gprx_trsm_lower_left(0, p, 64, p, off, 40, 64, 40, 1, 0, None) == e
    assert lib.gprx_trsm_lower_left(0, p, 128, p, p, 40, 100, 40, 1, 0, None) == e  # n % 64
    assert lib.gprx_trsm_lower_left(0, p, 128, p, p, 40, 128, 40, 1, 0, p) == e  # src at n != 64
    assert lib.gprx_trtri_lower(0, p, 64, p, p, 65, p, 64, 64, 1, 0, 0, 0) == e  # odd ldx
    assert lib.gprx_trtri_lower(0, p, 64, p, p, 64, off, 64, 64, 1, 0, 0, 0) == e
    assert lib.gprx_trtri_lower(0, p, 64, p, p, 64, p, 64, 64, 2, 4096, 4097, 0) == e  # odd cs_x
    assert lib.gprx_trtri_lower(0, p, 64, p, p, 64, p, 64, 64, 1, 0, 0, 32) == e  # tile
    assert lib.gprx_transpose_inplace(0, p, 65, 64, 1, 0) == e
    assert lib.gprx_transpose_inplace(0, off, 64, 64, 1, 0) == e
    assert lib.gprx_transpose_inplace(0, p, 100, 100, 1, 0) == e
    assert lib.gprx_alpha_from_inverse(0, p, 100, p, p, p, 100, 1, 0, 0, 0) == e
    assert lib.gprx_reduce_probe(0, _lib.REDUCE_ROW, p, 7, None, 4, 6, 0.0, 1.0, 0, None, 0, p, 1, 0, 0, 0, 0, None, None, 0) == e  # odd ldm
    assert lib.gprx_reduce_probe(0, _lib.REDUCE_ROW, p, 8, None, 4, 5, 0.0, 1.0, 0, None, 0, p, 1, 0, 0, 0, 0, None, None, 0) == e  # odd ncols
    assert lib.gprx_reduce_probe(0, _lib.REDUCE_ROW, off, 8, None, 4, 6, 0.0, 1.0, 0, None, 0, p, 1, 0, 0, 0, 0, None, None, 0) == e
    assert lib.gprx_reduce_probe(0, _lib.REDUCE_COL, p, 8, None, 4, 6, 0.0, 1.0, 0, None, 0, p, 1, 0, 0, 0, 0, None, None, 0) == e  # no partial
    assert lib.gprx_reduce_probe(0, 9, p, 8, None, 4, 6, 0.0, 1.0, 0, None, 0, p, 1, 0, 0, 0, 0, None, None, 0) == e
    buf.free()
