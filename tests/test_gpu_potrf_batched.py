"""Every route of the batched Cholesky, element by element, through the probe gprx_potrf_batched: potrf_lower with the fused panel
(route 0) and with the split panel (route 1: the diagonal-only launch of potrf_panel_kernel + potrf_rows_kernel in its four forms),
and potrf_cells (route 2: potrf_cell2_kernel with the right-hand side as tile rows and as a vector).

Every call works on a canary image (blocks_reference.Image): cells a stride apart with gaps between them, lda = np + 6 unless a case
says otherwise, separate parts for A (np + extra rows), inv_diag, the staging area and the vector right-hand side.  Only the lower
triangle and the full diagonal 64 x 64 blocks of A are uploaded -- the blocks strictly above the diagonal blocks keep the canary, a
NaN, so a read of them poisons the result.  After the call the padding columns, the gaps, the rows past np + extra and the blocks
above the diagonal hold the uploaded bits, the diagonal blocks hold exact zeros above the diagonal, inv_diag and the right-hand
sides are written everywhere; the staging area may hold anything.  EVERY cell is checked.

Bounds: golden/blocks_bounds.json records, for each matrix, the componentwise ratios of a float64 numpy restatement of the blocked
algorithm (blocks_reference.emu_potrf) -- |A - L L^T| / (u |L| |L|^T) for the factor, the solve and inverse ratios of
test_gpu_solve_blocks.py for the right-hand sides and the inverse blocks, both against the device's OWN factor -- and a kernel gets
8 x that; test_blocks_reference.py keeps 8 x the factor ratios within Higham's n + 2 (the cell kernel's own factor keys excepted:
see _limit).  On the noise-1e-2 matrices everything is also within 1e-11 relative of the longdouble factorisation.  The integer
matrices of blocks_reference.exact_factor have no rounding error under any schedule: there the results are compared bit for bit at
sizes where a longdouble reference would be too slow.
"""

import ctypes as C
import functools

import numpy as np
import pytest

import blocks_reference as br
from gpras_amd import _lib

pytestmark = pytest.mark.gpu

LD, NB, OK, ENOTPD = br.LD, br.NB, _lib.GPRX_OK, _lib.GPRX_ENOTPD
SLACK = 8.0
STAGE_LD = 129  # potrf.h STAGE_LD: doubles of staging area per matrix column
CELL_VECTOR_MAX_T = 16  # potrf_cell.h CELL2_BETA_MAXT: up to this many block columns one row of 64 right-hand-side rows travels as a vector
ROUTES = {0: "fused panel", 1: "split panel", 2: "cell kernel"}
SIZES_NOISES = [(n, noise) for n in br.SIZES for noise in br.NOISES]
HARD = br.NOISES[1]


def _block_lower(n, total_rows):
    """What a factorisation reads and writes of A: the blocks on and below the block diagonal, and the right-hand-side rows."""
    i, j = np.arange(total_rows)[:, None], np.arange(n)[None, :]
    return (i // NB >= j // NB) | (i >= n)


def factorise(lib, mats, rows=None, *, route, extra=0, y=None, pad=6, outer=0, tile=0, lookahead=0, col_base=0, expect=OK, unchecked=()):
    """One call of the probe on a canary image.  mats: one (n, n) matrix per cell; rows: per cell at least `extra` right-hand-side
    rows of length n; y: per cell the vector right-hand side.  Checks everything the call must leave alone and that every result
    element was written; returns (per cell: L with zeros above the block diagonal, inv (n / 64, 64, 64), the solved rows, y), info."""
    batch, n = len(mats), mats[0].shape[0]
    lda = n + pad
    what = f"route {route} ({ROUTES[route]}) n={n} extra={extra} batch={batch} lda={lda} outer_block={outer} update_tile={tile} lookahead={lookahead}" \
           f"{' yvec' if y is not None else ''}"
    # the cell kernel's vector form: of the 64 rows below the matrix only the first is read and written
    vector_row = route == 2 and extra == NB and n // NB <= CELL_VECTOR_MAX_T
    parts = dict(A=(n + extra, n, lda), inv=(n, NB, NB), stage=(n * STAGE_LD, 1, 1))
    if y is not None:
        parts["y"] = (n, 1, 1)
    img = br.Image(batch, extra_rows=2, **parts)
    mask = _block_lower(n, n + extra)
    if vector_row:
        mask[n + 1:] = False
    for c in range(batch):
        img.set_result("A", np.vstack([mats[c], rows[c][:extra]]) if extra else mats[c], c, where=mask)
        img.mark_result("inv", c)
        if y is not None:
            img.set_result("y", y[c][:, None], c)
    img.upload()
    info = np.full(batch, -77, dtype=np.int32)
    rc = lib.gprx_potrf_batched(0, img.ptr("A"), lda, n, extra, img.ptr("inv"), img.ptr("stage"), img.ptr("y") if y is not None else None, batch, img.cs,
                                route, outer, tile, lookahead, col_base, info.ctypes.data_as(C.POINTER(C.c_int)))
    got = img.download()
    assert rc == expect, f"{what}: status {rc}, {_lib.last_error()}"
    img.assert_unchanged_except(got, ["stage"], what)
    out = []
    for c in range(batch):
        a = img.view("A", c, got)
        res = {"L": np.where(mask[:n], a[:n], 0.0), "inv": img.view("inv", c, got).reshape(n // NB, NB, NB).copy(),
               "rows": a[n:n + (1 if vector_row else extra)].copy(), "y": None if y is None else img.view("y", c, got)[:, 0].copy()}
        if c not in unchecked:
            where = f"{what}, cell {c}"
            assert not np.any(np.isnan(a[mask])), f"{where}: {int(np.sum(np.isnan(a[mask])))} elements of the factor / right-hand-side rows are NaN"
            assert not np.any(np.isnan(res["inv"])), f"{where}: inv_diag holds NaN (block {int(np.argmax(np.isnan(res['inv']).any(axis=(1, 2))))})"
            assert y is None or not np.any(np.isnan(res["y"])), f"{where}: the vector right-hand side holds NaN"
            for b0 in range(0, n, NB):
                above = a[b0:b0 + NB, b0:b0 + NB][np.triu_indices(NB, 1)]
                assert np.all(above == 0.0), f"{where}: diagonal block {b0 // NB} is not zero above the diagonal"
        out.append(res)
    return out, info


# ---- references and limits ---------------------------------------------------------------------------------------------------------------
def _limit(kind, n, noise, seed):
    """8 x the recorded ratio.  potrf_cell (the factor of the cell kernel, whose rows are products with the explicit inverses of the
    diagonal blocks: recorded from the emulation of that form) is capped at Higham's n + 2, which 8 x its ratios would exceed."""
    limit = SLACK * br.bounds()[f"{kind}/n{n}/{br.tag(noise)}/seed{seed}"]
    return min(limit, n + 2.0) if kind == "potrf_cell" else limit


@functools.lru_cache(maxsize=None)
def _beta_ref(n, noise, seed):
    """(POTRF_RHS_ROWS, n) longdouble: the right-hand-side rows solved against the longdouble factor."""
    return br.solve_lower_ld(br.solve_inputs(n, noise, seed)[0], br.potrf_rhs(n, seed).T).T


def _inputs(n, noise, batch):
    return [br.potrf_input(n, noise, c) for c in range(batch)], [br.potrf_rhs(n, c) for c in range(batch)]


def check_cell(res, n, noise, seed, where, vector=False, factor="potrf"):
    """One cell against the recorded limits (and, well conditioned, against the longdouble factorisation).  Every figure is printed;
    returns what lies outside its limit, for assert_none: a test looks at all its cells before it fails."""
    a, low, inv = br.potrf_input(n, noise, seed), res["L"], res["inv"]
    beta = res["y"][None, :] if vector else res["rows"]
    rhs = br.potrf_rhs(n, seed)[:beta.shape[0]]
    fig = [(factor, br.factor_ratio(a, low))]
    if beta.shape[0]:
        fig.append(("potrf_beta", br.solve_ratio(low, beta.T, rhs.T)))
    fig.append(("potrf_inv", max(br.inverse_ratio(low[i:i + NB, i:i + NB], inv[i // NB]) for i in range(0, n, NB))))
    rel = []
    if noise == br.NOISES[0]:
        ref, ref_inv = br.solve_inputs(n, noise, seed)
        rel = [("L", br.rel_err(low, ref)), ("inv_diag", br.rel_err(inv, ref_inv))]
        if beta.shape[0]:
            rel.append(("beta", br.rel_err(beta, _beta_ref(n, noise, seed)[:beta.shape[0]])))
    print(f"{where} seed {seed} {br.tag(noise)}: " + ", ".join(f"{k} {v:.3e} (allowed {_limit(k, n, noise, seed):.3e})" for k, v in fig)
          + "".join(f", {k} rel {v:.2e}" for k, v in rel))
    return [f"{where}: {k} ratio {v:.3e}, allowed {_limit(k, n, noise, seed):.3e}" for k, v in fig if not v <= _limit(k, n, noise, seed)] + \
           [f"{where}: {k} is {v:.3e} from the longdouble reference" for k, v in rel if not v < 1e-11]


def assert_none(failures):
    assert not failures, f"{len(failures)} figures outside their limits:\n" + "\n".join(failures)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_same_cell(a, b, where, keys=("L", "inv", "rows")):
    for k in keys:
        assert same_bits(a[k], b[k]), f"{where}: {k} differs in {int(np.sum(a[k].view(np.uint64) != b[k].view(np.uint64)))} elements"


# ---- rounding bounds -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("n,noise", SIZES_NOISES)
def test_every_route_within_the_recorded_bounds(lib, n, noise, route):
    """1 to 5 block columns (lone panel, fused pair, K = 128 strip, K = 192 main GEMM; a last single column of the cell kernel at odd
    counts), no right-hand side, one tile row of them (the cell kernel's vector form) and two (its tile-row form), one matrix and
    three; once with lda == np, the layout of the sparse path.

    Route 2 has a factor limit of its own (potrf_cell/ keys, capped at n + 2, see _limit).  The cell kernel forms the rows below a
    diagonal block as products with the block's explicit inverse, which is not componentwise backward stable: measured on the
    noise-1e-6 matrices with n >= 128 its factor ratio is 72 .. 121, where 8 x the substitution ratios that routes 0 and 1 are held
    to would allow 61 .. 97 and n + 2 allows 130 .. 322.  Its beta and inverse blocks are held to the same limits as every route's."""
    failures = []
    combos = [(batch, extra, 6) for batch in ((1, 3) if route < 2 else (3,)) for extra in (0, NB, 2 * NB)] + [(3, NB, 0)]
    for batch, extra, pad in combos:
        mats, rows = _inputs(n, noise, batch)
        out, info = factorise(lib, mats, rows, route=route, extra=extra, pad=pad)
        assert np.all(info == 0), (route, n, extra, batch, info)
        for c in range(batch):
            failures += check_cell(out[c], n, noise, c, f"route {route} ({ROUTES[route]}) n={n} extra={extra} batch={batch} lda={n + pad}, cell {c}",
                                   factor="potrf_cell" if route == 2 else "potrf")
    if route == 1:  # potrf_rows_kernel<., YVEC> and the beta_j tail of the diagonal workgroup
        mats, rows = _inputs(n, noise, 3)
        out, info = factorise(lib, mats, route=1, y=[r[0] for r in rows])
        assert np.all(info == 0), info
        for c in range(3):
            failures += check_cell(out[c], n, noise, c, f"route 1 (split panel) n={n} yvec batch=3, cell {c}", vector=True)
    assert_none(failures)


@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("n", [64, 320])
def test_ragged_right_hand_side_rows(lib, n, route):
    """extra = 40: the last workgroup of the panel and rows kernels is partly filled (at n = 64 the only one), and the updates are
    products with a ragged row count."""
    failures = []
    for batch in (1, 3):
        mats, rows = _inputs(n, HARD, batch)
        out, info = factorise(lib, mats, rows, route=route, extra=40)
        assert np.all(info == 0), info
        for c in range(batch):
            failures += check_cell(out[c], n, HARD, c, f"route {route} ({ROUTES[route]}) n={n} extra=40 batch={batch}, cell {c}")
    assert_none(failures)


# ---- bit for bit -----------------------------------------------------------------------------------------------------------------------------
def test_split_panel_equals_fused_panel_bit_for_bit(lib):
    """potrf.h: the rows kernel repeats the fused kernel's arithmetic with L11 read from the staging area."""
    mats, rows = _inputs(320, HARD, 3)
    fused, _ = factorise(lib, mats, rows, route=0, extra=NB)
    split, _ = factorise(lib, mats, rows, route=1, extra=NB)
    for c in range(3):
        assert_same_cell(fused[c], split[c], f"route 0 against route 1, n=320 extra=64 batch=3, cell {c}")


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_a_batched_cell_equals_the_lone_call_and_itself(lib, route):
    """Three runs of three cells give the same bits; cell c of them equals the one-matrix call on the same matrix, with and without
    the look-ahead stream."""
    mats, rows = _inputs(320, HARD, 3)
    first, _ = factorise(lib, mats, rows, route=route, extra=NB)
    for rep in (1, 2):
        again, _ = factorise(lib, mats, rows, route=route, extra=NB)
        for c in range(3):
            assert_same_cell(first[c], again[c], f"route {route} ({ROUTES[route]}) n=320 batch=3, run {rep} against run 0, cell {c}")
    for c in range(3):
        for lookahead in ((0, 1) if route < 2 else (0,)):
            lone, _ = factorise(lib, mats[c:c + 1], rows[c:c + 1], route=route, extra=NB, lookahead=lookahead)
            assert_same_cell(first[c], lone[0], f"route {route} ({ROUTES[route]}) n=320: cell {c} of 3 against the lone call, lookahead={lookahead}")


@pytest.mark.parametrize("route", [0, 1])
def test_fused_k64_update_equals_the_separate_launch(lib, route):
    """n = 128: a 64-column outer block updates the second panel's columns by a K = 64 GEMM launch; the default schedule applies that
    update inside potrf_panel_kernel<true> (route 0) or potrf_rows_kernel<true, .> (route 1) -- operation for operation the same."""
    failures = []
    mats, rows = _inputs(128, HARD, 3)
    fused, _ = factorise(lib, mats, rows, route=route, extra=NB)
    separate, _ = factorise(lib, mats, rows, route=route, extra=NB, outer=64)
    for c in range(3):
        assert_same_cell(fused[c], separate[c], f"route {route} ({ROUTES[route]}) n=128: fused K=64 update against outer_block=64, cell {c}")
        failures += check_cell(separate[c], 128, HARD, c, f"route {route} ({ROUTES[route]}) n=128 outer_block=64, cell {c}")
    assert_none(failures)


def test_vector_right_hand_side_leaves_the_same_factor(lib):
    """The right-hand side as a vector: factor and inverse blocks bit for bit those of the tile-row form, beta within the limit."""
    failures = []
    mats, rows = _inputs(320, HARD, 3)
    tile_form, _ = factorise(lib, mats, rows, route=1, extra=NB)
    vector, info = factorise(lib, mats, route=1, y=[r[0] for r in rows])
    assert np.all(info == 0)
    for c in range(3):
        assert_same_cell(tile_form[c], vector[c], f"route 1 (split panel) n=320: yvec against tile rows, cell {c}", keys=("L", "inv"))
        failures += check_cell(vector[c], 320, HARD, c, f"route 1 (split panel) n=320 yvec, cell {c}", vector=True)
    assert_none(failures)


# ---- the outer-block schedule at a small size ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("outer", [64, 128])
def test_outer_blocks_head_and_tail_updates(lib, route, outer):
    """n = 320 in outer blocks of 64 or 128 columns: HEAD and TAIL updates with both bulk tiles, three cells on one stream and one
    matrix with the TAIL on the look-ahead stream."""
    failures = []
    for tile in (64, 128):
        mats, rows = _inputs(320, HARD, 3)
        out, info = factorise(lib, mats, rows, route=route, extra=NB, outer=outer, tile=tile)
        assert np.all(info == 0), info
        for c in range(3):
            failures += check_cell(out[c], 320, HARD, c, f"route {route} ({ROUTES[route]}) n=320 outer_block={outer} update_tile={tile} batch=3, cell {c}")
        mats, rows = _inputs(320, br.NOISES[0], 1)
        out, info = factorise(lib, mats, rows, route=route, extra=NB, outer=outer, tile=tile, lookahead=1)
        assert info[0] == 0
        failures += check_cell(out[0], 320, br.NOISES[0], 0, f"route {route} ({ROUTES[route]}) n=320 outer_block={outer} update_tile={tile} lookahead=1, cell 0")
    assert_none(failures)


# ---- matrices without rounding error ---------------------------------------------------------------------------------------------------------
def _exact(lib, n, batch, route, what, vector=False, **kw):
    cases = [br.exact_factor(n, c) for c in range(batch)]
    if vector:
        out, info = factorise(lib, [e[0] for e in cases], route=route, y=[e[3][0] for e in cases], **kw)
    else:
        out, info = factorise(lib, [e[0] for e in cases], [e[3] for e in cases], route=route, extra=NB, **kw)
    assert np.all(info == 0), (what, info)
    for c, (_, low, inv, _, z) in enumerate(cases):
        where = f"{what}, cell {c}"
        bad = np.argwhere(out[c]["L"] != low)
        assert bad.size == 0, f"{where}: {len(bad)} elements of L differ from the exact factor, first at {tuple(bad[0])}"
        bad = np.argwhere(out[c]["inv"] != inv)
        assert bad.size == 0, f"{where}: {len(bad)} elements of inv_diag differ from the exact inverses, first (block, row, column) {tuple(bad[0])}"
        beta = out[c]["y"][None, :] if vector else out[c]["rows"]
        bad = np.argwhere(beta != z[:beta.shape[0]])
        assert bad.size == 0, f"{where}: {len(bad)} elements of beta differ from the exact solution, first at {tuple(bad[0])}"


@pytest.mark.parametrize("n", [1024, 1088])
def test_exact_matrices_through_the_cell_kernel(lib, n):
    """16 block columns: the last size of the vector form; 17: the first of the tile-row form, with a last single column."""
    _exact(lib, n, 3, 2, f"route 2 (cell kernel) exact n={n} batch=3")


@pytest.mark.parametrize("route", [0, 1])
def test_exact_matrices_through_head_and_tail_updates(lib, route):
    """Default outer block (1024): n = 1152 is one HEAD update and no TAIL, two cells; n = 2112 a HEAD, then a TAIL on the look-ahead
    stream beside the second block's panels, one matrix."""
    _exact(lib, 1152, 2, route, f"route {route} ({ROUTES[route]}) exact n=1152 batch=2")
    _exact(lib, 2112, 1, route, f"route {route} ({ROUTES[route]}) exact n=2112 lookahead=1", lookahead=1)


def test_exact_matrices_at_the_default_split_threshold(lib):
    """24 cells, the batch size from which potrf_lower chooses the split panel by default; tile rows and vector."""
    _exact(lib, 128, 24, 1, "route 1 (split panel) exact n=128 batch=24")
    _exact(lib, 128, 24, 1, "route 1 (split panel) exact n=128 batch=24 yvec", vector=True)


# ---- a cell that is not positive definite ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_a_failing_pivot_is_reported_for_its_cell_alone(lib, route):
    n, col_base = 192, 1000
    mats, rows = _inputs(n, br.NOISES[0], 3)
    good, info = factorise(lib, mats, rows, route=route, extra=NB, col_base=col_base)
    assert np.all(info == 0)
    bad = mats[1].copy()
    bad[70, 70] = -1.0
    out, info = factorise(lib, [mats[0], bad, mats[2]], rows, route=route, extra=NB, col_base=col_base, expect=ENOTPD, unchecked=(1,))
    assert list(info) == [0, col_base + 71, 0], f"route {route} ({ROUTES[route]}): info {list(info)}"
    for c in (0, 2):
        assert_same_cell(good[c], out[c], f"route {route} ({ROUTES[route]}) n={n}: cell {c} beside a cell that is not positive definite")
