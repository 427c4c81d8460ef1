"""The device eigensolver's algorithm, checked on the host through its numpy restatement (tests/eig_numpy.py, DESIGN.md section
3.16): the tournament schedule, eigenvalues against LAPACK, the residual the stop rule leaves, the sweep count; and the argument
checks of ``gpras_amd.eigh`` and ``PreProcessor.eigensolver`` that come before any device work."""

import itertools

import numpy as np
import pytest

import eig_numpy as en

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("m", range(2, 10))
def test_schedule_meets_every_block_pair_once_per_sweep(m):
    rounds = en.schedule(m)
    assert len(rounds) == (m - 1 if m % 2 == 0 else m)
    met = []
    for rnd in rounds:
        assert len(rnd) == m // 2  # odd m: one block sits out
        used = [blk for pair in rnd for blk in pair]
        assert len(used) == len(set(used)), "a block twice in one round"
        assert all(0 <= i < j < m for i, j in rnd)
        met += rnd
    assert sorted(met) == sorted(itertools.combinations(range(m), 2))


def test_block_partition_covers_the_indices_with_a_ragged_last_block():
    for n in en.SIZES:
        blk = en.blocks(n)
        assert len(blk) == -(-n // en.BLOCK)
        assert np.array_equal(np.concatenate(blk), np.arange(n))
        assert all(len(b) == en.BLOCK for b in blk[:-1]) and 1 <= len(blk[-1]) <= en.BLOCK


@pytest.fixture(scope="module")
def solved():
    """Every test matrix through the restatement, once."""
    out = {}
    for kind, n in en.cases():
        g = en.make_matrix(kind, n)
        out[kind, n] = (g,) + en.eigh_jacobi(g)
    return out


@pytest.mark.parametrize("kind, n", en.cases())
def test_restatement_against_lapack(solved, kind, n):
    g, lam, v, sweeps, off_rel = solved[kind, n]
    want = np.linalg.eigvalsh(g)  # UPLO="L"
    scale = np.max(np.abs(want))
    assert np.max(np.abs(lam - want)) <= 1e-12 * scale
    assert np.all(np.diff(lam) >= 0.0)
    res, norm = en.residual(g, lam, v)
    assert res <= 4.0 * n * EPS * norm, res / (n * EPS * norm)
    assert sweeps < en.MAX_SWEEPS
    assert sweeps == 0 if (kind == "diagonal" or n == 1) else sweeps >= 1
    piv = v[np.argmax(np.abs(v), axis=0), np.arange(n)]
    assert np.all(piv > 0.0)


def test_upper_triangle_is_not_read(solved):
    for n in en.SIZES:
        a, b = solved["indefinite", n], solved["upper_garbage", n]
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_near_diagonal_takes_no_more_sweeps_than_dense(solved):
    for n in en.SIZES:
        assert solved["near_diagonal", n][3] <= solved["indefinite", n][3]


def test_worst_orthogonality_ratio_is_printed(solved):
    """max |V^T V - I| / (sqrt(n) eps) over the list: the figure DESIGN.md section 3.16 records and tests/test_gpu_eigh.py
    bounds the device by (ORTHO_RATIO there)."""
    worst = 0.0
    for (kind, n), (g, lam, v, sweeps, off_rel) in solved.items():
        ratio = np.max(np.abs(v.T @ v - np.eye(n))) / (np.sqrt(n) * EPS)
        worst = max(worst, ratio)
    print(f"worst max|V^T V - I| / (sqrt(n) eps) = {worst:.3f}")
    assert np.isfinite(worst)


def test_non_finite_matrix_ends_without_a_result():
    g = en.make_matrix("indefinite", 65)
    g[40, 3] = np.nan
    with pytest.raises(np.linalg.LinAlgError):
        en.eigh_jacobi(g)


# ---- argument checks before any device work ---------------------------------------------------------------------------------
def test_eigh_rejects_non_square_and_non_finite_input(monkeypatch):
    from gpras_amd import _lib, eigh as eigh_mod

    def no_device(*a, **k):
        raise AssertionError("the library was reached before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_device)
    with pytest.raises(ValueError):
        eigh_mod.eigh(np.zeros((3, 4)))
    with pytest.raises(ValueError):
        eigh_mod.eigh(np.zeros(5))
    with pytest.raises(ValueError):
        eigh_mod.eigh(np.zeros((0, 0)))
    bad = np.eye(4)
    bad[2, 1] = np.inf
    with pytest.raises(ValueError):
        eigh_mod.eigh(bad)
    bad[2, 1] = np.nan
    with pytest.raises(ValueError):
        eigh_mod.eigh(bad)
    with pytest.raises(ValueError):
        eigh_mod.SymmetricEigensolver(0)


def test_preprocessor_rejects_an_unknown_eigensolver_before_any_device_work(monkeypatch):
    from gpras_amd import _lib, preprocess

    def no_device(*a, **k):
        raise AssertionError("the library was reached before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_device)
    assert preprocess.PreProcessor.eigensolver == "host"
    pre = preprocess.PreProcessor(hydraulic_parameter="velocity")
    pre.eigensolver = "lapack"
    with pytest.raises(ValueError, match="eigensolver"):
        pre.fit(np.random.default_rng(0).random((4, 20)), None)
    assert "eigensolver" not in pre.to_dict()


def test_new_status_code_maps_to_linalg_error():
    from gpras_amd import _lib

    assert _lib.GPRX_ENOCONV == 7
    for name in ("gprx_eigh_create", "gprx_eigh", "gprx_eigh_dev", "gprx_eigh_info", "gprx_eigh_destroy", "gprx_eigh_last_error",
                 "gprx_pcafit_eig", "gprx_pcafit_components_dev", "gprx_pcafit_eig_ms"):
        assert name in _lib.PROTOTYPES
