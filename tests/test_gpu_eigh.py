"""The device eigensolver on the MI355X (``gprx_eigh_*``) against LAPACK on the test matrices of
tests/eig_numpy.py: eigenvalues, residual, orthogonality, eigenvectors where no eigenvalue is repeated, order, sign rule, sweep
counts, determinism, both entry points, reuse of one handle across sizes."""

import ctypes as C

import numpy as np
import pytest

import eig_numpy as en
from gpras_amd import _lib
from gpras_amd._lib import DeviceBuffer, ptr
from gpras_amd.eigh import SymmetricEigensolver, eigh

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
# worst max|V^T V - I| / (sqrt(n) eps) of the numpy restatement over the list (printed by tests/test_eigh.py); the device gets
# 4 x that: its MFMA products sum in another order than numpy's
ORTHO_RATIO = 4.824
N_MAX = max(en.SIZES)


@pytest.fixture(scope="module")
def solver():
    s = SymmetricEigensolver(N_MAX)
    yield s
    s.close()


@pytest.fixture(scope="module")
def solved(solver):
    """Every test matrix through the device, once, on one handle: (g, lam, v, sweeps, off_rel)."""
    out = {}
    for kind, n in en.cases():
        g = en.make_matrix(kind, n)
        keep = g.copy()
        lam, v = solver.eigh(g)
        assert np.array_equal(g, keep), "the input was changed"
        out[kind, n] = (g, lam, v) + solver.info
    return out


@pytest.mark.parametrize("kind, n", en.cases())
def test_against_lapack(solved, kind, n):
    g, lam, v, sweeps, off_rel = solved[kind, n]
    want, u = np.linalg.eigh(g)  # UPLO="L"
    scale = np.max(np.abs(want))
    print(f"{kind} n={n}: sweeps {sweeps}, off_rel {off_rel:.2e}, |dlam|/max {np.max(np.abs(lam - want)) / max(scale, 1e-300):.2e}")
    assert lam.shape == (n,) and v.shape == (n, n)
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(v))
    assert np.max(np.abs(lam - want)) <= 1e-12 * scale
    assert np.all(np.diff(lam) >= 0.0)
    res, norm = en.residual(g, lam, v)
    print(f"  residual / (n eps |G|) = {res / (n * EPS * norm) if norm else 0.0:.3f}")
    assert res <= 4.0 * n * EPS * norm
    ortho = np.max(np.abs(v.T @ v - np.eye(n)))
    print(f"  ortho / (sqrt(n) eps) = {ortho / (np.sqrt(n) * EPS):.3f}")
    assert ortho <= 4.0 * ORTHO_RATIO * np.sqrt(n) * EPS
    # the sign rule: the entry of largest magnitude of every eigenvector, first index on ties, is positive
    piv = v[np.argmax(np.abs(v), axis=0), np.arange(n)]
    assert np.all(piv > 0.0)
    if kind in en.DISTINCT:
        norm2 = max(abs(want[0]), abs(want[-1]))
        for i in range(n):
            gaps = [abs(want[i] - want[j]) for j in (i - 1, i + 1) if 0 <= j < n]
            bound = 1e-12 * norm2 / min(gaps) if gaps else 1e-12
            sign = 1.0 if v[:, i] @ u[:, i] >= 0.0 else -1.0
            err = np.max(np.abs(v[:, i] - sign * u[:, i]))
            assert err <= bound, (i, err, bound)


@pytest.mark.parametrize("n", en.SIZES)
def test_sweep_counts(solved, n):
    for kind in en.KINDS:
        sweeps = solved[kind, n][3]
        if kind == "diagonal" or n == 1:  # diagonal on entry (every 1 x 1 matrix is): the stop rule holds before the first sweep
            assert sweeps == 0, kind
        else:
            assert 1 <= sweeps <= en.MAX_SWEEPS, (kind, sweeps)
    assert solved["near_diagonal", n][3] <= solved["indefinite", n][3]


@pytest.mark.parametrize("n", en.SIZES)
def test_only_the_lower_triangle_is_read(solved, n):
    a, b = solved["indefinite", n], solved["upper_garbage", n]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("kind, n", [("gram", 200), ("indefinite", 257), ("repeated", 129)])
def test_two_calls_identical_bits(solver, solved, kind, n):
    g, lam, v = solved[kind, n][:3]
    lam2, v2 = solver.eigh(g)
    assert np.array_equal(lam, lam2) and np.array_equal(v, v2)


@pytest.mark.parametrize("kind, n", [("gram", 200), ("indefinite", 65), ("indefinite", 520)])
def test_device_entry_equals_host_entry_with_padded_rows(solver, solved, kind, n):
    g, lam, v = solved[kind, n][:3]
    lda, ldv = n + 7, n + 3
    a_pad = np.full((n, lda), 1e300)
    a_pad[:, :n] = g
    a_dev, lam_dev, v_dev = DeviceBuffer.from_array(a_pad), DeviceBuffer(8 * n), DeviceBuffer.from_array(np.full((n, ldv), -7.0))
    try:
        solver.eigh_dev(n, a_dev.ptr, lda, lam_dev.ptr, v_dev.ptr, ldv)
        lam2, v2 = lam_dev.to_array((n,)), v_dev.to_array((n, ldv))
        a_after = a_dev.to_array((n, lda))
    finally:
        for buf in (a_dev, lam_dev, v_dev):
            buf.free()
    assert np.array_equal(lam, lam2) and np.array_equal(v, v2[:, :n])
    assert np.all(v2[:, n:] == -7.0) and np.all(a_after[:, n:] == 1e300), "the padding columns were written"


def test_one_handle_serves_a_small_then_a_large_matrix():
    g65, g520 = en.make_matrix("gram", 65), en.make_matrix("indefinite", 520)
    with SymmetricEigensolver(520) as s:
        lam_a, v_a = s.eigh(g65)
        lam_b, v_b = s.eigh(g520)
        lam_c, v_c = s.eigh(g65)
        with pytest.raises(ValueError):
            s.eigh(np.eye(521))
    with SymmetricEigensolver(65) as s:
        lam_d, v_d = s.eigh(g65)
    assert np.array_equal(lam_a, lam_c) and np.array_equal(v_a, v_c)
    assert np.array_equal(lam_a, lam_d) and np.array_equal(v_a, v_d)
    assert np.max(np.abs(lam_b - np.linalg.eigvalsh(g520))) <= 1e-12 * np.max(np.abs(lam_b))


def test_function_form_and_eigenvalues_only(solved):
    g, lam, v = solved["gram", 129][:3]
    lam2, v2 = eigh(g)
    assert np.array_equal(lam, lam2) and np.array_equal(v, v2)
    with SymmetricEigensolver(129) as s:
        assert np.array_equal(s.eigh(g, eigenvectors=False), lam)
        lam3, v3 = s.eigh(np.asfortranarray(g))  # another memory order of the same matrix
        assert np.array_equal(lam3, lam) and np.array_equal(v3, v)


def test_a_non_finite_matrix_through_the_c_abi_is_no_convergence(solver):
    """The Python layer rejects it; the library itself must end with GPRX_ENOCONV and leave the outputs alone."""
    lib = _lib.load()
    g = en.make_matrix("indefinite", 65)
    g[40, 3] = np.nan
    lam, v = np.full(65, -1.0), np.full((65, 65), -1.0)
    rc = lib.gprx_eigh(solver._h, 65, ptr(g), 65, ptr(lam), ptr(v))
    assert rc == _lib.GPRX_ENOCONV
    assert np.all(lam == -1.0) and np.all(v == -1.0)
    with pytest.raises(np.linalg.LinAlgError):
        _lib.check(rc)
    # the handle stays usable
    lam2, _ = solver.eigh(en.make_matrix("gram", 31))
    assert np.all(np.isfinite(lam2))


def test_argument_checks_of_the_c_abi(solver):
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.gprx_eigh_create(0, 0, C.byref(h)) == _lib.GPRX_EINVAL
    assert lib.gprx_eigh_create(0, 16385, C.byref(h)) == _lib.GPRX_EINVAL
    g, lam = np.eye(4), np.empty(4)
    assert lib.gprx_eigh(solver._h, 4, ptr(g), 3, ptr(lam), None) == _lib.GPRX_EINVAL
    assert lib.gprx_eigh(solver._h, N_MAX + 1, ptr(g), N_MAX + 1, ptr(lam), None) == _lib.GPRX_EINVAL
    assert lib.gprx_eigh(solver._h, 4, ptr(g), 4, ptr(lam), None) == _lib.GPRX_OK
    assert np.array_equal(lam, np.ones(4))
