"""Eigenvalues and eigenvectors of a real symmetric matrix on the GPU (``gprx_eigh_*``: parallel two-sided block Jacobi in
fp64) with the conventions of ``numpy.linalg.eigh(a, UPLO="L")``: only the lower triangle is read, the
eigenvalues ascend, column ``i`` of ``v`` belongs to ``lam[i]``.  Every eigenvector is turned so that its entry of largest
magnitude (lowest index on ties) is positive, and two calls on the same input give the same bits."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._device import DeviceHandle
from ._lib import check, ptr

N_MAX = 16384


def _check_matrix(a) -> np.ndarray:
    """The input as a C-contiguous float64 copy-or-view; square and finite, or ValueError (before any device work)."""
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError(f"eigh needs a square matrix; got shape {a.shape}")
    if not 1 <= a.shape[0] <= N_MAX:
        raise ValueError(f"eigh needs 1 <= n <= {N_MAX}; got n = {a.shape[0]}")
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError("eigh needs a finite matrix (it holds NaN or inf)")
    return a


class SymmetricEigensolver(DeviceHandle):
    """Owns one ``gprx_eigh`` handle (device buffers for matrices up to ``n_max``) for repeated calls."""

    destroy_symbol = "gprx_eigh_destroy"
    create_on_use = False

    def __init__(self, n_max: int, device: int = 0):
        if int(n_max) != n_max or not 1 <= n_max <= N_MAX:
            raise ValueError(f"n_max must be an integer in [1, {N_MAX}]")
        self.n_max = int(n_max)
        self.device = device
        self._lib = _lib.load()
        super().__init__()

    def _create(self):
        check(self._lib.gprx_eigh_create(self.device, self.n_max, C.byref(self._h)))

    def eigh(self, a, eigenvectors: bool = True):
        """(lam, v) of the symmetric matrix given by the lower triangle of ``a``; ``a`` is not changed.  ``eigenvectors=False``
        returns lam alone.  ``numpy.linalg.LinAlgError`` when the sweep cap is reached."""
        return self._solve(_check_matrix(a), eigenvectors)

    def _solve(self, a: np.ndarray, eigenvectors: bool):
        """``eigh`` on a matrix that ``_check_matrix`` has passed."""
        n = a.shape[0]
        if n > self.n_max:
            raise ValueError(f"the handle holds matrices up to {self.n_max}; got n = {n}")
        lam = np.empty(n)
        v = np.empty((n, n)) if eigenvectors else None
        check(self._lib.gprx_eigh(self._h, n, ptr(a), n, ptr(lam), None if v is None else ptr(v)))
        return (lam, v) if eigenvectors else lam

    def eigh_dev(self, n: int, a_dev, lda: int, lam_dev, v_dev, ldv: int) -> None:
        """The same on device buffers (``_lib.DeviceBuffer.ptr``); the matrix behind ``a_dev`` is overwritten."""
        check(self._lib.gprx_eigh_dev(self._h, int(n), a_dev, int(lda), lam_dev, v_dev, int(ldv)))

    @property
    def info(self) -> tuple[int, float]:
        """(Jacobi sweeps, off(A)_F / ||A||_F at the end) of the last call."""
        sweeps, off = C.c_int(), C.c_double()
        check(self._lib.gprx_eigh_info(self._h, C.byref(sweeps), C.byref(off)))
        return sweeps.value, off.value


def eigh(a, device: int = 0):
    """``numpy.linalg.eigh(a)`` on the GPU: (lam ascending, v with the eigenvectors in its columns)."""
    a = _check_matrix(a)
    with SymmetricEigensolver(a.shape[0], device=device) as solver:
        return solver._solve(a, True)
