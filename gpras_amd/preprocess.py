"""EOF (PCA) preprocessing either side of the GP path on the GPU: the reference's ``PreProcessor``
(``gpras/preprocess.py:866-1162``) and ``HmsPreProcessor`` (:1165-1320) with the same names, arguments, attributes and pickle
format, and ``compute_norths_rule`` (:1323-1353).

``PreProcessor.fit`` runs the fit on the device (``gprx_pcafit_*``: wetness classes, input mean, compaction, both centrings
and the Gram matrix of the single-batch ``IncrementalPCA``, then the EOFs and the training projection); the
eigendecomposition of the small (n_samples x n_samples) Gram matrix runs on the host (``PreProcessor.eigensolver = "host"``, the
default) or on the device (``"device"``: the Gram matrix is not downloaded, only its eigenvalues are), North's rule on the host
(DESIGN.md section 3.12).  ``PreProcessor.sample_route = "auto"`` also fits more samples than wet cells, by the n_wet x n_wet
covariance (``gprx_pcafit_create_auto`` / ``_cov`` / ``_components_cov``).
``EOFProjector`` holds a fitted state and runs the two projections through ``libgprx.so``; ``PreProcessor`` keeps one for
``transform`` / ``reverse_transform``.
Difference from the reference: a ``PreProcessor`` fitted WITHOUT weights keeps ``weights = np.empty(0)``
(preprocess.py:917), so its ``transform`` fails on the broadcast at :1031; here missing or empty weights mean "unweighted".
"""

from __future__ import annotations

import ctypes as C
import pickle
import time
from dataclasses import dataclass
from typing import Any

import numpy as np

from . import _lib
from ._device import DeviceHandle, scoped_handle
from ._lib import as_f64, check, ptr


class EOFProjector(DeviceHandle):
    destroy_symbol = "gprx_pca_destroy"
    create_on_use = False

    def __init__(self, dry_indices, elevations, input_mean, weights, eofs, x_mean, x_std, hydraulic_parameter: str = "wse", device: int = 0):
        if hydraulic_parameter not in ("wse", "depth", "velocity"):
            raise ValueError(f"unknown hydraulic_parameter {hydraulic_parameter!r}")
        self._lib = _lib.load()
        self.device = device
        self.hydraulic_parameter = hydraulic_parameter
        self.dry_indices = np.ascontiguousarray(dry_indices, dtype=bool)
        self.elevations = None if elevations is None or np.size(elevations) == 0 else as_f64(elevations)
        self.input_mean = as_f64(input_mean)
        self.weights = None if weights is None or np.size(weights) == 0 else as_f64(weights)
        self.eofs = as_f64(np.atleast_2d(eofs))
        self.x_mean = as_f64(x_mean)
        self.x_std = as_f64(x_std)
        self.n_cells = int(self.dry_indices.size)
        self.spatial_mode_count = int(self.eofs.shape[0])
        n_wet = int(self.n_cells - self.dry_indices.sum())
        if self.eofs.shape[1] != n_wet or self.input_mean.shape != (n_wet,):
            raise ValueError("eofs must be (k, n_wet) and input_mean (n_wet,) over the cells that are not always dry")
        if self.weights is not None and self.weights.shape != (n_wet,):
            raise ValueError("weights must be (n_wet,)")
        if self.x_mean.shape != (self.spatial_mode_count,) or self.x_std.shape != (self.spatial_mode_count,):
            raise ValueError("x_mean and x_std must be (k,)")
        if self.elevations is not None and self.elevations.shape != (self.n_cells,):
            raise ValueError("elevations must be (n_cells,)")
        super().__init__()

    def _create(self):
        dry_u8 = np.ascontiguousarray(self.dry_indices, dtype=np.uint8)
        check(
            self._lib.gprx_pca_create(
                self.device, self.n_cells, self.spatial_mode_count, ptr(dry_u8), None if self.elevations is None else ptr(self.elevations),
                ptr(self.input_mean), None if self.weights is None else ptr(self.weights), ptr(self.eofs), ptr(self.x_mean), ptr(self.x_std),
                int(self.hydraulic_parameter == "depth"), C.byref(self._h),
            )
        )

    @classmethod
    def from_preprocessor(cls, pre: Any, device: int = 0) -> "EOFProjector":
        """Take the fitted state of a reference ``PreProcessor`` (attribute names of preprocess.py:868-927)."""
        return cls(pre.dry_indices, pre.elevations, pre.input_mean, pre.weights, pre.eofs, pre.x_mean, pre.x_std, pre.hydraulic_parameter, device=device)

    def truncate(self, k: int) -> "EOFProjector":
        """A new projector over the first ``k`` modes (``eofs[:k]``, ``x_mean[:k]``, ``x_std[:k]``): the state a fit with
        ``spatial_mode_count = k`` reaches on the same data (``gpras_amd.sweep``)."""
        if int(k) != k or not 1 <= k <= self.spatial_mode_count:
            raise ValueError(f"k must be an integer in [1, {self.spatial_mode_count}]")
        k = int(k)
        return type(self)(self.dry_indices, self.elevations, self.input_mean, self.weights, self.eofs[:k], self.x_mean[:k], self.x_std[:k],
                          self.hydraulic_parameter, device=self.device)

    def transform(self, x):
        """(samples, cells) -> EOF space (samples, spatial_mode_count)  (preprocess.py:1009-1038)."""
        x = as_f64(x)
        if x.ndim != 2 or x.shape[1] != self.n_cells:
            raise ValueError(f"x must be (samples, {self.n_cells})")
        z = np.empty((x.shape[0], self.spatial_mode_count))
        check(self._lib.gprx_pca_transform(self._h, ptr(x), x.shape[0], ptr(z)))
        return z

    def reverse_transform(self, mean, var=None):
        """EOF space -> (samples, cells); with ``var`` also the propagated variance  (preprocess.py:1052-1085)."""
        mean = as_f64(mean)
        if mean.ndim != 2 or mean.shape[1] != self.spatial_mode_count:
            raise ValueError(f"mean must be (samples, {self.spatial_mode_count})")
        full = np.empty((mean.shape[0], self.n_cells))
        if var is None:
            check(self._lib.gprx_pca_reverse(self._h, ptr(mean), None, mean.shape[0], ptr(full), None))
            return full
        var = as_f64(var)
        if var.shape != mean.shape:
            raise ValueError("var must have the shape of mean")
        var_full = np.empty_like(full)
        check(self._lib.gprx_pca_reverse(self._h, ptr(mean), ptr(var), mean.shape[0], ptr(full), ptr(var_full)))
        return full, var_full


# ---- fitting (preprocess.py:947-1007) -------------------------------------------------------------------------------------
MODES = ("wse", "depth", "velocity")
CLASS_NAMES = np.array(["", "AD", "TF", "AF"], dtype="<U2")  # gprx_pcafit_gram class codes -> _classify_depths strings


@dataclass
class PCAFit:
    """What ``PreProcessor.fit`` keeps of its PCA: the fields of a fitted single-batch ``IncrementalPCA`` that the fit and
    ``compute_norths_rule`` read.  ``components_`` holds the retained rows only (the reference slices ``[:k]`` at :1000)."""

    explained_variance_: np.ndarray
    n_samples_seen_: int
    components_: np.ndarray | None = None


def compute_norths_rule(pca: Any) -> int:
    """Number of significant EOF modes by North's rule (preprocess.py:1323-1353).  Duck-typed: a fitted ``PCA``
    (``n_samples_``), ``IncrementalPCA`` or ``PCAFit`` (``n_samples_seen_``); anything else gives 0, as in the reference."""
    if not hasattr(pca, "explained_variance_"):
        return 0
    if hasattr(pca, "n_samples_"):
        n = pca.n_samples_
    elif hasattr(pca, "n_samples_seen_"):
        n = pca.n_samples_seen_
    else:
        return 0
    eigenvalues = np.asarray(pca.explained_variance_)
    eigenvalues = eigenvalues[eigenvalues > 1]  # Kaiser rule
    if len(eigenvalues) == 0:
        return 0
    d_eigen = np.abs(np.diff(eigenvalues))
    d_error = np.sqrt(2 / n) * eigenvalues[:-1]
    ind = np.argmax(d_eigen <= d_error)
    if ind == 0:
        return int(len(eigenvalues))
    return int(ind)


def check_fit_args(x, elevations, weights, spatial_mode_count, hydraulic_parameter, allow_tall=False):
    """The domain of the device fit, checked before any device work: float64 (cast here), 2 <= n_samples <= n_cells (the
    fit itself also needs n_samples <= n_wet: one IncrementalPCA batch), k <= n_samples - 1 (the rank left after centring).
    ``allow_tall`` (``sample_route = "auto"``) lifts only the n_samples <= n_cells check; the mode count is then bounded by
    min(n_samples - 1, n_cells), and by min(n_samples - 1, n_wet) once the fit knows n_wet.
    Returns the cast (x, elevations, weights)."""
    if hydraulic_parameter not in MODES:
        raise ValueError(f"unknown hydraulic_parameter {hydraulic_parameter!r}")
    x = as_f64(x)
    if x.ndim != 2:
        raise ValueError("x must be (samples, cells)")
    n_s, n_cells = x.shape
    if allow_tall:
        if n_s < 2 or n_cells < 1 or n_s >= 2**31 - 16:
            raise ValueError(f"the fit needs 2 <= samples < 2^31 - 16 and at least one cell; x is {x.shape}")
    elif n_s < 2 or n_s > n_cells:
        raise ValueError(f"the fit needs 2 <= samples <= cells (one IncrementalPCA batch); x is {x.shape}")
    if elevations is None or np.size(elevations) == 0:
        if hydraulic_parameter != "velocity":
            raise ValueError(f"hydraulic_parameter {hydraulic_parameter!r} needs the cell elevations")
        elevations = None
    else:
        elevations = as_f64(elevations)
        if elevations.shape != (n_cells,):
            raise ValueError(f"elevations must be ({n_cells},)")
    if weights is not None:
        weights = as_f64(weights)
        if weights.shape != (n_cells,):
            raise ValueError(f"weights must be ({n_cells},)")
    if spatial_mode_count is not None:
        k_max = min(n_s - 1, n_cells) if allow_tall else n_s - 1
        if int(spatial_mode_count) != spatial_mode_count or not 0 <= spatial_mode_count <= k_max:
            raise ValueError(f"spatial_mode_count must be an integer in [0, {k_max}] (centring leaves rank samples - 1)")
    return x, elevations, weights


class PreProcessor:
    """The reference's ``PreProcessor`` (preprocess.py:866-1162): same constructor, attributes, ``to_dict`` / pickle
    format; ``fit``, ``transform``, ``reverse_transform`` and ``wse_2_depth`` on the device."""

    device = 0
    eigensolver = "host"  # "host": numpy.linalg.eigh of the downloaded Gram matrix; "device": gprx_pcafit_eig (block Jacobi)
    # "gram": n_samples <= n_wet only (one IncrementalPCA batch of at most as many rows as columns), anything else is a ValueError.
    # "auto": that route, same bits, when n_samples <= n_wet; otherwise the covariance route (n_wet x n_wet, n_wet <= 16384), the
    # reference's fit on more rows than columns or on several batches.  ``last_route`` tells which ran.
    sample_route = "gram"
    last_route = None

    def __init__(self, spatial_mode_count: int = 0, input_mean=None, wet_threshold: float = 0.03, elevations=None,
                 hydraulic_parameter: str = "wse", wetness_classes=None, weights=None, eofs=None, eigenvalues=None,
                 n_samples_fit: float = 0, x_mean=None, x_std=None):
        self.spatial_mode_count = spatial_mode_count
        self.input_mean = input_mean if input_mean is not None else np.empty(0, dtype=float)
        self.wet_threshold = wet_threshold
        self.elevations = elevations if elevations is not None else np.empty(0, dtype=float)
        self.hydraulic_parameter = hydraulic_parameter
        self.wetness_classes = wetness_classes if wetness_classes is not None else np.empty(0, dtype=np.str_)
        self.weights = weights if weights is not None else np.empty(0, dtype=float)
        self.eofs = eofs if eofs is not None else np.empty(0, dtype=float)
        self.eigenvalues = eigenvalues if eigenvalues is not None else np.empty(0, dtype=float)
        self.n_samples_fit = n_samples_fit
        self.x_mean = x_mean if x_mean is not None else np.empty(0, dtype=float)
        self.x_std = x_std if x_std is not None else np.empty(0, dtype=float)
        self._proj = None
        self.pca_ = None
        self.last_eig_sweeps = None  # Jacobi sweeps of the last fit with eigensolver = "device" (None: host route, or no fit yet)

    @property
    def dry_indices(self) -> np.ndarray:
        if self.wetness_classes is None:
            raise ValueError("wetness_classes must be numpy array to access dry_indices")
        return np.equal(self.wetness_classes, "AD")

    @property
    def eof(self) -> np.ndarray:
        if self.eofs is None:
            raise ValueError("EOFs have not been computed")
        return self.eofs

    def fit(self, x, elevations, weights=None, spatial_mode_count: int | None = None) -> None:
        """PreProcessor.fit (preprocess.py:947-1007) on the device; North's rule picks the mode count when it is None."""
        if self.eigensolver not in ("host", "device"):
            raise ValueError(f"eigensolver must be 'host' or 'device', not {self.eigensolver!r}")
        if self.sample_route not in ("gram", "auto"):
            raise ValueError(f"sample_route must be 'gram' or 'auto', not {self.sample_route!r}")
        auto = self.sample_route == "auto"
        x, elev, w = check_fit_args(x, elevations, weights, spatial_mode_count, self.hydraulic_parameter, allow_tall=auto)
        n_s, n_cells = x.shape
        on_device = self.eigensolver == "device"
        self.last_eig_sweeps = None
        lib = _lib.load()
        mode = MODES.index(self.hydraulic_parameter)
        route = C.c_int(0)
        args = (self.device, ptr(x), n_s, n_cells, None if elev is None else ptr(elev), None if w is None else ptr(w), mode, float(self.wet_threshold))
        handle = (scoped_handle(lib.gprx_pcafit_create_auto, "gprx_pcafit_destroy", *args, C.byref(route)) if auto
                  else scoped_handle(lib.gprx_pcafit_create, "gprx_pcafit_destroy", *args))
        with handle as h:
            cov = _lib.PCAFIT_ROUTES[route.value] == "covariance"
            g_side = min(n_cells, 16384) if cov else n_s  # the covariance is (n_wet, n_wet), n_wet <= min(n_cells, 16384)
            codes = np.empty(n_cells, dtype=np.uint8)
            mean = np.empty(n_cells)
            n_wet = C.c_int64()
            # the SVD of the twice-centred matrix from the eigendecomposition of its Gram matrix (n_samples x n_samples), or on the
            # covariance route of its covariance (n_wet x n_wet, at most n_cells), largest first
            if on_device:
                lam = np.empty(g_side)
                sweeps = C.c_int()
                check(lib.gprx_pcafit_eig(h, ptr(codes), ptr(mean), ptr(lam), C.byref(n_wet), C.byref(sweeps)))
                lam = np.maximum(lam[: n_wet.value] if cov else lam, 0.0)
            else:
                gram = np.empty((g_side, g_side))
                check((lib.gprx_pcafit_cov if cov else lib.gprx_pcafit_gram)(h, ptr(codes), ptr(mean), ptr(gram), C.byref(n_wet)))
                if cov:  # the library wrote (n_wet, n_wet) contiguously at the start of the block
                    gram = gram.reshape(-1)[: n_wet.value**2].reshape(n_wet.value, n_wet.value)
                lam, u = np.linalg.eigh(gram)
                lam, u = np.maximum(lam[::-1], 0.0), u[:, ::-1]
            n_wet = n_wet.value
            pca = PCAFit(explained_variance_=lam / (n_s - 1), n_samples_seen_=n_s)
            k = compute_norths_rule(pca) if spatial_mode_count is None else int(spatial_mode_count)
            if k > min(n_s - 1, len(lam)) or (k > 0 and not lam[k - 1] > 0.0):
                raise ValueError(f"{k} modes exceed the numerical rank of the centred data ({n_s} samples, {n_wet} wet cells)" if cov else
                                 f"{k} modes exceed the numerical rank of the centred data ({n_s} samples)")
            eofs = np.empty((k, n_wet))
            z = np.empty((n_s, k))
            if on_device:
                check(lib.gprx_pcafit_components_dev(h, k, ptr(eofs), ptr(z)))
            elif cov:
                v_k = np.ascontiguousarray(u[:, :k].T)  # the eigenvectors are the components, up to svd_flip
                check(lib.gprx_pcafit_components_cov(h, k, ptr(v_k), ptr(eofs), ptr(z)))
            else:
                u_k = np.ascontiguousarray(u[:, :k])
                lam_k = np.ascontiguousarray(lam[:k])
                check(lib.gprx_pcafit_components(h, k, ptr(u_k), ptr(lam_k), ptr(eofs), ptr(z)))
            self.last_timings_ms = self._timings(lib, h)
            if cov:  # the fourth stage of this route is the covariance product
                self.last_timings_ms["covariance"], self.last_timings_ms["gram"] = self.last_timings_ms["gram"], 0.0
            if on_device:
                ms = C.c_double()
                check(lib.gprx_pcafit_eig_ms(h, C.byref(ms)))
                self.last_timings_ms["eigensolver"] = ms.value
                self.last_eig_sweeps = sweeps.value
        self.last_route = "covariance" if cov else "gram"
        self.elevations = elevations if elev is None else elev
        self.wetness_classes = CLASS_NAMES[codes]
        self.input_mean = mean[:n_wet].copy()
        if w is not None:
            self.weights = w[~self.dry_indices]
        pca.components_ = eofs
        self.pca_ = pca
        self.spatial_mode_count = k
        self.eofs = eofs
        self.eigenvalues = pca.explained_variance_
        self.n_samples_fit = pca.n_samples_seen_
        self.x_mean = z.mean(axis=0)
        self.x_std = z.std(axis=0)
        self._close_projector()

    @staticmethod
    def _timings(lib, h) -> dict:
        ms = np.zeros(6)
        check(lib.gprx_pcafit_timings(h, ms.ctypes.data_as(C.POINTER(C.c_double))))
        return dict(zip(("upload", "stats", "centring", "gram", "components", "projection"), ms.tolist()))

    # ---- projections through one cached EOFProjector ----------------------------------------------------------------------
    def _projector(self) -> EOFProjector:
        if self._proj is None:
            if self._n_modes() == 0:
                raise ValueError("no spatial modes: fit first (a fit whose North's rule kept 0 modes has nothing to project)")
            self._proj = EOFProjector.from_preprocessor(self, device=self.device)
        return self._proj

    def _n_modes(self) -> int:
        return int(np.shape(self.eofs)[0]) if np.ndim(self.eofs) == 2 else 0

    def _close_projector(self):
        if self._proj is not None:
            self._proj.close()
            self._proj = None

    def transform(self, x):
        """(samples, cells) -> EOF space (samples, spatial_mode_count)  (preprocess.py:1009-1038)."""
        if np.ndim(self.eofs) == 2 and self._n_modes() == 0:
            x = as_f64(x)
            return np.empty((x.shape[0], 0))  # x @ eofs.T of the reference with no modes
        return self._projector().transform(x)

    def reverse_transform(self, mean, var=None):
        """EOF space -> (samples, cells) [, propagated variance]  (preprocess.py:1052-1085)."""
        return self._projector().reverse_transform(mean, var)

    def wse_2_depth(self, x):
        """max(x - elevations, 0) on the device (preprocess.py:1041-1045)."""
        proj = self._projector()
        x = as_f64(x)
        if x.ndim != 2 or x.shape[1] != proj.n_cells:
            raise ValueError(f"x must be (samples, {proj.n_cells})")
        if proj.elevations is None:
            raise ValueError("wse_2_depth needs the cell elevations")
        lib = _lib.load()
        buf = _lib.DeviceBuffer.from_array(x, self.device)
        try:
            check(lib.gprx_pca_to_depth_dev(proj.handle, buf.ptr, x.shape[0], 0))
            check(lib.gprx_pca_synchronize(proj.handle))
            return buf.to_array(x.shape)
        finally:
            buf.free()

    # ---- serialisation (preprocess.py:1135-1162) ----------------------------------------------------------------------
    def to_dict(self) -> dict[str, Any]:
        return {
            "spatial_mode_count": self.spatial_mode_count,
            "wet_threshold": self.wet_threshold,
            "hydraulic_parameter": self.hydraulic_parameter,
            "elevations": self.elevations,
            "wetness_classes": self.wetness_classes,
            "input_mean": self.input_mean,
            "weights": self.weights,
            "eofs": self.eofs,
            "eigenvalues": self.eigenvalues,
            "n_samples_fit": self.n_samples_fit,
            "x_mean": self.x_mean,
            "x_std": self.x_std,
        }

    def to_file(self, out_path) -> None:
        with open(out_path, mode="wb") as f:
            pickle.dump(self.to_dict(), f)

    @classmethod
    def from_file(cls, in_path) -> "PreProcessor":
        with open(in_path, mode="rb") as f:
            d = pickle.load(f)
        return cls(**d)


# ---- HmsPreProcessor (preprocess.py:1165-1320) ------------------------------------------------------------------------------
def _columns(mask, n_features: int, name: str) -> np.ndarray:
    """np.arange(n_features)[mask] (:1231-1232): boolean masks and integer index arrays select as x[:, mask] does."""
    m = np.asarray(mask)
    if m.dtype == bool and m.shape != (n_features,):
        raise ValueError(f"{name} has {m.size} entries, x has {n_features} features")
    try:
        return np.ascontiguousarray(np.arange(n_features)[m], dtype=np.int64).ravel()
    except IndexError as e:
        raise ValueError(f"{name}: {e}") from None


def _device_x(x) -> tuple[np.ndarray, int, int]:
    """x as float64, C or F order kept (DataFrame.values is usually F order): (x, ld, fortran)."""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError("x must be (samples, features)")
    if x.dtype != np.float64 or not (x.flags.c_contiguous or x.flags.f_contiguous):
        x = np.ascontiguousarray(x, dtype=np.float64)
    if x.flags.c_contiguous:
        return x, x.shape[1], 0
    return x, x.shape[0], 1


_API_WEIGHTS: dict = {}


def api_weights(k, window: int) -> np.ndarray:
    """The reference's weights ``[k**i for i in range(window)]`` (:1293), same bits, without the exactly-zero tail: for
    |k| < 1, k**i underflows to 0 and stays there (0.85**i beyond i = 4 580); k == 1 gives ones.  Cached per (k, window)."""
    key = (type(k), k, int(window))
    w = _API_WEIGHTS.get(key)
    if w is None:
        if k == 1:
            w = np.ones(window)
        elif abs(k) < 1:
            vals = []
            for i in range(window):
                v = k**i
                if v == 0:
                    break
                vals.append(v)
            w = np.array(vals, dtype=np.float64)
        else:
            w = np.array([k**i for i in range(window)], dtype=np.float64)
        w.setflags(write=False)
        if len(_API_WEIGHTS) > 64:
            _API_WEIGHTS.clear()
        _API_WEIGHTS[key] = w
    return w


class HmsPreProcessor:
    """The reference's ``HmsPreProcessor`` (preprocess.py:1165-1320): same constructor, attributes and ``to_dict`` / pickle
    format; ``fit``, ``transform`` and ``calc_antecedent_precipitation_index`` run their arithmetic on the device
    (``gprx_hms_*``, ``gprx_api``).  The host keeps the eigendecomposition of the small covariance
    (p x p, or the T x T Gram matrix when T < p) and North's rule."""

    device = 0

    def __init__(self, precip_spatial_mode_count: int = 0, bc_mask=None, precip_mask=None, eofs=None, eigenvalues=None,
                 n_samples_fit: float = 0, x_mean=None, x_std=None, input_mean=None):
        self.precip_spatial_mode_count = precip_spatial_mode_count
        self.bc_mask = bc_mask if bc_mask is not None else np.empty(0, dtype=float)
        self.precip_mask = precip_mask if precip_mask is not None else np.empty(0, dtype=float)
        self.eofs = eofs if eofs is not None else np.empty(0, dtype=float)
        self.eigenvalues = eigenvalues if eigenvalues is not None else np.empty(0, dtype=float)
        self.n_samples_fit = n_samples_fit
        self.x_mean = x_mean if x_mean is not None else np.empty(0, dtype=float)
        self.x_std = x_std if x_std is not None else np.empty(0, dtype=float)
        self.input_mean = input_mean if input_mean is not None else np.empty(0, dtype=float)
        self.pca_ = None
        self.last_timings_ms: dict = {}

    @staticmethod
    def check_fit_args(x, bc_mask, precip_mask, precip_spatial_mode_count=None):
        """The domain, checked before any device work: returns (x, ld, fortran, bc columns, precip columns)."""
        x, ld, fortran = _device_x(x)
        n_s, n_f = x.shape
        bc = _columns(bc_mask, n_f, "bc_mask")
        pc = _columns(precip_mask, n_f, "precip_mask")
        if pc.size == 0:
            raise ValueError("precip_mask selects no column")
        if n_s < 2:
            raise ValueError(f"the fit needs at least 2 samples; x is {x.shape}")
        if min(n_s, pc.size) > 16384:
            raise ValueError("min(samples, precip columns) must be <= 16384 (the host eigendecomposition)")
        k = precip_spatial_mode_count
        if k is not None and (int(k) != k or k < 0):
            raise ValueError("precip_spatial_mode_count must be a non-negative integer")
        return x, ld, fortran, bc, pc

    def fit(self, x, bc_mask, precip_mask, precip_spatial_mode_count: int | None = None) -> None:
        """HmsPreProcessor.fit (preprocess.py:1208-1261) on the device; North's rule picks the mode count when it is None."""
        x, ld, fortran, bc, pc = self.check_fit_args(x, bc_mask, precip_mask, precip_spatial_mode_count)
        n_s, n_f = x.shape
        p = pc.size
        lib = _lib.load()
        with scoped_handle(lib.gprx_hms_create, "gprx_hms_destroy", self.device, ptr(x), n_s, ld, n_f, fortran, ptr(bc), bc.size, ptr(pc), p, None) as h:
            input_mean = np.empty(n_f)
            route = C.c_int()
            n_cov = p if n_s >= p else n_s
            cov = np.empty((n_cov, n_cov))
            check(lib.gprx_hms_cov(h, ptr(input_mean), ptr(cov), C.byref(route)))
            t0 = time.perf_counter()
            lam, v = np.linalg.eigh(cov)
            lam, v = np.maximum(lam[::-1], 0.0), v[:, ::-1]
            eigh_ms = (time.perf_counter() - t0) * 1e3
            pca = PCAFit(explained_variance_=lam / (n_s - 1), n_samples_seen_=np.int64(n_s))
            k = compute_norths_rule(pca) if precip_spatial_mode_count is None else int(precip_spatial_mode_count)
            if route.value == 0:
                # covariance route: the components are the eigenvectors, signed by svd_flip(u_based_decision=False)
                comps = np.ascontiguousarray(v.T)
                piv = comps[np.arange(p), np.argmax(np.abs(comps), axis=1)]
                comps *= np.sign(piv)[:, None]
                eofs = comps[:k]
            else:
                # Gram route: the components are X2^T u / sqrt(lambda), formed on the device
                if k > n_s - 1 or (k > 0 and not lam[k - 1] > 0.0):
                    raise ValueError(f"{k} modes exceed the numerical rank of the centred precip block ({n_s} samples)")
                eofs = np.empty((k, p))
                u_k, lam_k = np.ascontiguousarray(v[:, :k]), np.ascontiguousarray(lam[:k])  # named: ptr() keeps no reference
                check(lib.gprx_hms_components(h, k, ptr(u_k), ptr(lam_k), ptr(eofs)))
            ke = eofs.shape[0]
            e_c = np.ascontiguousarray(eofs)
            w1, w2 = api_weights(0.85, n_s), api_weights(1, n_s)
            x_mean, x_std = np.empty(bc.size + ke + 3), np.empty(bc.size + ke + 3)
            check(lib.gprx_hms_features(h, ke, ptr(e_c), ptr(w1), w1.size, ptr(w2), w2.size, ptr(x_mean), ptr(x_std), 1, None))
            self.last_timings_ms = self._timings(lib, h)
            self.last_timings_ms["host_eigh"] = eigh_ms
        self.input_mean = input_mean
        self.bc_mask = bc_mask
        self.precip_mask = precip_mask
        pca.components_ = eofs
        self.pca_ = pca
        self.precip_spatial_mode_count = k
        self.eofs = eofs
        self.eigenvalues = pca.explained_variance_
        self.n_samples_fit = pca.n_samples_seen_
        self.x_mean = x_mean
        self.x_std = x_std

    @staticmethod
    def _timings(lib, h) -> dict:
        ms = np.zeros(7)
        check(lib.gprx_hms_timings(h, ms.ctypes.data_as(C.POINTER(C.c_double))))
        return dict(zip(("upload", "column_pass", "covariance", "components", "projection", "api", "features"), ms.tolist()))

    def transform(self, x):
        """(samples, features) -> standardised features (samples, n_bc + k + 3)  (preprocess.py:1263-1282)."""
        x, ld, fortran = _device_x(x)
        n_s, n_f = x.shape
        mean = as_f64(self.input_mean)
        if mean.shape != (n_f,):
            raise ValueError(f"x has {n_f} features, input_mean {mean.size}: fit first")
        bc = _columns(self.bc_mask, n_f, "bc_mask")
        pc = _columns(self.precip_mask, n_f, "precip_mask")
        if pc.size == 0:
            raise ValueError("precip_mask selects no column")
        eofs = as_f64(self.eofs)
        if eofs.ndim != 2 or eofs.shape[1] != pc.size:
            raise ValueError(f"eofs must be (k, {pc.size})")
        ke = eofs.shape[0]
        nf = bc.size + ke + 3
        x_mean, x_std = as_f64(self.x_mean), as_f64(self.x_std)
        if x_mean.shape != (nf,) or x_std.shape != (nf,):
            raise ValueError(f"x_mean and x_std must be ({nf},)")
        if n_s < 1:
            raise ValueError("x has no rows")
        lib = _lib.load()
        with scoped_handle(lib.gprx_hms_create, "gprx_hms_destroy", self.device, ptr(x), n_s, ld, n_f, fortran, ptr(bc), bc.size, ptr(pc), pc.size,
                           ptr(mean)) as h:
            w1, w2 = api_weights(0.85, n_s), api_weights(1, n_s)
            out = np.empty((n_s, nf))
            check(lib.gprx_hms_features(h, ke, ptr(eofs), ptr(w1), w1.size, ptr(w2), w2.size, ptr(x_mean), ptr(x_std), 0, ptr(out)))
            self.last_timings_ms = self._timings(lib, h)
        return out

    def calc_antecedent_precipitation_index(self, x, k: float = 0.85, window: int | None = None):
        """np.convolve(x, [k**i for i in range(window)], "full")[:len(x), None] (preprocess.py:1284-1294) on the device."""
        a = np.asarray(x)
        if a.ndim != 1:
            raise ValueError("x must be one-dimensional")
        a = np.ascontiguousarray(a, dtype=np.float64)
        if window is None:
            window = len(a)
        if len(a) == 0 or window <= 0:
            raise ValueError("the series and the window must not be empty")
        w = api_weights(k, window)
        if not np.all(np.isfinite(w)):
            raise ValueError(f"the weights {k}**i overflow within the window")
        out = np.empty((len(a), 1))
        check(_lib.load().gprx_api(self.device, ptr(a), len(a), ptr(w), w.size, int(window), ptr(out)))
        return out

    # ---- serialisation (preprocess.py:1296-1320) --------------------------------------------------------------------------
    def to_dict(self) -> dict[str, Any]:
        return {
            "precip_spatial_mode_count": self.precip_spatial_mode_count,
            "bc_mask": self.bc_mask,
            "precip_mask": self.precip_mask,
            "eofs": self.eofs,
            "eigenvalues": self.eigenvalues,
            "n_samples_fit": self.n_samples_fit,
            "x_mean": self.x_mean,
            "x_std": self.x_std,
            "input_mean": self.input_mean,
        }

    def to_file(self, out_path) -> None:
        with open(out_path, mode="wb") as f:
            pickle.dump(self.to_dict(), f)

    @classmethod
    def from_file(cls, in_path) -> "HmsPreProcessor":
        with open(in_path, mode="rb") as f:
            d = pickle.load(f)
        return cls(**d)
