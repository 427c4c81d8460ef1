"""The pseudo-surface low-fidelity model: from two boundary hydrographs to a water-surface field and its EOF features.

The reference builds this in ``PseudoSurfaceDataBuilder`` (``gpras/preprocess.py:516-697``) with ``RatingCurve`` (``:454-513``):

1. two stage-discharge rating curves (cubic least-squares splines) give the upstream and downstream water-surface elevation,
2. the centerline interpolater (``:643-667``: per centerline cell the median over time of ``(us_wse - wse) / (us_wse - ds_wse)``)
   spreads them along the stream (``:634-637``),
3. a nearest-centerline-cell lookup spreads that over all cells (``:639-641``),
4. the field is floored by the cell elevations and by the fluvial estimate (``:596-597``, ``:601-606``),
5. and ``PreProcessor.transform`` turns it into the GP's inputs (``production/analysis/pipeline.py:233-238``).

Here the classes take arrays (no geometry, DSS or HDF reading).  The spline *fit* stays on the host (scipy, 11 unknowns);
everything that touches ``T`` or ``n_cells`` numbers runs on the device (``csrc/pseudo.h``), and ``lf_features`` runs steps 1-5
without moving anything of size ``T x n_cells`` over the host link.
"""

from __future__ import annotations

import ctypes as C
from typing import Any

import numpy as np

from . import _lib
from ._device import DeviceHandle, StageTimer, load_npz, save_npz, slab_rows
from ._lib import DeviceBuffer, as_f64, check, ptr

MAX_KNOTS = 64  # interior knots the device evaluation is sized for
FILE_FORMAT = "gpras_amd-pseudo-1"


class RatingCurve:
    """Stage-discharge rating curve for boundary conditions (preprocess.py:454-513)."""

    def __init__(self, q, wse, drop_nonpos: bool = True, qmin: float | None = 10, qmax: float | None = 10e10, n_knots: int = 7, device: int = 0):
        self.device = device
        self._preprocess_data(np.asarray(q), np.asarray(wse), drop_nonpos, qmin, qmax)
        if len(self.q) < max(8, n_knots + 5):
            raise ValueError(f"Not enough points ({len(q)}) for knots={n_knots}. Reduce knots or add data.")
        if n_knots > MAX_KNOTS:
            raise ValueError(f"at most {MAX_KNOTS} knots")
        self.n_knots = n_knots
        self._fit()

    def _preprocess_data(self, q, wse, drop_nonpos: bool = True, qmin: float | None = 0, qmax: float | None = 10e10) -> None:
        mask = np.isfinite(q) & np.isfinite(wse)
        if drop_nonpos:
            mask &= q > 0
        if qmin is not None:
            mask &= q > float(qmin)
        if qmax is not None:
            mask &= q < float(qmax)
        q = q[mask]
        wse = wse[mask]
        order = np.argsort(q)
        self.q = q[order]
        self.wse = wse[order]

    def _fit(self) -> None:
        from scipy.interpolate import LSQUnivariateSpline

        qs_ = np.linspace(0.0, 1.0, self.n_knots + 2)[1:-1]
        interior_knots = np.quantile(self.q, qs_)
        self.spline = LSQUnivariateSpline(self.q, self.wse, t=interior_knots.tolist(), k=3)
        knots, coefficients = spline_arrays(self.spline)
        self.knots, self.coefficients = check_spline(knots, coefficients)

    @classmethod
    def from_arrays(cls, knots, coefficients, device: int = 0) -> "RatingCurve":
        """A fitted curve from its knot vector (boundary knots repeated) and coefficients; ``q``, ``wse`` and ``spline`` are not kept."""
        self = cls.__new__(cls)
        self.device = device
        self.knots, self.coefficients = check_spline(knots, coefficients)
        self.n_knots = len(self.knots) - 8
        self.q = self.wse = self.spline = None
        return self

    @property
    def fit_stats(self) -> dict[str, Any]:
        if self.q is None:
            raise ValueError("a curve restored from arrays does not hold its data")
        resid = self.predict(self.q) - self.wse
        return {"rmse": np.sqrt(np.mean(resid**2)), "mae": np.mean(np.abs(resid))}

    def predict(self, q):
        """Predict WSE from discharge, on the device; the result has the shape of ``q``."""
        q = as_f64(q)
        out = np.empty_like(q)
        lib = _lib.load()
        check(lib.gprx_spline_eval(self.device, ptr(self.knots), len(self.knots), ptr(self.coefficients), ptr(q), q.size, ptr(out)))
        return out


def spline_arrays(spline) -> tuple[np.ndarray, np.ndarray]:
    """FITPACK's full knot vector (boundary knots repeated k + 1 times) and the B-spline coefficients of a cubic scipy spline."""
    t = np.asarray(spline.get_knots(), dtype=np.float64)
    return np.concatenate([[t[0]] * 3, t, [t[-1]] * 3]), np.asarray(spline.get_coeffs(), dtype=np.float64)


def check_spline(knots, coefficients) -> tuple[np.ndarray, np.ndarray]:
    knots, coefficients = as_f64(knots), as_f64(coefficients)
    if knots.ndim != 1 or coefficients.ndim != 1 or len(knots) != len(coefficients) + 4:
        raise ValueError("a cubic spline has four knots more than coefficients")
    if not 8 <= len(knots) <= MAX_KNOTS + 8:
        raise ValueError(f"between 0 and {MAX_KNOTS} interior knots")
    if not np.all(np.isfinite(knots)) or np.any(np.diff(knots) < 0) or not knots[3] < knots[-4]:
        raise ValueError("the knots must be finite, non-decreasing and span an interval")
    return knots, coefficients


def _series(a, name: str) -> np.ndarray:
    """A (T,) series from (T,), (T, 1) or (1, T) input (the reference passes data-frame values of shape (T, 1))."""
    a = as_f64(a)
    if a.ndim == 2 and 1 in a.shape:
        a = a.reshape(-1)
    if a.ndim != 1 or a.size == 0:
        raise ValueError(f"{name} must be a non-empty series")
    return np.ascontiguousarray(a)


class PseudoSurface(DeviceHandle):
    """The numeric state of ``PseudoSurfaceDataBuilder`` on the device."""

    destroy_symbol = "gprx_ps_destroy"

    def __init__(self, cell_elevations, cell_interpolater, us_rating_curve: RatingCurve | None, ds_rating_curve: RatingCurve | None,
                 cl_interpolater=None, device: int = 0, n_centerline: int | None = None):
        super().__init__()
        self.device = device
        self.cell_elevations = as_f64(cell_elevations)
        ci = np.asarray(cell_interpolater)
        if self.cell_elevations.ndim != 1 or self.cell_elevations.size == 0:
            raise ValueError("cell_elevations must be (n_cells,)")
        if ci.shape != self.cell_elevations.shape or not np.issubdtype(ci.dtype, np.integer):
            raise ValueError("cell_interpolater must be an integer array (n_cells,)")
        self.cl_interpolater = None if cl_interpolater is None else as_f64(cl_interpolater)
        if self.cl_interpolater is not None and self.cl_interpolater.ndim != 1:
            raise ValueError("cl_interpolater must be (n_centerline,)")
        if self.cl_interpolater is not None:
            n_centerline = self.cl_interpolater.size
        elif n_centerline is None:
            n_centerline = int(ci.max()) + 1
        self.n_centerline = int(n_centerline)
        if self.n_centerline < 1 or ci.min() < 0 or ci.max() >= self.n_centerline:
            raise ValueError(f"cell_interpolater must hold indices in [0, {self.n_centerline})")
        self.cell_interpolater = np.ascontiguousarray(ci, dtype=np.int32)
        self.n_cells = int(self.cell_elevations.size)
        if (us_rating_curve is None) != (ds_rating_curve is None):
            raise ValueError("give both rating curves or neither")
        self.us_rating_curve, self.ds_rating_curve = us_rating_curve, ds_rating_curve
        self.last_timings_ms: dict[str, float] = {}

    def _create(self):
        us, ds = self.us_rating_curve, self.ds_rating_curve
        check(_lib.load().gprx_ps_create(
            self.device, self.n_cells, ptr(self.cell_elevations), ptr(self.cell_interpolater), self.n_centerline,
            None if self.cl_interpolater is None else ptr(self.cl_interpolater),
            None if us is None else ptr(us.knots), 0 if us is None else len(us.knots), None if us is None else ptr(us.coefficients),
            None if ds is None else ptr(ds.knots), 0 if ds is None else len(ds.knots), None if ds is None else ptr(ds.coefficients),
            C.byref(self._h)))

    # ---- preprocess.py:643-667 ----------------------------------------------------------------------------------------------
    def fit_centerline(self, us_wse, ds_wse, us_q, ds_q, centerline_wse) -> np.ndarray:
        wse = as_f64(centerline_wse)
        if wse.ndim != 2 or wse.shape[1] != self.n_centerline:
            raise ValueError(f"centerline_wse must be (rows, {self.n_centerline})")
        rows = wse.shape[0]
        series = [_series(a, n) for a, n in ((us_wse, "us_wse"), (ds_wse, "ds_wse"), (us_q, "us_q"), (ds_q, "ds_q"))]
        if any(s.shape != (rows,) for s in series):
            raise ValueError("the boundary series must have one entry per row of centerline_wse")
        if not np.any((series[2] > 0) | (series[3] > 0)):
            raise ValueError("no row has a positive upstream or downstream flow")
        w = np.empty(self.n_centerline)
        check(_lib.load().gprx_ps_fit_centerline(self.handle, ptr(series[0]), ptr(series[1]), ptr(series[2]), ptr(series[3]), ptr(wse), rows, ptr(w)))
        self.cl_interpolater = w
        return w

    def _require_weights(self):
        if self.cl_interpolater is None:
            raise ValueError("the centerline interpolater is not fitted")

    def _set_boundaries(self, us_wse, ds_wse) -> int:
        us, ds = _series(us_wse, "us_wse"), _series(ds_wse, "ds_wse")
        if us.shape != ds.shape:
            raise ValueError("us_wse and ds_wse must have the same length")
        check(_lib.load().gprx_ps_set_boundaries(self.handle, ptr(us), ptr(ds), us.size))
        return us.size

    def _rating(self, us_q, ds_q, want: bool = False):
        if self.us_rating_curve is None:
            raise ValueError("the estimator was built without rating curves")
        uq, dq = _series(us_q, "us_q"), _series(ds_q, "ds_q")
        if uq.shape != dq.shape:
            raise ValueError("us_q and ds_q must have the same length")
        us = np.empty(uq.size) if want else None
        ds = np.empty(uq.size) if want else None
        check(_lib.load().gprx_ps_rating(self.handle, ptr(uq), ptr(dq), uq.size, None if us is None else ptr(us), None if ds is None else ptr(ds)))
        return uq.size, us, ds

    # ---- preprocess.py:634-641 ----------------------------------------------------------------------------------------------
    def interpolate_centerline(self, us_wse, ds_wse) -> np.ndarray:
        self._require_weights()
        T = self._set_boundaries(us_wse, ds_wse)
        out = np.empty((T, self.n_centerline))
        check(_lib.load().gprx_ps_centerline(self.handle, ptr(out)))
        return out

    def interpolate_surface(self, cl) -> np.ndarray:
        cl = as_f64(cl)
        if cl.ndim != 2 or cl.shape[1] != self.n_centerline:
            raise ValueError(f"cl must be (T, {self.n_centerline})")
        out = np.empty((cl.shape[0], self.n_cells))
        check(_lib.load().gprx_ps_gather(self.handle, ptr(cl), cl.shape[0], ptr(out)))
        return out

    # ---- preprocess.py:581-599 ----------------------------------------------------------------------------------------------
    def _surface(self, T: int, fluvial) -> np.ndarray:
        out = np.empty((T, self.n_cells))
        if isinstance(fluvial, DeviceBuffer):
            if fluvial.nbytes < out.nbytes:
                raise ValueError(f"the fluvial buffer must hold ({T}, {self.n_cells}) doubles")
            res = DeviceBuffer(out.nbytes, self.device)
            try:
                check(_lib.load().gprx_ps_surface_dev(self.handle, 0, T, fluvial.ptr, self.n_cells, res.ptr, self.n_cells))
                check(_lib.load().gprx_ps_synchronize(self.handle))
                return res.to_array(out.shape)
            finally:
                res.free()
        if fluvial is not None:
            fluvial = as_f64(fluvial)
            if fluvial.shape != out.shape:
                raise ValueError(f"fluvial must be ({T}, {self.n_cells})")
        check(_lib.load().gprx_ps_surface(self.handle, None if fluvial is None else ptr(fluvial), ptr(out)))
        return out

    def surface_from_wse(self, us_wse, ds_wse, fluvial=None) -> np.ndarray:
        """Steps 2-4 for given boundary elevations (``get_lf_plan_data`` after its rating curves, :591-597)."""
        self._require_weights()
        return self._surface(self._set_boundaries(us_wse, ds_wse), fluvial)

    def lf_plan_data(self, us_q, ds_q, fluvial=None) -> np.ndarray:
        """``get_lf_plan_data``: flows -> (T, n_cells) field.  ``fluvial``: host array, ``DeviceBuffer`` or None (no such floor)."""
        self._require_weights()
        T, _, _ = self._rating(us_q, ds_q)
        return self._surface(T, fluvial)

    def lf_features(self, us_q, ds_q, projector, fluvial_x=None, fluvial_gpr=None, fluvial_projector=None) -> np.ndarray:
        """Flows -> (T, k) inputs of the GP; with the three fluvial arguments the fluvial estimate (``get_lf_fluvial_est``, :601-606:
        predict and reverse projection) is computed and consumed on the device.  Only flows (and ``fluvial_x``) go up, ``(T, k)`` comes
        down.  The rows run in the slabs of ``gprx_pca_transform``, so the result equals ``projector.transform(lf_plan_data(...))``."""
        self._require_weights()
        given = [a is not None for a in (fluvial_x, fluvial_gpr, fluvial_projector)]
        if any(given) and not all(given):
            raise ValueError("give fluvial_x, fluvial_gpr and fluvial_projector together")
        if projector.n_cells != self.n_cells or (fluvial_projector is not None and fluvial_projector.n_cells != self.n_cells):
            raise ValueError(f"the projectors must cover the {self.n_cells} cells of the surface")
        lib = _lib.load()
        timer = StageTimer(("rating", "predict", "reverse", "surface", "transform", "download"))
        T, _, _ = self._rating(us_q, ds_q)
        timer.lap("rating")
        k = projector.spatial_mode_count
        cells, cells_p = self.n_cells, -(-self.n_cells // 16) * 16
        slab = slab_rows(projector, T)
        bufs: list[DeviceBuffer] = []
        try:
            modes = None
            if all(given):
                from .pipeline import DevicePipeline

                if np.shape(fluvial_x)[0] != T:
                    raise ValueError("fluvial_x must have one row per flow")
                modes, var, _ = DevicePipeline(fluvial_gpr, fluvial_projector).predict_modes_dev(fluvial_x)
                var.free()
                bufs.append(modes)
                kf = fluvial_projector.spatial_mode_count
                fl = DeviceBuffer(8 * slab * cells, self.device)
                bufs.append(fl)
                timer.lap("predict")
            field = DeviceBuffer(8 * slab * cells_p, self.device)
            z = DeviceBuffer(8 * T * k, self.device)
            bufs += [field, z]
            for t0 in range(0, T, slab):
                nr = min(slab, T - t0)
                if modes is not None:
                    check(lib.gprx_pca_reverse_dev(fluvial_projector.handle, modes.at(t0 * kf), None, nr, fl.ptr, None))
                    check(lib.gprx_pca_synchronize(fluvial_projector.handle))
                    timer.lap("reverse")
                check(lib.gprx_ps_surface_dev(self.handle, t0, nr, None if modes is None else fl.ptr, cells, field.ptr, cells_p))
                check(lib.gprx_ps_synchronize(self.handle))
                timer.lap("surface")
                check(lib.gprx_pca_transform_dev(projector.handle, field.ptr, nr, z.at(t0 * k)))
                check(lib.gprx_pca_synchronize(projector.handle))
                timer.lap("transform")
            out = z.to_array((T, k))
            timer.lap("download")
            # what crossed the host link: the flows and the fluvial model's inputs up, the features down
            timer.link_bytes = 8 * (2 * T + (np.size(fluvial_x) if modes is not None else 0) + T * k)
            self.last_timings_ms = timer.finish()
            return out
        finally:
            for b in bufs:
                b.free()

    # ---- storage ------------------------------------------------------------------------------------------------------------
    def to_dict(self) -> dict[str, np.ndarray]:
        """Plain arrays (what ``to_file`` stores)."""
        d = {"cell_elevations": self.cell_elevations, "cell_interpolater": self.cell_interpolater, "n_centerline": np.array(self.n_centerline)}
        if self.cl_interpolater is not None:
            d["cl_interpolater"] = self.cl_interpolater
        for tag, rc in (("us", self.us_rating_curve), ("ds", self.ds_rating_curve)):
            if rc is not None:
                d[f"{tag}_knots"], d[f"{tag}_coefficients"] = rc.knots, rc.coefficients
        return d

    @classmethod
    def from_dict(cls, d, device: int = 0) -> "PseudoSurface":
        curves = [RatingCurve.from_arrays(d[f"{t}_knots"], d[f"{t}_coefficients"], device) if f"{t}_knots" in d else None for t in ("us", "ds")]
        return cls(d["cell_elevations"], np.asarray(d["cell_interpolater"]), curves[0], curves[1], d["cl_interpolater"] if "cl_interpolater" in d else None,
                   n_centerline=int(d["n_centerline"]), device=device)

    def to_file(self, out_path) -> None:
        """``to_dict`` as an ``.npz`` (``_device.save_npz``); the caller's path is kept as given."""
        save_npz(out_path, FILE_FORMAT, self.to_dict())

    @classmethod
    def from_file(cls, in_path, device: int = 0) -> "PseudoSurface":
        return cls.from_dict(load_npz(in_path, FILE_FORMAT, "pseudo-surface"), device=device)
