"""The low-fidelity field of the two "Upskill HEC-RAS" builders on the high-fidelity cells, and its EOF features.

The reference resamples a low-fidelity (LF) plan's output block onto the high-fidelity (HF) cells in two ways:

- ``RasUpskillDataBuilder.get_lf_plan_data`` (``gpras/preprocess.py:363-377``): every HF cell takes the value of the LF cell it
  overlaps most (``vals[:, lf_resampler]``), floored by the HF cell elevation; for ``hydraulic_parameter == "velocity"`` the
  magnitude ``sqrt(vx**2 + vy**2)`` without a floor.  ``MeshResampler.nearest``.
- ``RasInterpolaterBuilder.get_lf_plan_data`` (``:433-451``): a Delaunay triangulation of the LF centroids and one
  ``LinearNDInterpolator`` per time step, evaluated at the HF centroids; values below the cell elevation and NaN (outside the hull)
  become the cell elevation.  ``MeshResampler.linear``: the points are located once on the host with the reference's own scipy calls
  (``Delaunay``, ``find_simplex``), the barycentric weights are formed once, and every row is a three-term weighted gather.

Everything of size ``T x n_hf`` is produced on the device (``csrc/resample.h``); ``lf_features`` feeds it to the EOF projection
there, so only ``T x n_lf`` numbers go up and ``T x k`` come down.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._device import DeviceHandle, StageTimer, load_npz, save_npz, slab_rows
from ._lib import DeviceBuffer, as_f64, check, ptr

FILE_FORMAT = "gpras_amd-resample-1"
MAX_SOURCE_CELLS, MAX_OUTPUT_CELLS = 2**28, 2**31 - 1024  # csrc/resample.h: RS_MAX_SRC; the index range of the other handles


def _elevations(cell_elevations, n_out: int):
    if cell_elevations is None:
        return None
    e = as_f64(cell_elevations)
    if e.shape != (n_out,):
        raise ValueError(f"cell_elevations must be ({n_out},)")
    return e


def barycentric_weights(transform, simplex, points) -> np.ndarray:
    """The coordinates scipy's ``LinearNDInterpolator`` forms for ``points`` in their located simplices, in its operations and their
    order: ``d = p - transform[s, 2]``, ``c_i = (0 + T_i0 d_0) + T_i1 d_1``, ``c_2 = (1 - c_0) - c_1``.  Rows of points outside the
    hull (``simplex == -1``) are NaN."""
    inside = simplex >= 0
    s = np.where(inside, simplex, 0)
    t = transform[s]
    d = points - t[:, 2, :]
    c0 = (0.0 + t[:, 0, 0] * d[:, 0]) + t[:, 0, 1] * d[:, 1]
    c1 = (0.0 + t[:, 1, 0] * d[:, 0]) + t[:, 1, 1] * d[:, 1]
    c = np.stack([c0, c1, (1.0 - c0) - c1], axis=1)
    c[~inside] = np.nan
    return c


class MeshResampler(DeviceHandle):
    """Index (and weight) arrays that turn ``(T, n_lf)`` rows of a plan's output block into the ``(T, n_hf)`` field, on the device."""

    destroy_symbol = "gprx_rs_destroy"

    def __init__(self, n_src: int, idx, weights=None, cell_elevations=None, hydraulic_parameter: str = "wse", device: int = 0):
        super().__init__()
        self.device = device
        ix = np.asarray(idx)
        if ix.size == 0 or not np.issubdtype(ix.dtype, np.integer) or ix.ndim not in (1, 2) or (ix.ndim == 2 and ix.shape[1] != 3):
            raise ValueError("idx must be a non-empty integer array (n_hf,) or (n_hf, 3)")
        self.n_vert = 1 if ix.ndim == 1 else 3
        self.n_src, self.n_out = int(n_src), int(ix.shape[0])
        if not 1 <= self.n_src <= MAX_SOURCE_CELLS or self.n_out >= MAX_OUTPUT_CELLS:
            raise ValueError("need 1 <= n_lf <= 2^28 and n_hf < 2^31 - 1024")
        outside = np.all(ix == -1, axis=1) if self.n_vert == 3 else np.zeros(self.n_out, dtype=bool)
        inside = ix[~outside]
        if inside.size and (inside.min() < 0 or inside.max() >= self.n_src):
            raise ValueError(f"idx must hold indices in [0, {self.n_src})" + (" or the outside marker (-1, -1, -1)" if self.n_vert == 3 else ""))
        self.idx = np.ascontiguousarray(ix, dtype=np.int32)
        if (weights is not None) != (self.n_vert == 3):
            raise ValueError("weights go with (n_hf, 3) indices and with nothing else")
        self.weights = None if weights is None else as_f64(weights)
        if self.weights is not None and self.weights.shape != (self.n_out, 3):
            raise ValueError(f"weights must be ({self.n_out}, 3)")
        if hydraulic_parameter not in ("wse", "depth", "velocity"):
            raise ValueError("hydraulic_parameter must be 'wse', 'depth' or 'velocity'")
        if hydraulic_parameter == "velocity" and self.n_vert != 1:
            raise ValueError("the interpolating builder has no velocity form")
        self.hydraulic_parameter = hydraulic_parameter
        # the velocity magnitude has no floor (preprocess.py:374)
        self.cell_elevations = None if hydraulic_parameter == "velocity" else _elevations(cell_elevations, self.n_out)
        self.last_timings_ms: dict[str, float] = {}

    # ---- constructors ---------------------------------------------------------------------------------------------------------------
    @classmethod
    def nearest(cls, lf_resampler, n_lf: int, cell_elevations=None, hydraulic_parameter: str = "wse", device: int = 0) -> "MeshResampler":
        """``RasUpskillDataBuilder`` (:363-377): ``lf_resampler[j]`` is the column of the plan's output block that HF cell j takes.
        Without elevations it is the plain gather of ``get_hf_plan_data`` (:173) for ``hf_resampler``."""
        ix = np.asarray(lf_resampler)
        if ix.ndim != 1:
            raise ValueError("lf_resampler must be (n_hf,)")
        return cls(n_lf, ix, None, cell_elevations, hydraulic_parameter, device)

    @classmethod
    def linear(cls, lf_points, hf_points, cell_elevations=None, lf_cell_ids=None, n_lf: int | None = None, device: int = 0) -> "MeshResampler":
        """``RasInterpolaterBuilder`` (:433-451).  ``lf_points`` (n_aoi, 2): the LF centroids; ``hf_points`` (n_hf, 2): the HF centroids;
        ``lf_cell_ids`` (n_aoi): the columns of the plan's output block the centroids belong to (``lf_geometry_aoi["cell_id"]``, :438;
        default: the block holds exactly the n_aoi cells, in order); ``n_lf``: the columns of that block (default: n_aoi, or
        ``max(lf_cell_ids) + 1``)."""
        from scipy.spatial import Delaunay

        lf, hf = as_f64(lf_points), as_f64(hf_points)
        if lf.ndim != 2 or lf.shape[1] != 2 or hf.ndim != 2 or hf.shape[1] != 2 or hf.shape[0] == 0:
            raise ValueError("lf_points and hf_points must be (n, 2)")
        if lf.shape[0] < 3:
            raise ValueError("a triangulation needs three LF points at least")
        if not (np.all(np.isfinite(lf)) and np.all(np.isfinite(hf))):
            raise ValueError("the points must be finite")
        if lf_cell_ids is None:
            ids = np.arange(lf.shape[0])
        else:
            ids = np.asarray(lf_cell_ids)
            if ids.shape != (lf.shape[0],) or not np.issubdtype(ids.dtype, np.integer) or ids.min() < 0:
                raise ValueError("lf_cell_ids must hold one non-negative integer per LF point")
        if n_lf is None:
            n_lf = int(ids.max()) + 1
        tri = Delaunay(lf)
        simplex = tri.find_simplex(hf)
        inside = simplex >= 0
        degenerate = int(np.isnan(tri.transform[simplex[inside]]).any(axis=(1, 2)).sum())
        if degenerate:
            raise ValueError(f"{degenerate} HF points lie in degenerate simplices of the LF triangulation (no barycentric transform)")
        weights = barycentric_weights(tri.transform, simplex, hf)
        idx = np.where(inside[:, None], ids[tri.simplices[np.where(inside, simplex, 0)]], -1)
        return cls(n_lf, idx, weights, cell_elevations, "wse", device)

    # ---- device state -------------------------------------------------------------------------------------------------------------
    def _create(self):
        check(_lib.load().gprx_rs_create(
            self.device, self.n_src, self.n_out, self.n_vert, ptr(self.idx), None if self.weights is None else ptr(self.weights),
            None if self.cell_elevations is None else ptr(self.cell_elevations), C.byref(self._h)))

    def _sources(self, z, vy):
        z = as_f64(z)
        if z.ndim != 2 or z.shape[1] != self.n_src:
            raise ValueError(f"z must be (T, {self.n_src})")
        if (vy is not None) != (self.hydraulic_parameter == "velocity"):
            raise ValueError("the second velocity component goes with hydraulic_parameter='velocity' and with nothing else")
        if vy is not None:
            vy = as_f64(vy)
            if vy.shape != z.shape:
                raise ValueError("the two velocity components must have the same shape")
        return z, vy

    # ---- preprocess.py:363-377, :433-451 ------------------------------------------------------------------------------------------
    def lf_plan_data(self, z, vy=None) -> np.ndarray:
        """``get_lf_plan_data``: ``z`` (T, n_lf), the plan's output block ("Water Surface", or "Velocity X" with ``vy`` = "Velocity Y")
        -> the (T, n_hf) field."""
        z, vy = self._sources(z, vy)
        out = np.empty((z.shape[0], self.n_out))
        check(_lib.load().gprx_rs_apply(self.handle, ptr(z), None if vy is None else ptr(vy), z.shape[0], ptr(out)))
        return out

    def hf_plan_data(self, z, vy=None) -> np.ndarray:
        """``get_hf_plan_data`` (:163-174): the plain gather ``vals[:, hf_resampler]`` of a resampler built by ``nearest`` without
        elevations."""
        if self.n_vert != 1 or self.cell_elevations is not None:
            raise ValueError("hf_plan_data is the plain gather: build the resampler with MeshResampler.nearest(hf_resampler, n_cells)")
        return self.lf_plan_data(z, vy)

    def lf_features(self, z, projector, vy=None) -> np.ndarray:
        """``z`` (T, n_lf) -> the (T, k) inputs of the GP: resampling and ``PreProcessor.transform`` on the device.  Only the LF rows go
        up and the features come down; the rows run in the slabs of ``gprx_pca_transform``, so the result equals
        ``projector.transform(lf_plan_data(z))`` bit for bit, and device memory is two slabs whatever T is."""
        z, vy = self._sources(z, vy)
        if projector.n_cells != self.n_out:
            raise ValueError(f"the projector must cover the {self.n_out} cells of the resampler")
        lib = _lib.load()
        timer = StageTimer(("upload", "resample", "transform", "download"))
        T, k = z.shape[0], projector.spatial_mode_count
        cells_p = -(-self.n_out // 16) * 16
        slab = slab_rows(projector, T)
        bufs: list[DeviceBuffer] = []
        try:
            srcs = [DeviceBuffer(8 * slab * self.n_src, self.device) for _ in range(1 if vy is None else 2)]
            field = DeviceBuffer(8 * slab * cells_p, self.device)
            feat = DeviceBuffer(8 * max(T * k, 1), self.device)
            bufs += srcs + [field, feat]
            for t0 in range(0, T, slab):
                nr = min(slab, T - t0)
                for buf, a in zip(srcs, (z, vy)):
                    check(lib.gprx_memcpy_h2d(self.device, buf.ptr, ptr(a[t0 : t0 + nr]), 8 * nr * self.n_src))
                timer.lap("upload")
                check(lib.gprx_rs_apply_dev(self.handle, nr, srcs[0].ptr, self.n_src, None if vy is None else srcs[1].ptr, field.ptr, cells_p))
                check(lib.gprx_rs_synchronize(self.handle))
                timer.lap("resample")
                check(lib.gprx_pca_transform_dev(projector.handle, field.ptr, nr, feat.at(t0 * k)))
                check(lib.gprx_pca_synchronize(projector.handle))
                timer.lap("transform")
            out = feat.to_array((T, k))
            timer.lap("download")
            timer.link_bytes = 8 * (T * self.n_src * len(srcs) + T * k)  # the LF rows up, the features down
            self.last_timings_ms = timer.finish()
            return out
        finally:
            for b in bufs:
                b.free()

    # ---- storage --------------------------------------------------------------------------------------------------------------------
    def to_dict(self) -> dict[str, np.ndarray]:
        """Plain arrays (what ``to_file`` stores)."""
        d = {"n_src": np.array(self.n_src), "idx": self.idx, "hydraulic_parameter": np.array(self.hydraulic_parameter)}
        if self.weights is not None:
            d["weights"] = self.weights
        if self.cell_elevations is not None:
            d["cell_elevations"] = self.cell_elevations
        return d

    @classmethod
    def from_dict(cls, d, device: int = 0) -> "MeshResampler":
        return cls(int(d["n_src"]), np.asarray(d["idx"]), d["weights"] if "weights" in d else None,
                   d["cell_elevations"] if "cell_elevations" in d else None, str(d["hydraulic_parameter"]), device)

    def to_file(self, out_path) -> None:
        """``to_dict`` as an ``.npz`` (``_device.save_npz``); the caller's path is kept as given."""
        save_npz(out_path, FILE_FORMAT, self.to_dict())

    @classmethod
    def from_file(cls, in_path, device: int = 0) -> "MeshResampler":
        return cls.from_dict(load_npz(in_path, FILE_FORMAT, "mesh-resampler"), device=device)
