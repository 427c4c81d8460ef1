"""Mode-count sweep: the field metrics of ``export_metric_summary`` at every EOF truncation of one fit -- the outer loop of the
reference's model selection (``production/analysis/cross_validation.py:96-102``, ``run_spatial_modes``, which runs the
whole pipeline once per count in ``[1, 3, 5, 7, 10, 15, 20, 30, 50]``).

The modes of one ``GPRAS`` are independent models (gpr.py:272-274) and the leading ``k`` EOFs of a fit do not depend on how many are kept
(tests/test_sweep.py pins that), so the prediction at ``k`` modes is the first ``k`` columns of the prediction at ``K`` and the projector
at ``k`` modes is ``EOFProjector.truncate(k)``.  ``ModeCountSweep(projector, counts).evaluate(mean, var, truth, ranges)`` takes the
``(rows, K)`` prediction of the FULL model once and returns, for every count and every event, what ``FieldMetrics`` holds of the field
reconstructed by ``projector.truncate(count)``:

* ``route="fused"``: one device pass per group of counts (``gprx_pca_sweep_dev``, csrc/sweep.h) that reads the truth once per group, walks
  the modes once and never writes a field.  ``t_tol = 0`` only.
* ``route="refield"``: for every count ``truncate(k)`` -> ``gprx_pca_reverse_dev`` -> ``gprx_pca_to_depth_dev`` -> ``gprx_pca_sqrt_dev`` ->
  ``FieldMetrics.from_device`` per event, on the kernels of the per-count chain.  Any ``t_tol`` the metrics support.

Per cell the two routes agree bit for bit; the per-timestep sums over the cells are reduced in different fixed orders (DESIGN.md
section 3.21).  The default route is the one measured faster at the production shape (``DEFAULT_ROUTE``).

What the sweep answers: with the reference's ``hms_upskill`` formulation the GP inputs come from ``HmsPreProcessor`` and do not depend on
``spatial_mode_count`` (pipeline.py:77-87), so the sweep equals ``run_spatial_modes``.  For the other low-fidelity types the inputs are
``hf_reducer.transform(lf)`` and have ``k`` columns themselves: there the sweep answers "how many OUTPUT modes" at fixed inputs.
"""

from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import _lib
from ._device import StageTimer
from ._lib import DeviceBuffer, as_f64, check, ptr
from .diagnostics import check_ranges
from .metrics import FieldMetrics, event_tables, write_metric_db

ROUTES = ("fused", "refield")
DEFAULT_ROUTE = "fused"
DEPTH_MODES = {"velocity": 0, "wse": 1, "depth": 2}
SCALAR_COLUMNS = ("rmse_aoi_toi", "mae_aoi_toi", "conf_aoi_toi", "rmse_aoi_mts", "nse_aoi_mts", "err_aoi_toi", "err_aoi_mts", "fi_aoi_toi", "pod_mts",
                  "rfa_mts", "csi_mts", "f2_mts", "f3_mts")


def check_counts(counts, k_max: int) -> np.ndarray:
    """The counts as an int32 array: between 1 and 64 strictly increasing integers in ``[1, k_max]``."""
    arr = np.asarray(counts)
    if arr.ndim != 1 or arr.size == 0 or arr.size > 64:
        raise ValueError("counts must be a list of between 1 and 64 mode counts")
    if arr.dtype.kind not in "iu":
        raise ValueError("counts must be integers")
    if arr[0] < 1 or arr[-1] > k_max or np.any(np.diff(arr) <= 0):
        raise ValueError(f"counts must be strictly increasing in [1, {k_max}]")
    return np.ascontiguousarray(arr, dtype=np.int32)


class FieldSummary(FieldMetrics):
    """The reductions of one (count, event) with the attribute and method surface of ``FieldMetrics`` (``event_tables`` takes it
    unchanged), filled from downloaded accumulators.  No field is resident: ``peaks`` serves ``None``, the object's own ``x_mts`` and
    its own ``y_mts`` -- including the truth at the prediction's argmax, which the reference's positional ``f2_mts(x, y, x_mts, y_mts)``
    (metrics.py:52-53) reads -- and raises ``ValueError`` for any other timesteps."""

    def __init__(self, rows, cells, v_tol, has_conf, row_sums, cell_sums, y_mts, x_peak, x_mts, matches, row_sum_abs=None, t_tol=0):
        self.rows, self.cells = int(rows), int(cells)
        self.t_tol, self.v_tol = int(t_tol), float(v_tol)
        self.has_conf = bool(has_conf)
        row_sums, cell_sums = np.asarray(row_sums), np.asarray(cell_sums)
        if row_sums.shape != (self.rows, 3) or cell_sums.shape != (6, self.cells):
            raise ValueError("row_sums must be (rows, 3) and cell_sums (6, cells)")
        self.row_sum_e, self.row_sum_e2, self.row_sum_conf = row_sums[:, 0], row_sums[:, 1], row_sums[:, 2]
        self.row_sum_abs = None if row_sum_abs is None else np.asarray(row_sum_abs)
        self.cell_sum_e, self.cell_sum_e2, self.cell_sum_conf, self.cell_sum_abs, self.y_peak, self.x_at_y_mts = cell_sums
        self.x_peak = np.asarray(x_peak)
        self.x_mts, self.y_mts = np.asarray(x_mts, dtype=np.int64), np.asarray(y_mts, dtype=np.int64)
        self.matches = int(matches)

    def close(self):
        pass

    def _own(self, mts, own) -> bool:
        return mts is own or (np.shape(mts) == own.shape and np.array_equal(mts, own))

    def peaks(self, x_mts=None, y_mts=None):
        if x_mts is None or self._own(x_mts, self.x_mts):
            xp = self.x_peak
        elif self._own(x_mts, self.y_mts):
            xp = self.x_at_y_mts
        else:
            raise ValueError("no field is resident: a sweep summary serves the truth only at its own x_mts or y_mts")
        if y_mts is None or self._own(y_mts, self.y_mts):
            yp = self.y_peak
        else:
            raise ValueError("no field is resident: a sweep summary serves the prediction only at its own y_mts")
        return xp, yp

    def mae_aoi_toi(self) -> float:
        total = self.cell_sum_abs.sum() if self.row_sum_abs is None else self.row_sum_abs.sum()
        return float(total / (self.rows * self.cells))


class SweepResult:
    """What ``ModeCountSweep.evaluate`` returns: ``row_sums (n_counts, rows, 3)`` and ``matches (n_counts, n_events)`` on the host, the per-cell
    tables on the device (fused route) until ``summary`` or ``export`` asks for one."""

    def __init__(self, counts, ranges, names, rows, cells, v_tol, t_tol, has_conf, route, row_sums, matches, timings, device=0, cell_dev=None,
                 cell_host=None, row_abs=None):
        self.counts = [int(c) for c in counts]
        self.ranges = [(int(lo), int(hi)) for lo, hi in ranges]
        self.names = list(range(len(self.ranges))) if names is None else list(names)
        if len(self.names) != len(self.ranges):
            raise ValueError("one name per event")
        self.rows, self.cells = int(rows), int(cells)
        self.v_tol, self.t_tol, self.has_conf, self.route, self.device = float(v_tol), int(t_tol), bool(has_conf), route, device
        self.row_sums, self.matches, self.row_abs = np.asarray(row_sums), np.asarray(matches), row_abs
        self._timings = dict(timings)
        self._dev = cell_dev          # fused: (cell_sums, cell_arg, truth_peak, truth_arg) device buffers
        self._host = cell_host or {}  # (j, i) -> (cell_sums (6, cells), y_mts); ("x", i) -> (x_peak, x_mts)

    def close(self):
        if self._dev is not None:
            for b in self._dev:
                b.free()
            self._dev = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stage_timings_ms(self) -> dict:
        return dict(self._timings)

    def _index(self, count, event):
        try:
            j = self.counts.index(int(count))
        except ValueError:
            raise KeyError(f"count {count!r} is not in this sweep: {self.counts}") from None
        if event in self.names:
            return j, self.names.index(event)
        raise KeyError(f"event {event!r} is not in this sweep")

    def _fetch(self, buf, offset_items, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        src = C.c_void_p(buf.ptr.value + out.itemsize * int(offset_items))
        check(_lib.load().gprx_memcpy_d2h(self.device, ptr(out), src, out.nbytes))
        return out

    def cell_block(self, j: int, i: int):
        """``(cell_sums (6, cells), y_mts)`` of count ``j`` and event ``i`` (positions), downloaded once."""
        if (j, i) not in self._host:
            if self._dev is None:
                raise ValueError("the sweep result is closed")
            blk = j * len(self.ranges) + i
            self._host[(j, i)] = (self._fetch(self._dev[0], blk * 6 * self.cells, (6, self.cells), np.float64),
                                  self._fetch(self._dev[1], blk * self.cells, (self.cells,), np.int32))
        return self._host[(j, i)]

    def truth_block(self, i: int):
        """``(x_peak, x_mts)`` of event ``i``."""
        if ("x", i) not in self._host:
            if self._dev is None:
                raise ValueError("the sweep result is closed")
            self._host[("x", i)] = (self._fetch(self._dev[2], i * self.cells, (self.cells,), np.float64),
                                    self._fetch(self._dev[3], i * self.cells, (self.cells,), np.int32))
        return self._host[("x", i)]

    def summary(self, count, event) -> FieldSummary:
        j, i = self._index(count, event)
        lo, hi = self.ranges[i]
        cell_sums, y_mts = self.cell_block(j, i)
        x_peak, x_mts = self.truth_block(i)
        return FieldSummary(hi - lo, self.cells, self.v_tol, self.has_conf, self.row_sums[j, lo:hi], cell_sums, y_mts, x_peak, x_mts, self.matches[j, i],
                            row_sum_abs=None if self.row_abs is None else self.row_abs[j, lo:hi], t_tol=self.t_tol)

    def _tables(self, count, event, tsteps, columns, depth_threshold, hydraulic_parameter):
        return event_tables(self.summary(count, event), event, tsteps, columns, depth_threshold, hydraulic_parameter)

    def scalar_table(self, depth_threshold: float = 0.5, hydraulic_parameter: str = "depth"):
        """One data frame: ``spatial_mode_count``, ``event`` and the reference's scalar columns (metrics.py:39-54), one row per (count, event)."""
        import pandas as pd

        frames = []
        for count in self.counts:
            for i, event in enumerate(self.names):
                lo, hi = self.ranges[i]
                scalar = self._tables(count, event, np.arange(hi - lo), np.arange(self.cells), depth_threshold, hydraulic_parameter)[0]
                scalar.insert(0, "spatial_mode_count", count)
                frames.append(scalar)
        return pd.concat(frames, ignore_index=True)

    def export(self, base_dir, index, columns, depth_threshold: float = 0.5, hydraulic_parameter: str = "depth") -> list[Path]:
        """``base_dir/<i>/performance_metrics.db`` with the reference's three tables for the ``i``-th count, as ``run_cv_serial`` lays the
        options out (cross_validation.py:61-70).  ``index``: the ``(event, timestep)`` index of the truth's data frame; ``columns``: its cell ids."""
        tlevel = np.asarray(index.get_level_values(1))
        if tlevel.shape[0] != self.rows:
            raise ValueError("index must have one entry per row of the truth")
        paths = []
        for pos, count in enumerate(self.counts):
            tabs = [self._tables(count, event, tlevel[lo:hi], columns, depth_threshold, hydraulic_parameter) for event, (lo, hi) in zip(self.names, self.ranges)]
            out_dir = Path(base_dir) / str(pos)
            out_dir.mkdir(parents=True, exist_ok=True)
            write_metric_db([t[0] for t in tabs], [t[1] for t in tabs], [t[2] for t in tabs], out_dir / "performance_metrics.db")
            paths.append(out_dir / "performance_metrics.db")
        return paths


def _device_block(a, shape, device):
    """``a`` as a device block of ``shape``: ``(buffer, owned)``.  A host array is uploaded; anything with a ``.ptr`` is taken as it is."""
    if hasattr(a, "ptr"):
        nbytes = getattr(a, "nbytes", None)
        if nbytes is not None and nbytes < 8 * int(np.prod(shape)):
            raise ValueError(f"a device buffer of {nbytes} bytes cannot hold {shape}")
        return a, False
    arr = as_f64(a)
    if arr.shape != tuple(shape):
        raise ValueError(f"expected an array of shape {tuple(shape)}, got {arr.shape}")
    return DeviceBuffer.from_array(arr, device), True


def _at(buf, offset_elems: int):
    return C.c_void_p(buf.ptr.value + 8 * int(offset_elems))


class ModeCountSweep:
    def __init__(self, projector, counts):
        """``projector``: the ``EOFProjector`` of the fit with ALL ``K`` modes; ``counts``: strictly increasing mode counts in ``[1, K]``."""
        self.projector = projector
        self.counts = check_counts(counts, projector.spatial_mode_count)
        self.device = projector.device

    def evaluate(self, mean, var, truth, ranges, v_tol: float = 0.0, t_tol: int = 0, route: str | None = None, names=None, rows: int | None = None) -> SweepResult:
        """``mean``, ``var`` (or ``None``): the ``(rows, K)`` prediction in EOF-score space; ``truth``: ``(rows, cells)`` in the metrics' space
        (as ``DevicePipeline.truth_depth_dev`` leaves it); host arrays or device buffers (then pass ``rows``); ``ranges``: the events' ``(lo, hi)``
        row ranges, disjoint; ``names``: their labels (default: their positions)."""
        route = DEFAULT_ROUTE if route is None else route
        if route not in ROUTES:
            raise ValueError(f"route must be one of {ROUTES}")
        if t_tol < 0 or t_tol > 8:
            raise ValueError("t_tol must be between 0 and 8")
        if route == "fused" and t_tol != 0:
            raise ValueError("the fused sweep evaluates the fidelity index at t_tol = 0 only: use route='refield'")
        if not v_tol >= 0:
            raise ValueError("v_tol must be non-negative")
        pr = self.projector
        k_full, cells = pr.spatial_mode_count, pr.n_cells
        if rows is None:
            if hasattr(mean, "ptr"):
                raise ValueError("pass rows with device buffers")
            rows = int(np.shape(mean)[0])
        rows = int(rows)
        if rows <= 0:
            raise ValueError("no rows")
        lo_arr, hi_arr = check_ranges(ranges, rows)
        order = np.argsort(lo_arr)
        if np.any(lo_arr[order][1:] < hi_arr[order][:-1]):
            raise ValueError("the events overlap")
        if pr.hydraulic_parameter != "velocity" and pr.elevations is None:
            raise ValueError("wse_2_depth needs the cell elevations (the projector was built without them)")
        timer = StageTimer(("upload", "evaluate", "download"))
        owned = []
        try:
            blocks = []
            for a, shape in ((mean, (rows, k_full)), (var, (rows, k_full)), (truth, (rows, cells))):
                if a is None:
                    blocks.append(None)
                    continue
                buf, own = _device_block(a, shape, self.device)
                if own:
                    owned.append(buf)
                    timer.link_bytes += buf.nbytes
                blocks.append(buf)
            if blocks[0] is None or blocks[2] is None:
                raise ValueError("mean and truth are required")
            timer.lap("upload")
            run = self._fused if route == "fused" else self._refield
            return run(blocks[0], blocks[1], blocks[2], rows, list(zip(lo_arr.tolist(), hi_arr.tolist())), names, float(v_tol), int(t_tol), timer)
        finally:
            for b in owned:
                b.free()

    # ---- one pass (csrc/sweep.h) ------------------------------------------------------------------------------------------------
    def _fused(self, mean, var, truth, rows, ranges, names, v_tol, t_tol, timer) -> SweepResult:
        pr, lib, dev = self.projector, _lib.load(), self.device
        cells, nc, ne = pr.n_cells, len(self.counts), len(ranges)
        lo = np.ascontiguousarray([r[0] for r in ranges], dtype=np.int64)
        hi = np.ascontiguousarray([r[1] for r in ranges], dtype=np.int64)
        bufs = [DeviceBuffer(8 * nc * ne * 6 * cells, dev), DeviceBuffer(4 * nc * ne * cells, dev), DeviceBuffer(8 * ne * cells, dev),
                DeviceBuffer(4 * ne * cells, dev)]
        drow = DeviceBuffer(8 * nc * rows * 3, dev)
        matches = np.zeros((nc, ne), dtype=np.uint64)
        try:
            check(lib.gprx_pca_sweep_dev(pr.handle, mean.ptr, None if var is None else var.ptr, rows, truth.ptr, ne, ptr(lo), ptr(hi), nc, ptr(self.counts),
                                         DEPTH_MODES[pr.hydraulic_parameter], v_tol, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, drow.ptr,
                                         ptr(matches)))
            timer.lap("evaluate")
            row_sums = drow.to_array((nc, rows, 3))
            timer.lap("download")
        except Exception:
            for b in bufs:
                b.free()
            raise
        finally:
            drow.free()
        ms = C.c_double()
        check(lib.gprx_pca_sweep_ms(pr.handle, C.byref(ms)))
        timings = timer.finish()
        timings["device_sweep"] = ms.value
        return SweepResult(self.counts, ranges, names, rows, cells, v_tol, t_tol, var is not None, "fused", row_sums, matches, timings, device=dev,
                           cell_dev=bufs)

    # ---- the per-count chain on the existing kernels --------------------------------------------------------------------------------
    def refield(self, count: int, mean_by_mode, var_by_mode, rows: int, out=None):
        """The fields of ``projector.truncate(count)`` as the metrics see them: ``(pred, conf)`` device buffers of ``(rows, cells)`` (``conf`` None
        without variances), from the ``(K, rows)`` mode-major blocks of the prediction.  ``out``: the two buffers to fill (a sweep reuses one
        pair for all its counts); without it new ones are made, which the caller frees."""
        pr, lib, dev = self.projector, _lib.load(), self.device
        cells = pr.n_cells
        sub = pr.truncate(count)
        made = []
        try:
            ph = sub.handle
            mean_k = DeviceBuffer(8 * rows * count, dev)
            made.append(mean_k)
            check(lib.gprx_pca_transpose_dev(ph, mean_by_mode.ptr, count, rows, mean_k.ptr))  # (count, rows) -> (rows, count)
            var_k = None
            if var_by_mode is not None:
                var_k = DeviceBuffer(8 * rows * count, dev)
                made.append(var_k)
                check(lib.gprx_pca_transpose_dev(ph, var_by_mode.ptr, count, rows, var_k.ptr))
            pred, conf = out if out is not None else (DeviceBuffer(8 * rows * cells, dev), None if var_k is None else DeviceBuffer(8 * rows * cells, dev))
            try:
                check(lib.gprx_pca_reverse_dev(ph, mean_k.ptr, None if var_k is None else var_k.ptr, rows, pred.ptr, None if conf is None else conf.ptr))
                if pr.hydraulic_parameter != "velocity":
                    check(lib.gprx_pca_to_depth_dev(ph, pred.ptr, rows, int(pr.hydraulic_parameter == "depth")))
                if conf is not None:
                    check(lib.gprx_pca_sqrt_dev(ph, conf.ptr, rows * cells))
                check(lib.gprx_pca_synchronize(ph))
            except Exception:
                if out is None:
                    pred.free()
                    if conf is not None:
                        conf.free()
                raise
            return pred, conf
        finally:
            for b in made:
                b.free()
            sub.close()

    def _refield(self, mean, var, truth, rows, ranges, names, v_tol, t_tol, timer) -> SweepResult:
        pr, lib, dev = self.projector, _lib.load(), self.device
        cells, k_full, nc, ne = pr.n_cells, pr.spatial_mode_count, len(self.counts), len(ranges)
        row_sums = np.zeros((nc, rows, 3))
        row_abs = np.zeros((nc, rows))
        matches = np.zeros((nc, ne), dtype=np.uint64)
        host = {}
        made = []
        try:
            # mode-major copies: the first `count` modes of every row are then one contiguous (count, rows) block
            by_mode = []
            for src in (mean, var):
                if src is None:
                    by_mode.append(None)
                    continue
                dst = DeviceBuffer(8 * rows * k_full, dev)
                made.append(dst)
                by_mode.append(dst)
                check(lib.gprx_pca_transpose_dev(pr.handle, src.ptr, rows, k_full, dst.ptr))
            check(lib.gprx_pca_synchronize(pr.handle))
            # one pair of field buffers for all counts
            pred = DeviceBuffer(8 * rows * cells, dev)
            made.append(pred)
            conf = None
            if var is not None:
                conf = DeviceBuffer(8 * rows * cells, dev)
                made.append(conf)
            for j, count in enumerate(self.counts.tolist()):
                self.refield(count, by_mode[0], by_mode[1], rows, out=(pred, conf))
                for i, (lo, hi) in enumerate(ranges):
                    fm = FieldMetrics.from_device(_at(truth, lo * cells), pred.at(lo * cells), None if conf is None else conf.at(lo * cells), hi - lo, cells,
                                                  t_tol=t_tol, v_tol=v_tol, device=dev)
                    row_sums[j, lo:hi, 0], row_sums[j, lo:hi, 1], row_sums[j, lo:hi, 2] = fm.row_sum_e, fm.row_sum_e2, fm.row_sum_conf
                    row_abs[j, lo:hi] = fm.row_sum_abs
                    matches[j, i] = fm.matches
                    x_at_y = fm.peaks(fm.y_mts, None)[0]  # the truth at the prediction's argmax: gathered from the resident field
                    # (the chain's kernels keep no per-cell sum |e|: the mean absolute error comes from its per-timestep sums)
                    host[(j, i)] = (np.stack([fm.cell_sum_e, fm.cell_sum_e2, fm.cell_sum_conf, np.full(cells, np.nan), fm.y_peak, x_at_y]),
                                    fm.y_mts.astype(np.int32))
                    if j == 0:
                        host[("x", i)] = (fm.x_peak, fm.x_mts.astype(np.int32))
            timer.lap("evaluate")
        finally:
            for b in made:
                b.free()
        return SweepResult(self.counts, ranges, names, rows, cells, v_tol, t_tol, var is not None, "refield", row_sums, matches, timer.finish(), device=dev,
                           cell_host=host, row_abs=row_abs)
