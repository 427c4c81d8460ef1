"""The numerics inside the reference's diagnostic plots (``gen_plots``, ``production/analysis/pipeline.py:90-210``;
``gpras/utils/plotting.py``) on the device, so that no ``(T*, cells)`` field has to come down for them:

* ``performance_cdf`` (plotting.py:201-233): ``np.sort(np.abs(lf - hf).flatten())``, a radix sort of fp64 keys (``csrc/diag.h``),
  equal to ``np.sort`` bit for bit; ``residual_cdf`` brings down an exact subsample of the curve the reference plots;
* ``performance_scatterplot`` (plotting.py:155-198): the line ends ``(ll, ur)`` and the rmse of the label;
* ``map_detection_categories`` (plotting.py:716-859): one category code per event and cell.

Nothing is drawn here: the numbers are what a plotting front end needs.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._device import DeviceHandle
from ._lib import DeviceBuffer, as_f64, check, ptr

DG_TILE = 4096  # csrc/diag.h: DG_TILE, the keys of one workgroup per sort pass
DG_RT = 16  # csrc/diag.h: DG_RT, the row tile of the detection kernel
DG_SUM_CHUNK = 8192  # csrc/diag.h: DG_SUM_CHUNK
# the codes of detection_categories; plotting.py:797-802 (0: the reference's empty string)
CATEGORY_NAMES = ("", "Detected", "Miss", "False Alarm", "Correct Negative")


def sum_depth(n: int) -> int:
    """``D(n)`` of csrc/diag.h (dg_sum_depth): the additions on the longest path of the scatter summary's summation tree."""
    chunks = -(-int(n) // DG_SUM_CHUNK)
    return 32 + 6 + 3 + -(-chunks // 256) + 6 + 3


def cdf_ranks(n: int, n_points: int) -> np.ndarray:
    """The ranks of the sorted residuals that ``residual_cdf`` brings down: ``n_points`` of them evenly over ``[0, n - 1]``, every
    one when ``n_points >= n``."""
    n, n_points = int(n), int(n_points)
    if n < 1 or n_points < 1:
        raise ValueError("need n >= 1 and n_points >= 1")
    if n_points >= n:
        return np.arange(n, dtype=np.int64)
    return np.linspace(0, n - 1, n_points).round().astype(np.int64)


def cdf_pcts(n: int, ranks) -> np.ndarray:
    """``np.linspace(0, 100, n)[ranks]`` (plotting.py:223) without the ``n`` numbers: the same expression numpy evaluates,
    ``start + i * step`` with ``step = 100 / (n - 1)`` and the last point set to 100 exactly."""
    n = int(n)
    ranks = np.asarray(ranks, dtype=np.int64)
    if n == 1:
        return np.zeros(ranks.shape)
    out = ranks.astype(np.float64) * (100.0 / (n - 1)) + 0.0
    out[ranks == n - 1] = 100.0
    return out


def event_ranges(index):
    """``(events, [(lo, hi)])`` of a two-level ``(event, timestep)`` index whose events are contiguous runs of rows, in order of first
    appearance -- the grouping of ``DevicePipeline.export_metric_summary``."""
    level = np.asarray(index.get_level_values(0))
    events, ranges = [], []
    for event in index.unique(level=0):
        pos = np.flatnonzero(level == event)
        lo, n = int(pos[0]), int(pos.size)
        if not np.array_equal(pos, np.arange(lo, lo + n)):
            raise ValueError(f"the rows of event {event!r} are not contiguous in hf_test_data_df (sort the index by event first)")
        events.append(event)
        ranges.append((lo, lo + n))
    return events, ranges


def check_ranges(events, rows: int):
    """A list of ``(lo, hi)`` row ranges as two int64 arrays; every range non-empty and inside ``[0, rows]``."""
    ranges = [(int(lo), int(hi)) for lo, hi in events]
    if not ranges:
        raise ValueError("no events")
    for e, (lo, hi) in enumerate(ranges):
        if not 0 <= lo < hi <= rows:
            raise ValueError(f"event {e}: need 0 <= lo < hi <= rows, got ({lo}, {hi}) with {rows} rows")
    return np.array([r[0] for r in ranges], dtype=np.int64), np.array([r[1] for r in ranges], dtype=np.int64)


class _Held:
    """A device array for the length of a call: an upload that is freed at the end, or the caller's ``DeviceBuffer`` left alone."""

    def __init__(self, a, device, n=None):
        if isinstance(a, DeviceBuffer):
            self.buf, self.owned = a, False
            self.n = a.nbytes // 8 if n is None else int(n)
            self.shape = (self.n,)
            if self.n * 8 > a.nbytes:
                raise ValueError("n exceeds the device buffer")
        else:
            a = as_f64(a)
            self.shape = a.shape
            self.n = a.size
            if self.n == 0:
                raise ValueError("an empty array")
            self.buf, self.owned = DeviceBuffer.from_array(a, device), True

    def free(self):
        if self.owned:
            self.buf.free()


class FieldDiagnostics(DeviceHandle):
    destroy_symbol = "gprx_dg_destroy"

    def __init__(self, device: int = 0):
        super().__init__()
        self.device = device

    def _create(self):
        """The device state: a stream and the sort's workspace, reused across calls."""
        check(_lib.load().gprx_dg_create(self.device, C.byref(self._h)))

    def _pair(self, a, b, n=None):
        held = []
        try:
            for x in (a, b):
                held.append(_Held(x, self.device, n))
        except Exception:
            for x in held:
                x.free()
            raise
        if held[0].n != held[1].n:
            for x in held:
                x.free()
            raise ValueError(f"the two fields must have the same size, got {held[0].n} and {held[1].n}")
        return held

    # ---- plotting.py:201-233 ----------------------------------------------------------------------------------------------------------
    def sorted_abs_residual_dev(self, a, b, n=None) -> tuple[DeviceBuffer, int]:
        """``np.sort(np.abs(a - b).flatten())`` left on the device: ``(buffer, n)``; the caller frees the buffer.  ``a`` and ``b``:
        host arrays of one shape or ``DeviceBuffer`` s of ``n`` doubles (all of the buffer by default); they are not changed."""
        held = self._pair(a, b, n)
        try:
            out = DeviceBuffer(8 * held[0].n, self.device)
            try:
                check(_lib.load().gprx_dg_sort_abs_residual_dev(self.handle, held[0].buf.ptr, held[1].buf.ptr, held[0].n, out.ptr))
            except Exception:
                out.free()
                raise
            return out, held[0].n
        finally:
            for x in held:
                x.free()

    def sorted_abs_residual(self, a, b, n=None) -> np.ndarray:
        """``np.sort(np.abs(a - b).flatten())`` (plotting.py:221-222), all ``n`` values on the host."""
        out, n = self.sorted_abs_residual_dev(a, b, n)
        try:
            return out.to_array((n,))
        finally:
            out.free()

    def sort_u64(self, keys) -> np.ndarray:
        """``np.sort`` of unsigned 64-bit keys (the raw sort under ``sorted_abs_residual``)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
        src = DeviceBuffer(max(keys.nbytes, 8), self.device)
        dst = DeviceBuffer(max(keys.nbytes, 8), self.device)
        try:
            lib = _lib.load()
            if keys.size:
                check(lib.gprx_memcpy_h2d(self.device, src.ptr, ptr(keys), keys.nbytes))
            check(lib.gprx_dg_sort_u64_dev(self.handle, src.ptr, keys.size, dst.ptr))
            out = np.empty(keys.size, dtype=np.uint64)
            check(lib.gprx_memcpy_d2h(self.device, ptr(out), dst.ptr, out.nbytes))
            return out
        finally:
            src.free()
            dst.free()

    def last_sort_info(self) -> dict:
        """Of the last sort: which of the eight passes ran (byte 0 first) and the device milliseconds of its two stages."""
        mask, ms = C.c_int(), np.zeros(2)
        check(_lib.load().gprx_dg_sort_info(self.handle, C.byref(mask), ms.ctypes.data_as(C.POINTER(C.c_double))))
        executed = [p for p in range(8) if mask.value >> p & 1]
        return {"executed_passes": executed, "skipped_passes": 8 - len(executed), "histogram_ms": float(ms[0]), "passes_ms": float(ms[1])}

    def gather(self, sorted_dev: DeviceBuffer, n: int, ranks) -> np.ndarray:
        """``sorted[ranks]`` of a device array of ``n`` doubles."""
        ranks = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
        out = np.empty(ranks.size)
        check(_lib.load().gprx_dg_gather_dev(self.handle, sorted_dev.ptr, n, ptr(ranks), ranks.size, ptr(out)))
        return out

    def residual_cdf(self, lf, hf, upskill, n_points: int = 2048, n=None):
        """The two curves of ``performance_cdf`` (plotting.py:221-227) at ``n_points`` ranks spread evenly over the sorted residuals:
        ``(values_lf, values_upskill, pcts)`` with ``values = np.sort(np.abs(x - hf).flatten())[ranks]`` and ``pcts =
        np.linspace(0, 100, n)[ranks]`` -- points of the reference's own curve, not an approximation of it.  ``lf`` may be None
        (``values_lf`` is then None).  ``n_points >= n`` gives the whole curve.  Only ``n_points`` doubles per curve come down."""
        hf_held = _Held(hf, self.device, n)
        try:
            ranks = cdf_ranks(hf_held.n, n_points)
            values = []
            for field in (lf, upskill):
                if field is None:
                    values.append(None)
                    continue
                srt, m = self.sorted_abs_residual_dev(field, hf_held.buf, hf_held.n)
                try:
                    values.append(self.gather(srt, m, ranks))
                finally:
                    srt.free()
            return values[0], values[1], cdf_pcts(hf_held.n, ranks)
        finally:
            hf_held.free()

    # ---- plotting.py:155-198 ----------------------------------------------------------------------------------------------------------
    def scatter_summary(self, p, hf, n=None) -> dict:
        """One panel of ``performance_scatterplot``: ``ll``, ``ur`` (the ends of the dashed line, plotting.py:183-184) and ``rmse``
        (plotting.py:185), with the sum of squares ``sum_sq`` it comes from (summed in the fixed order of csrc/diag.h) and ``n``."""
        held = self._pair(p, hf, n)
        try:
            out = np.empty(4)
            check(_lib.load().gprx_dg_scatter_summary_dev(self.handle, held[0].buf.ptr, held[1].buf.ptr, held[0].n, ptr(out)))
        finally:
            for x in held:
                x.free()
        return {"ll": float(out[0]), "ur": float(out[1]), "rmse": float((out[2] / out[3]) ** 0.5), "sum_sq": float(out[2]), "n": int(out[3])}

    # ---- plotting.py:716-859 ----------------------------------------------------------------------------------------------------------
    def detection_categories_dev(self, truth: DeviceBuffer, pred: DeviceBuffer, rows: int, cells: int, events, wet_threshold_depth: float = 0.0,
                                 include_correct_negative: bool = False, names=None) -> np.ndarray:
        """The codes of ``detection_categories`` from two ``(rows, cells)`` device fields and ``[(lo, hi)]`` row ranges."""
        lo, hi = check_ranges(events, rows)
        E = lo.size
        lib = _lib.load()
        codes_dev = DeviceBuffer(-(-E * cells // 8) * 8, self.device)
        try:
            first = C.c_int64(-1)
            check(lib.gprx_dg_detect_dev(self.handle, truth.ptr, pred.ptr, rows, cells, ptr(lo), ptr(hi), E, float(wet_threshold_depth),
                                         int(bool(include_correct_negative)), codes_dev.ptr, C.byref(first)))
            if first.value >= 0:
                which = names[first.value] if names is not None else first.value
                raise ValueError(f"y_true and y_pred must be non-negative. (event {which!r})")
            codes = np.empty((E, cells), dtype=np.uint8)
            check(lib.gprx_memcpy_d2h(self.device, ptr(codes), codes_dev.ptr, codes.nbytes))
            return codes
        finally:
            codes_dev.free()

    def detection_categories(self, y_true, y_pred, events, wet_threshold_depth: float = 0.0, include_correct_negative: bool = False):
        """``map_detection_categories`` (plotting.py:758-802) without the drawing.  ``y_true``, ``y_pred``: ``(rows, cells)``; ``events``:
        a list of contiguous row ranges ``(lo, hi)``, or a two-level ``(event, timestep)`` pandas index whose events are contiguous.
        Returns ``(codes, CATEGORY_NAMES)``: ``codes`` ``(E, cells)`` uint8 in the order of the input columns (the reference sorts the
        cells by id for drawing), ``CATEGORY_NAMES[code]`` the reference's category, code 0 its empty string (a comparison with
        NaN, or a Correct Negative that is not included).  Raises ``ValueError("y_true and y_pred must be non-negative. ...")`` naming the
        first event with a negative maximum (plotting.py:776-777)."""
        y_true, y_pred = as_f64(y_true), as_f64(y_pred)
        if y_true.ndim != 2 or y_true.shape != y_pred.shape or y_true.size == 0:
            raise ValueError("y_true and y_pred must be (rows, cells) arrays of one shape")
        names = None
        if hasattr(events, "get_level_values"):
            names, events = event_ranges(events)
        check_ranges(events, y_true.shape[0])  # before anything goes up
        held = self._pair(y_true, y_pred)
        try:
            codes = self.detection_categories_dev(held[0].buf, held[1].buf, y_true.shape[0], y_true.shape[1], events, wet_threshold_depth,
                                                  include_correct_negative, names)
        finally:
            for x in held:
                x.free()
        return codes, CATEGORY_NAMES
