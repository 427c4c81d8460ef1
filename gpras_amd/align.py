"""Per-event temporal clipping of the HF and LF fields: ``DataBuilder._align_datasets`` / ``get_cutoff`` / ``_delta_cols_norm``
(``gpras/preprocess.py:89-155``) on the device.

For one plan the reference lays the HF field and the resampled LF field side by side (``combo``), drops the rows from the first NaN
on, normalises the absolute row-to-row changes of every column by their sum, and reads two indices off the cumulative curve of the
summed changes: ``start``, where it passes ``10e-4`` (the warm-up), and ``stop``, where it passes ``flow_convergence_threshold``.
Rows ``[start, stop)`` of both fields are kept.  Both are indices of *difference* rows used unshifted as row indices, as in the
reference.

``EventAligner`` runs that rule on the GPU (``csrc/align.h``) over device blocks, so that the chain plan blocks -> gather / resample
(``MeshResampler``) -> cutoff -> clip -> EOF features (``aligned_features``) moves only the raw rows up and ``(stop - start, k)``
numbers per plan down.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._device import DeviceHandle, StageTimer, slab_rows
from ._lib import DeviceBuffer, as_f64, check, ptr

FILE_FORMAT = "gpras_amd-align-1"
MAX_BLOCKS = 4  # csrc/align.h: AL_MAX_BLOCKS


class _Slab:
    """One projector's slab of clipped rows on the device, (rows, cells_p), filled across plans and projected whenever it is full:
    the slabs of ``PreProcessor.transform`` over the concatenated rows."""

    def __init__(self, aligner, projector, n_cells, cells_p, most_rows, laps):
        self.al, self.proj, self.n_cells, self.cells_p, self.laps = aligner, projector, n_cells, cells_p, laps
        self.k, self.fill, self.buf, self.out = projector.spatial_mode_count, 0, None, []
        self.rows = slab_rows(projector, most_rows)

    def take(self, field, start, stop):
        """Rows [start, stop) of ``field`` (., cells_p) go into the slab."""
        lib = _lib.load()
        if self.buf is None:
            self.buf = DeviceBuffer(8 * self.rows * self.cells_p, self.al.device)
        while start < stop:
            n = min(stop - start, self.rows - self.fill)
            check(lib.gprx_al_clip_dev(self.al.handle, field.ptr, self.cells_p, self.n_cells, start, start + n, self.buf.at(self.fill * self.cells_p), self.cells_p))
            check(lib.gprx_al_synchronize(self.al.handle))  # before the projector's stream reads the slab
            self.laps.lap("clip")
            self.fill += n
            start += n
            if self.fill == self.rows:
                self.flush()

    def flush(self):
        """Project the rows held and bring their features down."""
        if not self.fill:
            return
        lib = _lib.load()
        feat = DeviceBuffer(8 * self.fill * self.k, self.al.device)
        try:
            check(lib.gprx_pca_transform_dev(self.proj.handle, self.buf.ptr, self.fill, feat.ptr))
            check(lib.gprx_pca_synchronize(self.proj.handle))
            self.laps.lap("transform")
            self.out.append(feat.to_array((self.fill, self.k)))
            self.laps.link_bytes += 8 * self.fill * self.k
            self.laps.lap("download")
        finally:
            feat.free()
        self.fill = 0

    def features(self):
        return np.concatenate(self.out) if self.out else np.empty((0, self.k))

    def free(self):
        if self.buf is not None:
            self.buf.free()
            self.buf = None


def _pair(block):
    return tuple(block) if isinstance(block, (tuple, list)) else (block, None)


class EventAligner(DeviceHandle):
    """``flow_convergence_threshold`` and ``cutoffs`` of ``DataBuilder`` (:70-71, :85), and the clipping they drive."""

    destroy_symbol = "gprx_al_destroy"

    def __init__(self, flow_convergence_threshold: float = 0.95, cutoffs=None, device: int = 0):
        super().__init__()
        threshold = float(flow_convergence_threshold)
        if not np.isfinite(threshold):
            raise ValueError("flow_convergence_threshold must be finite")
        self.flow_convergence_threshold = threshold
        self.cutoffs: dict = {}
        for plan, c in dict(cutoffs or {}).items():
            self.cutoffs[plan] = self._cutoff_entry(c)
        self.device = device
        self.last_timings_ms: dict[str, float] = {}

    @staticmethod
    def _cutoff_entry(c) -> tuple[int, int]:
        c = tuple(c)
        if len(c) != 2 or any(int(v) != v or v < 0 for v in c):
            raise ValueError("a cutoff is (start, stop): two non-negative integers")
        return int(c[0]), int(c[1])

    # ---- device state -------------------------------------------------------------------------------------------------------------
    def _create(self):
        check(_lib.load().gprx_al_create(self.device, C.byref(self._h)))

    @staticmethod
    def _two_rows(T: int) -> None:
        if T < 2:
            raise ValueError("fewer than 2 rows: no difference row to judge")  # the reference: argmax of an empty sequence

    @classmethod
    def _combo(cls, combo) -> np.ndarray:
        a = as_f64(combo)
        if a.ndim != 2 or a.shape[1] < 1:
            raise ValueError("combo must be (T, C) with at least one column")
        cls._two_rows(a.shape[0])
        return a

    def _cutoff_dev(self, blocks, rows: int, want_curve: bool = False):
        """``blocks``: [(device pointer, cols, ld)] sharing ``rows`` -> (start, stop, rows_used, curve or None)."""
        if not 1 <= len(blocks) <= MAX_BLOCKS:
            raise ValueError(f"1 to {MAX_BLOCKS} blocks")
        n = len(blocks)
        ptrs = (C.c_void_p * n)(*[b[0] if isinstance(b[0], C.c_void_p) else C.c_void_p(b[0]) for b in blocks])
        cols = (C.c_int64 * n)(*[int(b[1]) for b in blocks])
        ld = (C.c_int64 * n)(*[int(b[2]) for b in blocks])
        start, stop, used = C.c_int64(), C.c_int64(), C.c_int64()
        curve = np.empty(max(rows - 1, 1)) if want_curve else None
        check(_lib.load().gprx_al_cutoff_dev(self.handle, n, ptrs, cols, ld, rows, self.flow_convergence_threshold, C.byref(start), C.byref(stop),
                                             C.byref(used), None if curve is None else ptr(curve)))
        return int(start.value), int(stop.value), int(used.value), None if curve is None else curve[: used.value - 1].copy()

    # ---- preprocess.py:135-155 ------------------------------------------------------------------------------------------------------
    def _cutoff_host(self, combo, want_curve: bool):
        a = self._combo(combo)
        start, stop, used = C.c_int64(), C.c_int64(), C.c_int64()
        curve = np.empty(a.shape[0] - 1) if want_curve else None
        check(_lib.load().gprx_al_cutoff(self.handle, ptr(a), a.shape[0], a.shape[1], self.flow_convergence_threshold, C.byref(start), C.byref(stop),
                                         C.byref(used), None if curve is None else ptr(curve)))
        return int(start.value), int(stop.value), None if curve is None else curve[: used.value - 1].copy()

    def get_cutoff(self, combo) -> tuple[int, int]:
        """``DataBuilder.get_cutoff`` (:135-147) for a host array ``combo`` (T, C)."""
        return self._cutoff_host(combo, False)[:2]

    def cutoff_curve(self, combo) -> np.ndarray:
        """The cumulative curve of ``get_cutoff`` (:143), (T' - 1,): the curve whose crossings are the cutoffs, what ``_plot_cutoff_diagnostic``
        (:157-161) is about."""
        return self._cutoff_host(combo, True)[2]

    # ---- preprocess.py:89-133 -------------------------------------------------------------------------------------------------------
    def align(self, plan_data):
        """``_align_datasets`` (:89-116).  ``plan_data``: an iterable of ``(plan, hf (T, n_hf), lf (T, n_lf))``.  A plan already in
        ``self.cutoffs`` keeps its entry, another gets one computed over its two blocks on the device; only rows ``[start, stop)`` of
        both come back.  Returns ``(hf_aligned, lf_aligned, runs, t)``: the plans' rows concatenated in order and the two levels of
        the reference's index."""
        lib = _lib.load()
        hf_store, lf_store, runs, ts = [], [], [], []
        n_hf = n_lf = None
        for plan, hf, lf in plan_data:
            hf, lf = as_f64(hf), as_f64(lf)
            if hf.ndim != 2 or lf.ndim != 2 or hf.shape[0] != lf.shape[0] or hf.shape[1] < 1 or lf.shape[1] < 1:
                raise ValueError(f"plan {plan!r}: hf and lf must be (T, n_hf) and (T, n_lf) with the same T")
            if n_hf is not None and (hf.shape[1], lf.shape[1]) != (n_hf, n_lf):
                raise ValueError(f"plan {plan!r}: every plan must have the same columns")
            n_hf, n_lf = hf.shape[1], lf.shape[1]
            T = hf.shape[0]
            if plan in self.cutoffs:  # nothing to compute: the slices of the host arrays are the result
                start, stop = self.cutoffs[plan]
                hf_rows, lf_rows = hf[start:stop].copy(), lf[start:stop].copy()
            else:
                self._two_rows(T)  # before anything goes up
                bufs: list[DeviceBuffer] = []
                try:
                    for a in (hf, lf):
                        bufs.append(DeviceBuffer.from_array(a, self.device))
                    start, stop, _, _ = self._cutoff_dev([(bufs[0].ptr, n_hf, n_hf), (bufs[1].ptr, n_lf, n_lf)], T)
                    self.cutoffs[plan] = (start, stop)
                    dur = max(stop - start, 0)
                    hf_rows, lf_rows = np.empty((dur, n_hf)), np.empty((dur, n_lf))
                    if dur:  # pitch = columns: the kept rows are one contiguous piece of each block
                        check(lib.gprx_memcpy_d2h(self.device, ptr(hf_rows), bufs[0].at(start * n_hf), hf_rows.nbytes))
                        check(lib.gprx_memcpy_d2h(self.device, ptr(lf_rows), bufs[1].at(start * n_lf), lf_rows.nbytes))
                finally:
                    for b in bufs:
                        b.free()
            hf_store.append(hf_rows)
            lf_store.append(lf_rows)
            runs += [plan] * len(hf_rows)
            ts.append(np.arange(len(hf_rows)))
        if not hf_store:
            raise ValueError("no plans")
        return np.concatenate(hf_store), np.concatenate(lf_store), np.array(runs), np.concatenate(ts)

    def clip(self, plan, table):
        """The slice ``aligned_ref_line_df`` (:125-133) takes of another per-plan table: rows ``[start, stop)`` by the plan's cutoff."""
        if plan not in self.cutoffs:
            raise KeyError(f"no cutoff for plan {plan!r}: align it first")
        start, stop = self.cutoffs[plan]
        return table.iloc[start:stop].copy() if hasattr(table, "iloc") else np.asarray(table)[start:stop].copy()

    def aligned_features(self, plan_rows, hf_gather, lf_resampler, hf_projector, lf_projector):
        """Plan blocks -> the GP's ``(x, y, runs, t)`` without a ``T x n_cells`` field on the host.  ``plan_rows``: an iterable of
        ``(plan, hf_block (T, n_hf_full), lf_block (T, n_lf))``; a block of a velocity resampler is the pair ``(vx, vy)``.  Per plan:
        the raw rows go up, ``hf_gather`` (``MeshResampler.nearest(hf_resampler, n_cells)``) and ``lf_resampler`` build the two
        fields in HBM, the cutoff runs over them as two device blocks, and rows ``[start, stop)`` of each are clipped into that
        side's slab, which ``gprx_pca_transform_dev`` projects whenever it is full and at the end: the slabs are those of
        ``PreProcessor.transform`` over the concatenated aligned rows, so ``x`` = ``lf_projector.transform(lf_aligned)`` and ``y`` =
        ``hf_projector.transform(hf_aligned)`` of the host chain bit for bit.  Only the features come down.  A slab holds the
        projector's slab rows, or the rows of all plans when ``plan_rows`` is a sequence and they are fewer."""
        lib = _lib.load()
        n_cells = hf_gather.n_out
        if lf_resampler.n_out != n_cells or hf_projector.n_cells != n_cells or lf_projector.n_cells != n_cells:
            raise ValueError(f"the resamplers and the projectors must cover the same {n_cells} cells")
        laps = StageTimer(("upload", "resample", "cutoff", "clip", "transform", "download"))
        cells_p = -(-n_cells // 16) * 16
        most_rows = sum(int(np.shape(_pair(hf)[0])[0]) for _, hf, _ in plan_rows) if hasattr(plan_rows, "__len__") else None
        runs, ts = [], []
        slabs = [_Slab(self, proj, n_cells, cells_p, most_rows, laps) for proj in (hf_projector, lf_projector)]
        try:
            for plan, hf_block, lf_block in plan_rows:
                hf_src, lf_src = hf_gather._sources(*_pair(hf_block)), lf_resampler._sources(*_pair(lf_block))
                T = hf_src[0].shape[0]
                if lf_src[0].shape[0] != T:
                    raise ValueError(f"plan {plan!r}: the HF and LF blocks must have the same rows")
                if plan not in self.cutoffs:
                    self._two_rows(T)
                bufs: list[DeviceBuffer] = []
                try:
                    fields = []
                    for rs, src in ((hf_gather, hf_src), (lf_resampler, lf_src)):
                        up = []
                        for a in src:
                            if a is not None:
                                up.append(DeviceBuffer.from_array(a, self.device))
                                bufs.append(up[-1])
                                laps.link_bytes += up[-1].nbytes
                        laps.lap("upload")
                        field = DeviceBuffer(8 * T * cells_p, self.device)
                        bufs.append(field)
                        check(lib.gprx_rs_apply_dev(rs.handle, T, up[0].ptr, rs.n_src, up[1].ptr if len(up) > 1 else None, field.ptr, cells_p))
                        check(lib.gprx_rs_synchronize(rs.handle))
                        fields.append(field)
                        laps.lap("resample")
                    if plan not in self.cutoffs:
                        start, stop, _, _ = self._cutoff_dev([(f.ptr, n_cells, cells_p) for f in fields], T)
                        self.cutoffs[plan] = (start, stop)
                        laps.link_bytes += 16  # the two integers
                    start, stop = self.cutoffs[plan]
                    stop = min(stop, T)  # a preset cutoff: numpy's slice stops at the last row
                    laps.lap("cutoff")
                    for slab, field in zip(slabs, fields):
                        slab.take(field, start, stop)
                finally:
                    for b in bufs:
                        b.free()
                dur = max(stop - start, 0)
                runs += [plan] * dur
                ts.append(np.arange(dur))
            for slab in slabs:
                slab.flush()
        finally:
            for slab in slabs:
                slab.free()
        if not ts:
            raise ValueError("no plans")
        y, x = slabs[0].features(), slabs[1].features()
        self.last_timings_ms = laps.finish()  # the link bytes: the raw rows up; the features, and two integers per computed cutoff, down
        return x, y, np.array(runs), np.concatenate(ts)

    def stage_timings_ms(self) -> dict[str, float]:
        """Device milliseconds of the last cutoff call by stage (``gprx_al_timings``)."""
        out = np.zeros(4)
        check(_lib.load().gprx_al_timings(self.handle, out.ctypes.data_as(C.POINTER(C.c_double))))
        return dict(zip(("scan", "normalisers", "row_sums", "finish"), out.tolist()))

    # ---- storage --------------------------------------------------------------------------------------------------------------------
    def to_dict(self) -> dict[str, np.ndarray]:
        """Plain arrays (what an ``.npz`` stores) plus the format string.  Plans are stored by name: a plan key that is not a string
        would come back as another key (and its cutoff be computed again), so it is refused here."""
        plans = list(self.cutoffs)
        if not all(isinstance(p, str) for p in plans):
            raise ValueError("to_dict stores plans by name: every key of cutoffs must be a string")
        return {"format": np.array(FILE_FORMAT), "flow_convergence_threshold": np.array(self.flow_convergence_threshold),
                "cutoff_plans": np.array(plans, dtype=np.str_),
                "cutoffs": np.array([self.cutoffs[p] for p in plans], dtype=np.int64).reshape(len(plans), 2)}

    @classmethod
    def from_dict(cls, d, device: int = 0) -> "EventAligner":
        if "format" not in d or str(d["format"]) != FILE_FORMAT:
            raise ValueError("not an event-aligner record")
        plans, cut = [str(p) for p in np.asarray(d["cutoff_plans"]).reshape(-1)], np.asarray(d["cutoffs"]).reshape(-1, 2)
        if len(plans) != len(cut):
            raise ValueError("cutoff_plans and cutoffs disagree")
        return cls(float(d["flow_convergence_threshold"]), {p: (int(c[0]), int(c[1])) for p, c in zip(plans, cut)}, device)
