"""Depth-frequency maps: a weighted storm catalogue accumulated on the device into the rate at which every cell exceeds every depth level.

What a flood-risk study delivers is, per cell, the depth exceeded with a given annual probability (the "1 % depth").  It comes from a
whole catalogue of storms, each with a weight -- the annual rate of the stratum it stands for -- and each contributing its peak with the
surrogate's uncertainty: the ``peak (S, cells)`` block of ``PeakEnsemble`` (``S = 1``: a deterministic peak, of the mean prediction or of
the truth).

``FrequencyMaps(projector, levels)`` owns one device block, ``rate (L, cells)`` doubles and ``nan_members (cells,)`` int32, both zero at
first.  ``add_peaks(peak, members, weight)`` adds one event (``gprx_pca_freq_accumulate_dev``, csrc/frequency.h): per cell and level
``n = #{s: peak[s, c] > d_l}`` (strict), ``t = n / S``, ``u = w t``, ``rate += u`` -- three rounded operations, the counting in integers.
``depth_at(aep)`` inverts (``gprx_pca_freq_invert_dev``): ``k = #{l: rate[l, c] >= p}`` and the depth between the levels ``k - 1`` and ``k``.
``rate[:, c]`` is non-increasing in the level exactly; a permutation of an event's members or an event of weight 0 changes no bit; a
cell's state depends on its own column alone; the order of the events is the caller's and does matter.  DESIGN.md section 3.26 has the
definitions and the argument; ``PeakEnsemble.evaluate(frequency=..., weights=...)`` feeds every event's peaks.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._device import load_npz, save_npz
from ._lib import DeviceBuffer, as_f64, check, ptr

MAX_LEVELS, MAX_MEMBERS, MAX_TARGETS = 256, 4096, 16
INTERPS = {"linear": 0, "step": 1}
FILE_FORMAT = "gpras_amd.frequency_maps.v1"


def check_levels(levels) -> np.ndarray:
    """``levels`` as float64: between 1 and ``MAX_LEVELS`` finite, strictly increasing depths."""
    lv = np.ascontiguousarray(np.atleast_1d(np.asarray(levels, dtype=np.float64)))
    if lv.ndim != 1 or not 1 <= lv.size <= MAX_LEVELS:
        raise ValueError(f"need between 1 and {MAX_LEVELS} levels")
    if not np.all(np.isfinite(lv)):
        raise ValueError("the levels must be finite")
    if np.any(lv[1:] <= lv[:-1]):
        raise ValueError("the levels must be strictly increasing")
    return lv


def check_weight(weight) -> float:
    """An event's weight, the annual rate of its stratum: finite and not negative."""
    try:
        w = float(weight)
    except (TypeError, ValueError):
        raise ValueError("the weight must be a number") from None
    if not np.isfinite(w) or w < 0.0:
        raise ValueError("the weight must be finite and not negative")
    return w


def check_weights(weights, n_events: int) -> np.ndarray:
    """The weights of a catalogue of ``n_events`` events as float64: one per event, each as ``check_weight`` takes it."""
    if weights is None:
        raise ValueError("the frequency maps need the events' weights: one per event")
    w = np.ascontiguousarray(np.atleast_1d(np.asarray(weights, dtype=np.float64)))
    if w.ndim != 1 or w.size != int(n_events):
        raise ValueError(f"need one weight per event: {int(n_events)}")
    for value in w.tolist():
        check_weight(value)
    return w


def check_targets(aep) -> np.ndarray:
    """The targets of an inversion as float64: between 1 and ``MAX_TARGETS`` finite, positive rates."""
    p = np.ascontiguousarray(np.atleast_1d(np.asarray(aep, dtype=np.float64)))
    if p.ndim != 1 or not 1 <= p.size <= MAX_TARGETS:
        raise ValueError(f"need between 1 and {MAX_TARGETS} targets")
    if not np.all(np.isfinite(p)) or np.any(p <= 0.0):
        raise ValueError("the targets must be finite and positive")
    return p


def check_interp(interp) -> int:
    if interp not in INTERPS:
        raise ValueError(f"interp must be one of {tuple(INTERPS)}")
    return INTERPS[interp]


def check_members(members) -> int:
    members = int(members)
    if not 1 <= members <= MAX_MEMBERS:
        raise ValueError(f"members must be between 1 and {MAX_MEMBERS}")
    return members


@dataclass
class FrequencyDepth:
    """``depth (n_aep, cells)``: the depth exceeded at the rate ``aep[j]``; ``-inf`` where even the lowest level is exceeded less often,
    ``+inf`` where the levels do not reach high enough, NaN where a member of the cell was NaN.  ``bracket (n_aep, cells)`` int32: the
    number ``k`` of levels whose rate is at least the target (the depth lies between the levels ``k - 1`` and ``k``), -1 where flagged."""

    depth: np.ndarray
    bracket: np.ndarray
    aep: np.ndarray
    levels: np.ndarray
    interp: str

    def resolved(self) -> np.ndarray:
        """True where the depth lies inside the levels: ``0 < bracket < L``."""
        return (self.bracket > 0) & (self.bracket < self.levels.size)


class FrequencyMaps:
    def __init__(self, projector, levels):
        """``projector``: the ``EOFProjector`` whose cells and stream the maps share; ``levels``: the depths ``d_0 < d_1 < ...``, at most 256.
        The device block is made at the first use, so building the object needs no device."""
        self.levels = check_levels(levels)
        self.projector = projector
        self.device = projector.device
        self.cells = int(projector.n_cells)
        self.n_events = 0
        self.weights: list[float] = []
        self.last_device_ms = 0.0  # device time of the last accumulate (``gprx_pca_freq_ms``)
        self._block = None

    # ---- the device block: rate (L, cells) doubles, then nan_members (cells) int32 ---------------------------------------------------
    @property
    def _rate_doubles(self) -> int:
        return int(self.levels.size) * self.cells

    @property
    def _block_doubles(self) -> int:
        return self._rate_doubles + (self.cells + 1) // 2

    def _state(self) -> DeviceBuffer:
        if self._block is None:
            self._block = DeviceBuffer.from_array(np.zeros(self._block_doubles), self.device)
        return self._block

    def _upload(self, rate: np.ndarray, nan_members: np.ndarray) -> None:
        host = np.zeros(self._block_doubles)
        host[: self._rate_doubles] = rate.ravel()
        host[self._rate_doubles:].view(np.int32)[: self.cells] = nan_members
        self.close()
        self._block = DeviceBuffer.from_array(host, self.device)

    def _download(self):
        if self._block is None:
            return np.zeros((self.levels.size, self.cells)), np.zeros(self.cells, dtype=np.int32)
        host = self._block.to_array((self._block_doubles,))
        return (host[: self._rate_doubles].reshape(self.levels.size, self.cells).copy(),
                host[self._rate_doubles:].view(np.int32)[: self.cells].copy())

    def close(self):
        if self._block is not None:
            self._block.free()
            self._block = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        if rc == _lib.GPRX_EINVAL:
            raise ValueError((_lib.load().gprx_pca_last_error(self.projector.handle) or b"").decode())
        check(rc)

    # ---- the catalogue -----------------------------------------------------------------------------------------------------------------
    def add_peaks(self, peak, members: int, weight) -> None:
        """One event: ``peak`` a ``DeviceBuffer`` of the ``(members, cells)`` block (it stays the caller's) or a host array of that shape."""
        members, w = check_members(members), check_weight(weight)
        owned = None
        if isinstance(peak, DeviceBuffer):
            if peak.nbytes < 8 * members * self.cells:
                raise ValueError(f"the peak buffer must hold ({members}, {self.cells}) doubles")
        else:
            arr = as_f64(peak)
            if arr.shape != (members, self.cells):
                raise ValueError(f"peak must be ({members}, {self.cells})")
            peak = owned = DeviceBuffer.from_array(arr, self.device)
        try:
            lib, block = _lib.load(), self._state()
            self._check(lib.gprx_pca_freq_accumulate_dev(self.projector.handle, peak.ptr, members, int(self.levels.size), ptr(self.levels), w, block.ptr,
                                                         block.at(self._rate_doubles)))
            ms = C.c_double()
            check(lib.gprx_pca_freq_ms(self.projector.handle, C.byref(ms)))
            self.last_device_ms = ms.value
        finally:
            if owned is not None:
                owned.free()
        self.n_events += 1
        self.weights.append(w)

    def add_field(self, field, ranges, weights) -> None:
        """Deterministic peaks: per event ``(lo, hi)`` of ``ranges`` the maximum over the rows ``[lo, hi)`` of ``field (rows, cells)``, a host array
        or a ``DeviceBuffer`` (``gprx_pca_member_peaks_dev`` with one member: the first maximum, a NaN taken as the maximum), added with one
        member and the event's weight."""
        from .diagnostics import check_ranges

        resident = isinstance(field, DeviceBuffer)
        if resident:
            rows = field.nbytes // (8 * self.cells)
        else:
            field = np.asarray(field)
            if field.ndim != 2 or field.shape[1] != self.cells:
                raise ValueError(f"field must be (rows, {self.cells})")
            rows = field.shape[0]
        lo, hi = check_ranges(ranges, rows)
        w = check_weights(weights, lo.size)
        lib, ph = _lib.load(), self.projector.handle
        peak = DeviceBuffer(8 * self.cells, self.device)
        try:
            for a, b, we in zip(lo.tolist(), hi.tolist(), w.tolist()):
                owned = None if resident else DeviceBuffer.from_array(field[a:b], self.device)
                try:
                    check(lib.gprx_pca_member_peaks_dev(ph, field.at(a * self.cells) if resident else owned.ptr, 1, b - a, peak.ptr))
                    check(lib.gprx_pca_synchronize(ph))
                finally:
                    if owned is not None:
                        owned.free()
                self.add_peaks(peak, 1, we)
        finally:
            peak.free()

    # ---- what has been accumulated ---------------------------------------------------------------------------------------------------------
    def rate(self) -> np.ndarray:
        """``(L, cells)``: the rate at which each cell exceeds each level, in the weights' unit."""
        return self._download()[0]

    def nan_members(self) -> np.ndarray:
        """``(cells,)`` int32: the NaN members met per cell over the whole catalogue."""
        return self._download()[1]

    def depth_at(self, aep, interp: str = "linear") -> FrequencyDepth:
        """The depth exceeded at each rate of ``aep`` (at most 16, finite and positive): ``interp="linear"`` between the bracketing levels in the
        rate, ``"step"`` the level below."""
        p, mode = check_targets(aep), check_interp(interp)
        cells, n = self.cells, int(p.size)
        # one block: depth (n, cells) doubles | bracket (n, cells) int32
        out = DeviceBuffer(8 * (n * cells + (n * cells + 1) // 2), self.device)
        try:
            block = self._state()
            self._check(_lib.load().gprx_pca_freq_invert_dev(self.projector.handle, block.ptr, block.at(self._rate_doubles), int(self.levels.size),
                                                             ptr(self.levels), n, ptr(p), mode, out.ptr, out.at(n * cells)))
            host = out.to_array((n * cells + (n * cells + 1) // 2,))
        finally:
            out.free()
        return FrequencyDepth(host[: n * cells].reshape(n, cells).copy(), host[n * cells:].view(np.int32)[: n * cells].reshape(n, cells).copy(), p,
                              self.levels.copy(), interp)

    # ---- storage -------------------------------------------------------------------------------------------------------------------------
    def to_file(self, path) -> None:
        """The levels, the state and the catalogue's weights: a catalogue continued from the file has the bits of an uninterrupted one."""
        rate, nan_members = self._download()
        save_npz(path, FILE_FORMAT, {"levels": self.levels, "rate": rate, "nan_members": nan_members, "weights": np.asarray(self.weights, dtype=np.float64),
                                     "n_events": np.array(self.n_events, dtype=np.int64)})

    @classmethod
    def from_file(cls, path, projector) -> "FrequencyMaps":
        z = load_npz(path, FILE_FORMAT, "frequency maps")
        fm = cls(projector, z["levels"])
        rate, nan_members = as_f64(z["rate"]), np.ascontiguousarray(z["nan_members"], dtype=np.int32)
        if rate.shape != (fm.levels.size, fm.cells) or nan_members.shape != (fm.cells,):
            raise ValueError(f"{path}: the maps are over {rate.shape[-1]} cells, the projector over {fm.cells}")
        fm.weights = [float(v) for v in z["weights"].tolist()]
        fm.n_events = int(z["n_events"])
        fm._upload(rate, nan_members)
        return fm
