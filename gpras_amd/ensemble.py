"""Peak ensembles: joint posterior draws of a fitted ``GPRAS`` pushed through the field chain to maps of an EVENT's peak.

Every uncertainty ``GPRAS.predict`` returns is a marginal per (time step, cell); the reference forms the 2.5 % / 97.5 % bands from it
(production/analysis/pipeline.py:262-263).  What a flood-risk user asks for is a functional of a whole event -- the probability that the
event's maximum depth exceeds a threshold, the quantile maps of the peak depth, the distribution of the inundated area -- and the
maximum over an event's rows does not follow from marginals: the GP's predictions at those rows are strongly correlated.

``PeakEnsemble(gpr, projector).evaluate(x_test, ranges, members, ...)`` works event by event:

* ``Engine.predict_joint_batch_dev`` (``gprx_predict_joint_batch_dev``): per mode the mean over the event's rows and the lower Cholesky
  factor ``Lc`` of the joint predictive covariance ``Kss - tmp1^T tmp1 + tmp2^T tmp2`` (the quantities of gpflow's ``SGPR.predict_f`` with
  the diagonal kept joint), padded with the identity to ``Tp`` = rows rounded up to 64;
* standard normals ``Zn (K, S, Tp)`` from the caller or from ``np.random.default_rng(seed)``, drawn event by event in the order of
  ``ranges`` as ``rng.standard_normal((K, S, rows))`` -- or, with ``rng="device"``, drawn on the device by address
  (``gprx_pca_normals_dev``, csrc/normals.h: Philox4x64-10 and Wichura's AS 241; a draw is a function of seed, stream, event, mode, member
  and row alone); ``W_k = Zn_k Lc_k^T`` by the batched fp64 GEMM and one packing kernel give the
  members' scores ``(S rows, K)``.  Modes are independent of each other, as the reference's variance propagation assumes, and so are events;
* ``route="fused"``: ``gprx_pca_ensemble_peaks_dev`` (csrc/ensemble.h) walks every member's rows per cell and writes only
  ``peak (S, cells)``;  ``route="refield"``: the same numbers, bit for bit, from ``gprx_pca_reverse_dev`` -> ``gprx_pca_to_depth_dev`` on
  slabs of whole members and a per-member row maximum;
* ``gprx_pca_member_stats_dev``: exceedance counts, mean, standard deviation, order statistics and wet areas over the members;
* with ``observed=`` the truth: ``gprx_pca_member_verify_dev`` (csrc/verify.h) sorts every cell's members on chip and scores them against the
  event's observed peak -- the CRPS and the rank counts per cell --, and ``PeakVerification`` aggregates those maps on the host: rank
  histogram, mean CRPS, Brier score, reliability table, coverage of a quantile band.

* with ``timing=True``: the same walk (``gprx_pca_ensemble_timing_dev``, csrc/timing.h, in place of the peaks kernel) also leaves per member
  the row of the peak and per threshold the rows above it and the first of them; ``gprx_pca_timing_stats_dev`` reduces those integer maps over
  the members and ``EventTiming`` holds the result: when the water arrives, how long it stays, when it peaks.

DESIGN.md section 3.23 has the mapping, the determinism argument and the measurement behind ``DEFAULT_ROUTE``; section 3.24 the verification;
section 3.25 the event timing.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._device import StageTimer, slab_rows
from ._lib import DeviceBuffer, as_f64, check, ptr
from .diagnostics import check_ranges

ROUTES = ("fused", "refield")
DEFAULT_ROUTE = "fused"  # the route measured faster at the production shape (profiles/ensemble_peaks.json)
RNGS = ("host", "device")
# "host" keeps the bits every earlier release drew (np.random.default_rng(seed), one sequential stream); "device" draws by address on the
# GPU (csrc/normals.h) and removes the host generator and the upload from the call -- measured in one run at the production shape
# (profiles/ensemble_rng.json): the draw_upload stage 300 ms against 3.1 ms, the whole call 1.05 s against 0.73 s.
# The default stays "host" so that a seed keeps its draws.
DEFAULT_RNG = "host"
DEPTH_MODES = {"velocity": 0, "wse": 1, "depth": 2}
JOINT_MAX_M, JOINT_MAX_ROWS, JOINT_MAX_D = 320, 1024, 64
MAX_MEMBERS, MAX_THRESHOLDS, MAX_RANKS = 4096, 8, 8
MAX_LEVELS = 8  # levels of the distribution function per ``gprx_pca_timing_stats_dev``: ``durations`` and ``arrive_by`` of ``evaluate``
MAX_EVENT_ROWS = 2**31 - 2  # the timing maps are int32 and the arrival's sentinel is the row count itself
# (the statistics' stage includes their download; ``observed=`` adds "verify", ``timing=True`` adds "timing", ``frequency=`` adds "frequency")
STAGES = ("joint", "draw_upload", "draws", "peaks", "stats")


def joint_applies(n_inducing, d: int, rows: int) -> str | None:
    """None when ``gprx_predict_joint_batch_dev`` takes this configuration, else the reason it does not."""
    if n_inducing is None:
        return "exact model (n_inducing=None)"
    if int(n_inducing) > JOINT_MAX_M:
        return f"more than {JOINT_MAX_M} inducing points"
    if d > JOINT_MAX_D:
        return f"more than {JOINT_MAX_D} features"
    if rows > JOINT_MAX_ROWS:
        return f"an event of more than {JOINT_MAX_ROWS} rows"
    if rows < 1:
        return "an event without rows"
    return None


def padded_rows(rows: int) -> int:
    """``Tp``: an event's rows rounded up to 64, the order of its padded Cholesky factor."""
    return (int(rows) + 63) // 64 * 64


def quantile_ranks(quantiles, members: int) -> np.ndarray:
    """``floor(q (S - 1))`` per quantile: the rank ``np.quantile(..., method="lower")`` reads."""
    q = np.atleast_1d(np.asarray(quantiles, dtype=np.float64))
    if q.ndim != 1 or np.any(~(q >= 0.0)) or np.any(~(q <= 1.0)):
        raise ValueError("quantiles must lie in [0, 1]")
    return np.floor(q * (int(members) - 1)).astype(np.int32)


def check_stats_args(members: int, thresholds, ranks):
    """``(thresholds float64, ranks int32)`` as ``gprx_pca_member_stats_dev`` takes them."""
    members = int(members)
    if not 1 <= members <= MAX_MEMBERS:
        raise ValueError(f"members must be between 1 and {MAX_MEMBERS}")
    thr = np.ascontiguousarray(np.atleast_1d(np.asarray(thresholds, dtype=np.float64)))
    if thr.ndim != 1 or thr.size > MAX_THRESHOLDS:
        raise ValueError(f"at most {MAX_THRESHOLDS} thresholds")
    if np.any(np.isnan(thr)):
        raise ValueError("a threshold is NaN")
    rk = np.atleast_1d(np.asarray(ranks))
    if rk.size and rk.dtype.kind not in "iu":
        raise ValueError("ranks must be integers")
    rk = np.ascontiguousarray(rk, dtype=np.int32)
    if rk.ndim != 1 or rk.size > MAX_RANKS:
        raise ValueError(f"at most {MAX_RANKS} ranks")
    if np.any(rk < 0) or np.any(rk >= members):
        raise ValueError("ranks must lie in [0, members)")
    return thr, rk


def check_verify_args(members: int, ranks) -> np.ndarray:
    """``ranks`` int32 as ``gprx_pca_member_verify_dev`` takes them: at most ``MAX_RANKS`` integers in ``[0, members)``, ``members`` in range."""
    return check_stats_args(members, (), ranks)[1]


def check_observed(observed, rows: int, cells: int):
    """``observed`` of ``evaluate``: a ``DeviceBuffer`` of at least ``(rows, cells)`` doubles as it is, anything else as a float64 array of
    exactly that shape."""
    if isinstance(observed, DeviceBuffer):
        if observed.nbytes < 8 * rows * cells:
            raise ValueError(f"the observed buffer must hold ({rows}, {cells}) doubles")
        return observed
    arr = as_f64(observed)
    if arr.shape != (rows, cells):
        raise ValueError(f"observed must be ({rows}, {cells}): one row per row of x_test, one column per cell")
    return arr


def check_seed(value, name: str) -> int:
    """``value`` as the unsigned 64-bit integer a key word of the device generator is."""
    try:
        v = int(value)
        ok = v == value and 0 <= v < 2**64
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{name} must be an integer in [0, 2**64)")
    return v


def check_event_ranges(ranges, rows: int):
    """The events' ``(lo, hi)`` as int64 arrays: non-empty, inside ``[0, rows]``, in ascending order and disjoint."""
    lo, hi = check_ranges(ranges, rows)
    if np.any(lo[1:] < lo[:-1]):
        raise ValueError("the events must be in ascending order")
    if np.any(lo[1:] < hi[:-1]):
        raise ValueError("the events overlap")
    return lo, hi


def timing_maps(n_thr: int) -> int:
    """The maps of a timing block: ``t_peak``, then a duration and an arrival per threshold."""
    return 1 + 2 * int(n_thr)


def check_levels(values, name: str) -> np.ndarray:
    """``values`` (``durations`` or ``arrive_by``) as int32: at most ``MAX_LEVELS`` non-negative integers, in rows."""
    v = np.atleast_1d(np.asarray(values))
    if v.size == 0:
        return np.zeros(0, dtype=np.int32)
    if v.dtype.kind not in "iu":
        raise ValueError(f"{name} must be integers (rows)")
    if v.ndim != 1 or v.size > MAX_LEVELS:
        raise ValueError(f"at most {MAX_LEVELS} {name}")
    if np.any(v < 0) or np.any(v > MAX_EVENT_ROWS):
        raise ValueError(f"{name} must lie in [0, {MAX_EVENT_ROWS}]")
    return np.ascontiguousarray(v, dtype=np.int32)


def check_timing_args(timing: bool, thresholds, durations=(), arrive_by=()):
    """``(durations, arrive_by)`` int32 as ``evaluate`` takes them: each at most ``MAX_LEVELS`` non-negative integers; ``timing=True`` needs a
    threshold, and without it neither list may be given."""
    dur, by = check_levels(durations, "durations"), check_levels(arrive_by, "arrive_by")
    if not timing:
        if dur.size or by.size:
            raise ValueError("durations and arrive_by need timing=True")
    elif np.atleast_1d(np.asarray(thresholds)).size == 0:
        raise ValueError("timing=True needs at least one threshold")
    return dur, by


def check_timing_stats_args(members: int, n_maps: int, map0: int, n_sel: int, rows: int, sentinel: int = -1, levels=(), ranks=()):
    """``(levels int32, ranks int32)`` as ``gprx_pca_timing_stats_dev`` takes them, the other arguments checked as it checks them."""
    _, rk = check_stats_args(members, (), ranks)
    n_maps, map0, n_sel, rows, sentinel = int(n_maps), int(map0), int(n_sel), int(rows), int(sentinel)
    if not 1 <= rows <= MAX_EVENT_ROWS:
        raise ValueError(f"an event has between 1 and {MAX_EVENT_ROWS} rows")
    if not 1 <= n_maps <= timing_maps(MAX_THRESHOLDS) or map0 < 0 or n_sel < 1 or map0 + n_sel > n_maps:
        raise ValueError(f"the maps [map0, map0 + n_sel) must lie inside the block's n_maps <= {timing_maps(MAX_THRESHOLDS)}")
    if sentinel != -1 and not 0 <= sentinel <= rows:
        raise ValueError("the sentinel must be -1 (none) or a value in [0, rows]")
    lv = np.atleast_1d(np.asarray(levels))
    if lv.size and lv.dtype.kind not in "iu":
        raise ValueError("levels must be integers")
    if lv.ndim != 1 or lv.size > MAX_LEVELS:
        raise ValueError(f"at most {MAX_LEVELS} levels")
    if lv.size and (np.any(lv < -(2**31)) or np.any(lv >= 2**31)):
        raise ValueError("levels must be 32-bit integers")
    return np.ascontiguousarray(lv, dtype=np.int32), rk


@dataclass
class EnsembleResult:
    """Per event ``e``: ``p_exceed (E, n_thr, cells)`` = exceedance counts / S; ``peak_mean``, ``peak_std`` ``(E, cells)`` (ddof = 0);
    ``peak_quantiles (E, n_q, cells)`` = the order statistic of rank ``floor(q (S - 1))``; ``wet_area (E, S, n_thr)``; ``exceed_counts`` the
    integer counts themselves."""

    p_exceed: np.ndarray
    peak_mean: np.ndarray
    peak_std: np.ndarray
    peak_quantiles: np.ndarray
    wet_area: np.ndarray
    exceed_counts: np.ndarray
    thresholds: np.ndarray
    quantiles: np.ndarray
    ranges: list
    members: int
    route: str
    last_timings_ms: dict = field(default_factory=dict)
    names: list = field(default_factory=list)  # the events' labels (``DevicePipeline.peak_ensemble``)
    rng: str = DEFAULT_RNG  # where the normals were drawn ("host" also when the caller passed ``normals``)
    verification: "PeakVerification | None" = None  # the ensemble against the observed peaks (``evaluate(observed=...)``)
    timing: "EventTiming | None" = None  # arrival, duration and time of the peak (``evaluate(timing=True)``)


@dataclass
class PeakVerification:
    """The ensemble of every event against the peak that happened, per cell as ``gprx_pca_member_verify_dev`` leaves it: ``crps (E, cells)``,
    ``below`` and ``equal`` ``(E, cells)`` int32 -- the members below the observed peak and equal to it, -1 where the observation or a member
    is NaN --, ``observed_peak (E, cells)``, and the result's ``exceed_counts (E, n_thr, cells)`` at ``thresholds``.  The aggregations are
    host numpy over these ``(E, cells)`` maps: O(cells), and exact integers where they count.  A cell with an infinite member or
    observation is valid (its counts are counts) while its CRPS may be NaN: pass a ``mask`` to keep it out of ``mean_crps``."""

    crps: np.ndarray
    below: np.ndarray
    equal: np.ndarray
    observed_peak: np.ndarray
    members: int
    thresholds: np.ndarray
    exceed_counts: np.ndarray
    names: list = field(default_factory=list)

    @property
    def valid(self) -> np.ndarray:
        return self.below >= 0

    def _mask(self, mask) -> np.ndarray:
        if mask is None:
            return self.valid
        m = np.asarray(mask, dtype=bool)
        return self.valid & np.broadcast_to(m, self.below.shape)

    def _weights(self, cell_areas, mask) -> np.ndarray:
        a = np.ones(self.below.shape[1]) if cell_areas is None else np.asarray(cell_areas, dtype=np.float64)
        if a.shape != (self.below.shape[1],):
            raise ValueError(f"cell_areas must be ({self.below.shape[1]},)")
        return np.where(self._mask(mask), a[None, :], 0.0)

    def rank_histogram(self, mask=None) -> np.ndarray:
        """``(E, S + 1)``: the Talagrand histogram of the observation's rank among the members.  A cell with ``(b, q) = (below, equal)`` puts
        ``1 / (q + 1)`` into each of the bins ``b .. b + q`` (ties share the cell evenly).  The default mask is ``valid & (equal < S)``: it
        drops the cells where the truth and every member coincide (dry everywhere).  A row sums to the number of counted cells."""
        s = int(self.members)
        m = self._mask(self.equal < s if mask is None else mask)
        hist = np.zeros((self.below.shape[0], s + 1))
        for e in range(hist.shape[0]):
            b, q = self.below[e][m[e]].astype(np.int64), self.equal[e][m[e]].astype(np.int64)
            for ties in np.unique(q).tolist():
                start = np.bincount(b[q == ties], minlength=s + 1)  # cells whose run of bins starts here: integers
                run = np.cumsum(start)
                run[ties + 1:] -= run[: s - ties].copy()  # cells whose run covers the bin, still integers
                hist[e] += run if ties == 0 else run / (ties + 1.0)
        return hist

    def mean_crps(self, cell_areas=None, mask=None) -> np.ndarray:
        """``(E,)``: the (area-weighted) mean of the CRPS over the valid cells of ``mask``."""
        w = self._weights(cell_areas, mask)
        with np.errstate(invalid="ignore", divide="ignore"):
            return (np.where(w > 0.0, self.crps, 0.0) * w).sum(axis=1) / w.sum(axis=1)

    def brier(self, cell_areas=None, mask=None) -> np.ndarray:
        """``(E, n_thr)``: the (area-weighted) mean of ``(p - o)^2`` with ``p = exceed_counts / S`` and ``o = observed_peak > threshold``
        (strict, as the exceedance itself)."""
        w = self._weights(cell_areas, mask)
        p = self.exceed_counts / float(self.members)
        o = (self.observed_peak[:, None, :] > np.asarray(self.thresholds, dtype=np.float64)[None, :, None]).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return ((p - o) ** 2 * w[:, None, :]).sum(axis=2) / w.sum(axis=1)[:, None]

    def reliability(self, bins: int = 10) -> np.ndarray:
        """int64 ``(E, n_thr, bins, 2)`` over the valid cells: ``[..., 0]`` the forecasts whose exceedance count falls into the bin
        ``min(bins - 1, count * bins // S)`` (integer arithmetic), ``[..., 1]`` those among them where the observed peak exceeded."""
        bins = int(bins)
        if bins < 1:
            raise ValueError("bins must be positive")
        ne, n_thr = self.exceed_counts.shape[:2]
        out = np.zeros((ne, n_thr, bins, 2), dtype=np.int64)
        idx = np.minimum(bins - 1, self.exceed_counts.astype(np.int64) * bins // int(self.members))
        for e in range(ne):
            v = self.valid[e]
            for j in range(n_thr):
                o = self.observed_peak[e][v] > self.thresholds[j]
                out[e, j, :, 0] = np.bincount(idx[e, j][v], minlength=bins)
                out[e, j, :, 1] = np.bincount(idx[e, j][v][o], minlength=bins)
        return out

    def coverage(self, lo_rank: int, hi_rank: int) -> np.ndarray:
        """``(E,)``: the share of the valid cells whose observed peak lies in ``[x_(lo_rank), x_(hi_rank)]`` of the sorted members:
        ``below + equal >= lo_rank + 1`` and ``below <= hi_rank``."""
        lo_rank, hi_rank = int(lo_rank), int(hi_rank)
        if not 0 <= lo_rank <= hi_rank < int(self.members):
            raise ValueError("need 0 <= lo_rank <= hi_rank < members")
        v = self.valid
        inside = v & (self.below.astype(np.int64) + self.equal >= lo_rank + 1) & (self.below <= hi_rank)
        with np.errstate(invalid="ignore", divide="ignore"):
            return inside.sum(axis=1) / v.sum(axis=1).astype(np.float64)


@dataclass
class EventTiming:
    """When the water arrives, how long it stays and when it peaks, per event ``e`` and cell over the ``members`` of the ensemble, in ROWS
    counted from the event's first (hours are the caller's ``dt``).  Per member: ``t_peak`` the row of the first maximum, ``duration[j]``
    the rows with depth ``> thresholds[j]`` (strict), ``arrival[j]`` the first of them.  What is stored are the exact integers
    ``gprx_pca_timing_stats_dev`` leaves; the probabilities and means are properties, one division each:

    * ``t_peak_sum (E, cells)`` int64, ``t_peak_quantiles (E, n_q, cells)`` int32 (rank ``floor(q (S - 1))``, as the peak's quantiles);
    * ``duration_sum (E, n_thr, cells)`` int64, ``duration_quantiles (E, n_thr, n_q, cells)``, ``duration_below_counts (E, n_thr, n_dur, cells)``:
      the members with ``duration <= durations[i] - 1``;
    * ``arrival_counts (E, n_thr, cells)``: the members that arrive at all (it equals the exceedance count of the peak), ``arrival_sum`` over those
      members, ``arrival_quantiles (E, n_thr, n_q, cells)`` over ALL members -- the value ``rows[e]`` reads "not within the event" --,
      ``arrival_by_counts (E, n_thr, n_by, cells)``: the members with ``arrival <= arrive_by[i]`` (a member that never arrives is in none);
    * with ``observed=``: ``observed (E, n_maps, cells)`` the same maps of the truth (``n_maps = 1 + 2 n_thr``: ``t_peak``, the durations, the
      arrivals) and ``below``, ``equal`` ``(E, n_maps, cells)``: the members below the observed value and equal to it."""

    t_peak_sum: np.ndarray
    t_peak_quantiles: np.ndarray
    duration_sum: np.ndarray
    duration_quantiles: np.ndarray
    duration_below_counts: np.ndarray
    arrival_counts: np.ndarray
    arrival_sum: np.ndarray
    arrival_quantiles: np.ndarray
    arrival_by_counts: np.ndarray
    rows: np.ndarray
    members: int
    thresholds: np.ndarray
    quantiles: np.ndarray
    durations: np.ndarray
    arrive_by: np.ndarray
    observed: np.ndarray | None = None
    below: np.ndarray | None = None
    equal: np.ndarray | None = None
    names: list = field(default_factory=list)

    @property
    def t_peak_mean(self) -> np.ndarray:
        """``(E, cells)``: the mean row of the peak."""
        return self.t_peak_sum / float(self.members)

    @property
    def duration_mean(self) -> np.ndarray:
        """``(E, n_thr, cells)``: the mean number of rows above the threshold (members that stay dry count with 0)."""
        return self.duration_sum / float(self.members)

    @property
    def p_duration_at_least(self) -> np.ndarray:
        """``(E, n_thr, n_dur, cells)``: ``P(duration >= durations[i]) = 1 - cdf(durations[i] - 1) / S``."""
        return 1.0 - self.duration_below_counts / float(self.members)

    @property
    def p_arrival(self) -> np.ndarray:
        """``(E, n_thr, cells)``: the share of the members in which the water arrives within the event."""
        return self.arrival_counts / float(self.members)

    @property
    def arrival_mean(self) -> np.ndarray:
        """``(E, n_thr, cells)``: the mean arrival row over the members that arrive; NaN where none does."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.arrival_counts > 0, self.arrival_sum / self.arrival_counts.astype(np.float64), np.nan)

    @property
    def p_arrival_by(self) -> np.ndarray:
        """``(E, n_thr, n_by, cells)``: ``P(arrival <= arrive_by[i])``."""
        return self.arrival_by_counts / float(self.members)


class PeakEnsemble:
    def __init__(self, gpr, projector):
        """``gpr``: a fitted (or loaded) ``gpras_amd.GPRAS`` of sparse models; ``projector``: the ``EOFProjector`` of its outputs."""
        if not getattr(gpr, "models", None):
            raise ValueError("the GPRAS model has not been fitted or loaded")
        if len(gpr.models) != projector.spatial_mode_count:
            raise ValueError(f"the model has {len(gpr.models)} outputs, the projector {projector.spatial_mode_count} spatial modes")
        self.gpr, self.projector = gpr, projector
        self.device = projector.device
        self._lib = _lib.load()
        self.last_device_peaks_ms = 0.0  # device time of the last fused peak kernel (``gprx_pca_ensemble_ms``)
        self.last_device_verify_ms = 0.0  # device time of the last verification kernel (``gprx_pca_member_verify_ms``)
        self.last_device_timing_ms = 0.0  # device time of the last fused timing kernel (``gprx_pca_ensemble_timing_ms``)

    def _check(self, rc: int) -> None:
        """``check``, with the handle's reason as a ValueError where the library refused the arguments."""
        if rc == _lib.GPRX_EINVAL:
            raise ValueError((self._lib.gprx_pca_last_error(self.projector.handle) or b"").decode())
        check(rc)

    # ---- 1. joint prediction over one event -------------------------------------------------------------------------------------------
    def joint_dev(self, x_event, include_noise: bool = True):
        """``(mean, Lc, rows)``: device buffers ``(K, rows)`` and ``(K, Tp, Tp)`` of one event's joint prediction.  The caller frees them."""
        x = as_f64(np.asarray(x_event).astype(np.float64))
        models = self.gpr.models
        if x.ndim != 2 or x.shape[1] != self.gpr.x.shape[1]:
            raise ValueError(f"x must be (rows, {self.gpr.x.shape[1]})")
        rows, k = int(x.shape[0]), len(models)
        for mod in models:
            why_not = joint_applies(None if mod.Z is None else mod.Z.shape[0], x.shape[1], rows)
            if why_not:
                raise ValueError(f"the joint prediction does not serve this model: {why_not}")
        tp = padded_rows(rows)
        dev = self.device
        xs_dev = DeviceBuffer.from_array(x, dev)
        mean = DeviceBuffer(8 * k * rows, dev)
        lc = DeviceBuffer(8 * k * tp * tp, dev)
        try:
            by_engine: dict[int, list[int]] = {}
            for i, mod in enumerate(models):
                by_engine.setdefault(id(mod.backend), []).append(i)
            for idx in by_engine.values():
                eng = models[idx[0]].backend
                chunk = max(1, min(64, eng.max_cells(want_grad=False)))
                runs: list[list[int]] = []
                for i in idx:
                    if runs and runs[-1][-1] + 1 == i and len(runs[-1]) < chunk:
                        runs[-1].append(i)
                    else:
                        runs.append([i])
                for part in runs:
                    units = [models[i].unit for i in part]
                    thetas = np.stack([models[i].theta() for i in part])
                    zs = np.stack([models[i].Z for i in part])
                    eng.predict_joint_batch_dev(units, thetas, xs_dev, rows, mean.at(part[0] * rows), lc.at(part[0] * tp * tp), zs=zs,
                                                include_noise=include_noise)
        except Exception:
            mean.free()
            lc.free()
            raise
        finally:
            xs_dev.free()
        return mean, lc, rows

    # ---- 2. draws -----------------------------------------------------------------------------------------------------------------------
    def normals_dev(self, event: int, members: int, rows: int, seed: int = 0, stream: int = 0, antithetic: bool = False, member0: int = 0,
                    raw: bool = False) -> DeviceBuffer:
        """The standard normals ``(K, members, Tp)`` of event ``event`` on the device, as ``scores_dev`` takes them: the draw of
        ``(seed, stream, event, mode, member0 + slot, row)`` by ``gprx_pca_normals_dev`` (include/gprx.h has the addressing), exact zeros in the
        columns ``rows <= t < Tp``.  ``antithetic``: the second half of the ``members`` (counted from member 0; ``members`` even) is the exact
        negation of the first; a slice ``member0, members`` of a larger antithetic ensemble passes ``antithetic=`` that ensemble's half size.
        ``raw``: the generator's 64-bit words instead (``to_array(...).view(np.uint64)``).  The caller frees the buffer."""
        event, members, rows, member0 = int(event), int(members), int(rows), int(member0)
        seed, stream = check_seed(seed, "seed"), check_seed(stream, "stream")
        if members < 1 or rows < 1:
            raise ValueError("members and rows must be positive")
        if isinstance(antithetic, (bool, np.bool_)):
            if antithetic and (member0 != 0 or members % 2):
                raise ValueError("antithetic=True pairs the halves of an even number of members counted from member 0; pass the half size for a slice")
            pair = members // 2 if antithetic else 0
        else:
            pair = int(antithetic)
        k, tp = self.projector.spatial_mode_count, padded_rows(rows)
        zbuf = DeviceBuffer(8 * k * members * tp, self.device)
        try:
            rc = self._lib.gprx_pca_normals_dev(self.projector.handle, seed, stream, event, member0, members, pair, rows, tp, int(bool(raw)), zbuf.ptr)
            if rc == _lib.GPRX_EINVAL:
                raise ValueError((self._lib.gprx_pca_last_error(self.projector.handle) or b"").decode())
            check(rc)
            # the batched GEMM that reads the block runs on the library's utility stream, not the projector's: hand over a finished block
            check(self._lib.gprx_pca_synchronize(self.projector.handle))
        except Exception:
            zbuf.free()
            raise
        return zbuf

    def scores_dev(self, mean_dev, lc_dev, normals, members: int, rows: int, timer: StageTimer | None = None) -> DeviceBuffer:
        """The members' scores ``(S rows, K)`` on the device: ``scores[s, t, k] = mean[k, t] + (Zn_k Lc_k^T)[s, t]``.  ``normals``: ``(K, S, rows)``
        or ``(K, S, Tp)`` standard normals on the host (the columns beyond ``rows`` meet the identity padding and are not read back), or a
        ``DeviceBuffer`` of the ``(K, S, Tp)`` block with zeros in those columns (``normals_dev``): nothing is staged or uploaded then, and
        the buffer stays the caller's."""
        k, tp, dev = self.projector.spatial_mode_count, padded_rows(rows), self.device
        resident = isinstance(normals, DeviceBuffer)
        if resident:
            if normals.nbytes < 8 * k * members * tp:
                raise ValueError(f"the normals buffer must hold ({k}, {members}, {tp}) doubles")
        else:
            zn = np.asarray(normals, dtype=np.float64)
            if zn.ndim != 3 or zn.shape[:2] != (k, members) or zn.shape[2] not in (rows, tp):
                raise ValueError(f"normals must be ({k}, {members}, {rows}) or ({k}, {members}, {tp})")
            zp = np.zeros((k, members, tp))
            zp[:, :, : zn.shape[2]] = zn
        zbuf = wbuf = scores = None
        try:
            zbuf = normals if resident else DeviceBuffer.from_array(zp, dev)
            wbuf = DeviceBuffer(8 * k * members * tp, dev)
            scores = DeviceBuffer(8 * members * rows * k, dev)
            if timer is not None:
                if not resident:
                    timer.link_bytes += zbuf.nbytes
                timer.lap("draw_upload")
            # W_k (S, Tp) = Zn_k (S, Tp) . Lc_k^T: the (0, 1) form, op(B) = Lc^T upper triangular (Lc's strict upper triangle is zero)
            check(self._lib.gprx_gemm_batched(dev, 0, 1, members, tp, tp, 1.0, zbuf.ptr, tp, lc_dev.ptr if hasattr(lc_dev, "ptr") else lc_dev, tp, 0.0,
                                              wbuf.ptr, tp, _lib.GEMM_B_UPPER, 64, k, members * tp, tp * tp, members * tp, 1, 0, 0, 0, None, 0, None, 0))
            check(self._lib.gprx_pca_pack_scores_dev(self.projector.handle, mean_dev.ptr if hasattr(mean_dev, "ptr") else mean_dev, wbuf.ptr, members,
                                                     rows, tp, scores.ptr))
            check(self._lib.gprx_pca_synchronize(self.projector.handle))
        except Exception:
            if scores is not None:
                scores.free()
            raise
        finally:
            for buf in (wbuf,) if resident else (zbuf, wbuf):
                if buf is not None:
                    buf.free()
        if timer is not None:
            timer.lap("draws")
        return scores

    # ---- 3. peaks -----------------------------------------------------------------------------------------------------------------------
    def member_peaks_dev(self, scores, members: int, rows: int, route: str | None = None, member_group: int = 0) -> DeviceBuffer:
        """``peak (S, cells)`` on the device from the members' scores: a host array ``(S, rows, K)`` or a device buffer of that block."""
        return self._member_walk(scores, members, rows, route, member_group, None)[0]

    def member_timing_dev(self, scores, members: int, rows: int, thresholds, route: str | None = None, member_group: int = 0):
        """``(peak, timing)`` on the device from the members' scores (as ``member_peaks_dev`` takes them): ``peak (S, cells)``, bit for bit
        ``member_peaks_dev``'s, and the int32 block ``timing (S, n_maps, cells)``, ``n_maps = 1 + 2 n_thr``: map 0 the row of the peak
        (``np.argmax`` over the member's rows), map ``1 + j`` the rows with depth ``> thresholds[j]`` (strict), map ``1 + n_thr + j`` the first
        of them, ``rows`` where there is none.  ``route="fused"``: ``gprx_pca_ensemble_timing_dev``, one walk for both; ``route="refield"``:
        reverse -> depth -> ``gprx_pca_member_timing_dev`` on slabs of whole members.  The caller frees both buffers."""
        thr, _ = check_stats_args(1, thresholds, ())
        return self._member_walk(scores, members, rows, route, member_group, thr)

    def _member_walk(self, scores, members: int, rows: int, route, member_group: int, thr):
        """``(peak, timing)`` of one walk over the members' rows; ``thr`` None: the peaks alone (``timing`` None)."""
        route = DEFAULT_ROUTE if route is None else route
        if route not in ROUTES:
            raise ValueError(f"route must be one of {ROUTES}")
        pr, lib, dev = self.projector, self._lib, self.device
        members, rows = int(members), int(rows)
        if members < 1 or rows < 1:
            raise ValueError("members and rows must be positive")
        if pr.hydraulic_parameter != "velocity" and pr.elevations is None:
            raise ValueError("wse_2_depth needs the cell elevations (the projector was built without them)")
        k, cells = pr.spatial_mode_count, pr.n_cells
        owned = None
        if not hasattr(scores, "ptr"):
            arr = as_f64(scores)
            if arr.shape != (members, rows, k):
                raise ValueError(f"scores must be ({members}, {rows}, {k})")
            scores = owned = DeviceBuffer.from_array(arr, dev)
        elif getattr(scores, "nbytes", 8 * members * rows * k) < 8 * members * rows * k:
            raise ValueError("the scores buffer is too small")
        n_thr = 0 if thr is None else int(thr.size)
        member_ints = timing_maps(n_thr) * cells  # int32 values of one member's maps
        peak = timing = None
        try:
            peak = DeviceBuffer(8 * members * cells, dev)
            if thr is not None:
                timing = DeviceBuffer((4 * members * member_ints + 7) // 8 * 8, dev)
            ph = pr.handle
            ms = C.c_double()
            if route == "fused" and thr is None:
                check(lib.gprx_pca_ensemble_peaks_dev(ph, scores.ptr, members, rows, DEPTH_MODES[pr.hydraulic_parameter], int(member_group), peak.ptr))
                check(lib.gprx_pca_ensemble_ms(ph, C.byref(ms)))
                self.last_device_peaks_ms = ms.value
            elif route == "fused":
                self._check(lib.gprx_pca_ensemble_timing_dev(ph, scores.ptr, members, rows, DEPTH_MODES[pr.hydraulic_parameter], int(member_group), n_thr,
                                                             ptr(thr), peak.ptr, timing.ptr))
                check(lib.gprx_pca_ensemble_timing_ms(ph, C.byref(ms)))
                self.last_device_timing_ms = ms.value
            else:
                per_slab = max(1, min(members, 65535, slab_rows(pr) // rows))
                fieldbuf = DeviceBuffer(8 * per_slab * rows * cells, dev)
                try:
                    for s0 in range(0, members, per_slab):
                        ns = min(per_slab, members - s0)
                        check(lib.gprx_pca_reverse_dev(ph, scores.at(s0 * rows * k), None, ns * rows, fieldbuf.ptr, None))
                        if pr.hydraulic_parameter != "velocity":
                            check(lib.gprx_pca_to_depth_dev(ph, fieldbuf.ptr, ns * rows, int(pr.hydraulic_parameter == "depth")))
                        if thr is None:
                            check(lib.gprx_pca_member_peaks_dev(ph, fieldbuf.ptr, ns, rows, peak.at(s0 * cells)))
                        else:
                            self._check(lib.gprx_pca_member_timing_dev(ph, fieldbuf.ptr, ns, rows, n_thr, ptr(thr), peak.at(s0 * cells),
                                                                       C.c_void_p(timing.ptr.value + 4 * s0 * member_ints)))
                    check(lib.gprx_pca_synchronize(ph))
                finally:
                    fieldbuf.free()
        except Exception:
            for buf in (peak, timing):
                if buf is not None:
                    buf.free()
            raise
        finally:
            if owned is not None:
                owned.free()
        return peak, timing

    # ---- 3b. event timing: the observed maps and the statistics over the members' maps ------------------------------------------------------
    def observed_timing_dev(self, truth, lo: int, hi: int, thresholds) -> DeviceBuffer:
        """The observed timing maps, int32 ``(n_maps, cells)`` on the device, of the event in rows ``[lo, hi)`` of ``truth (rows, cells)`` (as
        ``observed_peak_dev`` takes it): ``gprx_pca_member_timing_dev`` with one member, so every rule is the members' own.  The caller frees it."""
        thr, _ = check_stats_args(1, thresholds, ())
        lo, hi = int(lo), int(hi)
        cells, dev = self.projector.n_cells, self.device
        if not 0 <= lo < hi:
            raise ValueError("need 0 <= lo < hi")
        owned = None
        if isinstance(truth, DeviceBuffer):
            if truth.nbytes < 8 * hi * cells:
                raise ValueError(f"the truth buffer does not reach row {hi}")
            src = truth.at(lo * cells)
        else:
            arr = np.asarray(truth)
            if arr.ndim != 2 or arr.shape[1] != cells or arr.shape[0] < hi:
                raise ValueError(f"truth must be (rows >= {hi}, {cells})")
            owned = DeviceBuffer.from_array(arr[lo:hi], dev)
            src = owned.ptr
        out = DeviceBuffer((4 * timing_maps(thr.size) * cells + 7) // 8 * 8, dev)
        try:
            self._check(self._lib.gprx_pca_member_timing_dev(self.projector.handle, src, 1, hi - lo, int(thr.size), ptr(thr), None, out.ptr))
            check(self._lib.gprx_pca_synchronize(self.projector.handle))
        except Exception:
            out.free()
            raise
        finally:
            if owned is not None:
                owned.free()
        return out

    def timing_to_array(self, timing_dev, members: int, n_maps: int) -> np.ndarray:
        """A timing block on the device as the host array int32 ``(members, n_maps, cells)``."""
        n = int(members) * int(n_maps) * self.projector.n_cells
        return timing_dev.to_array(((n + 1) // 2,)).view(np.int32)[:n].reshape(int(members), int(n_maps), self.projector.n_cells).copy()

    def timing_stats(self, timing_dev, members: int, n_maps: int, map0: int, n_sel: int, rows: int, sentinel: int = -1, levels=(), ranks=(),
                     obs_dev=None) -> dict:
        """The statistics over the members of the maps ``[map0, map0 + n_sel)`` of a timing block ``(S, n_maps, cells)`` on the device, as host
        arrays (``gprx_pca_timing_stats_dev``, csrc/timing.h), all exact integers: ``cdf (n_sel, n_lev, cells)`` int32, the members with a value
        ``<= levels[l]``; ``n_valid (n_sel, cells)`` int32 and ``sum (n_sel, cells)`` int64 over the members whose value is not ``sentinel`` (-1: every
        member counts); ``order (n_sel, n_rank, cells)`` int32 = ``np.sort(v, axis=0)[ranks]`` over all members; and with ``obs_dev``, the observed value of
        each selected map ``(n_sel, cells)`` int32 on the device (a pointer or a buffer), ``below`` and ``equal`` ``(n_sel, cells)`` int32."""
        lv, rk = check_timing_stats_args(members, n_maps, map0, n_sel, rows, sentinel, levels, ranks)
        pr, dev = self.projector, self.device
        cells, members, n_sel = pr.n_cells, int(members), int(n_sel)
        n_lev, n_rk = int(lv.size), int(rk.size)
        with_obs = obs_dev is not None
        # one block: sum (int64) | cdf | n_valid | order | below | equal (int32)
        mc = n_sel * cells
        o_cdf = 2 * mc
        o_valid = o_cdf + n_lev * mc
        o_order = o_valid + mc
        o_below = o_order + n_rk * mc
        n_int = o_below + (2 * mc if with_obs else 0)
        out = DeviceBuffer((4 * n_int + 7) // 8 * 8, dev)

        def at(off):
            return C.c_void_p(out.ptr.value + 4 * off)

        try:
            self._check(self._lib.gprx_pca_timing_stats_dev(
                pr.handle, timing_dev.ptr if hasattr(timing_dev, "ptr") else timing_dev, members, int(n_maps), int(map0), n_sel, int(rows), int(sentinel),
                n_lev, ptr(lv), n_rk, ptr(rk), None if not with_obs else (obs_dev.ptr if hasattr(obs_dev, "ptr") else obs_dev),
                at(o_cdf) if n_lev else None, at(o_valid), out.ptr, at(o_order) if n_rk else None, at(o_below) if with_obs else None,
                at(o_below + mc) if with_obs else None))
            host = out.to_array(((n_int + 1) // 2,))
        finally:
            out.free()
        ints = host.view(np.int32)
        res = {"sum": host[:mc].view(np.int64).reshape(n_sel, cells).copy(), "cdf": ints[o_cdf:o_valid].reshape(n_sel, n_lev, cells).copy(),
               "n_valid": ints[o_valid:o_order].reshape(n_sel, cells).copy(), "order": ints[o_order:o_below].reshape(n_sel, n_rk, cells).copy(),
               "below": None, "equal": None}
        if with_obs:
            res["below"] = ints[o_below:o_below + mc].reshape(n_sel, cells).copy()
            res["equal"] = ints[o_below + mc:o_below + 2 * mc].reshape(n_sel, cells).copy()
        return res

    # ---- 4. statistics ------------------------------------------------------------------------------------------------------------------
    def member_stats(self, peak_dev, members: int, thresholds=(), ranks=(), cell_areas=None) -> dict:
        """The statistics over the members of a ``(S, cells)`` peak block on the device, as host arrays: ``exceed (n_thr, cells)`` int32,
        ``mean``, ``std`` ``(cells,)``, ``order (n_rank, cells)``, ``wet_area (S, n_thr)``."""
        thr, rk = check_stats_args(members, thresholds, ranks)
        pr, dev = self.projector, self.device
        cells, members = pr.n_cells, int(members)
        area = None
        if cell_areas is not None:
            a = as_f64(cell_areas)
            if a.shape != (cells,):
                raise ValueError(f"cell_areas must be ({cells},)")
            area = DeviceBuffer.from_array(a, dev)
        n_thr, n_rk = int(thr.size), int(rk.size)
        # one block: exceed (int32) | mean | std | order | wet_area
        o_mean = (4 * n_thr * cells + 7) // 8
        o_std, o_order = o_mean + cells, o_mean + 2 * cells
        o_wet = o_order + n_rk * cells
        out = DeviceBuffer(8 * (o_wet + members * n_thr + 1), dev)
        try:
            check(self._lib.gprx_pca_member_stats_dev(pr.handle, peak_dev.ptr if hasattr(peak_dev, "ptr") else peak_dev, members, n_thr, ptr(thr), n_rk,
                                                      ptr(rk), None if area is None else area.ptr, out.ptr, out.at(o_mean), out.at(o_std), out.at(o_order),
                                                      out.at(o_wet)))
            host = out.to_array((o_wet + members * n_thr,))
        finally:
            out.free()
            if area is not None:
                area.free()
        exceed = host[:o_mean].view(np.int32)[: n_thr * cells].reshape(n_thr, cells).copy()
        return {"exceed": exceed, "mean": host[o_mean:o_std].copy(), "std": host[o_std:o_order].copy(),
                "order": host[o_order:o_wet].reshape(n_rk, cells).copy(), "wet_area": host[o_wet:].reshape(members, n_thr).copy()}

    # ---- 5. verification against the observed peak -----------------------------------------------------------------------------------------
    def observed_peak_dev(self, truth, lo: int, hi: int) -> DeviceBuffer:
        """The observed peak ``(cells,)`` of the event in rows ``[lo, hi)`` of ``truth (rows, cells)``, a host array or a device buffer already
        in the peaks' units: ``gprx_pca_member_peaks_dev`` with one member, so the first-maximum rule (a NaN is the maximum) is the members'
        own.  The caller frees the buffer."""
        lo, hi = int(lo), int(hi)
        cells, dev = self.projector.n_cells, self.device
        if not 0 <= lo < hi:
            raise ValueError("need 0 <= lo < hi")
        owned = None
        if isinstance(truth, DeviceBuffer):
            if truth.nbytes < 8 * hi * cells:
                raise ValueError(f"the truth buffer does not reach row {hi}")
            src = truth.at(lo * cells)
        else:
            arr = np.asarray(truth)
            if arr.ndim != 2 or arr.shape[1] != cells or arr.shape[0] < hi:
                raise ValueError(f"truth must be (rows >= {hi}, {cells})")
            owned = DeviceBuffer.from_array(arr[lo:hi], dev)
            src = owned.ptr
        out = DeviceBuffer(8 * cells, dev)
        try:
            check(self._lib.gprx_pca_member_peaks_dev(self.projector.handle, src, 1, hi - lo, out.ptr))
            check(self._lib.gprx_pca_synchronize(self.projector.handle))
        except Exception:
            out.free()
            raise
        finally:
            if owned is not None:
                owned.free()
        return out

    def verify_peaks(self, peak_dev, obs_dev, members: int, ranks=()) -> dict:
        """A ``(S, cells)`` peak block on the device against the observed peak ``(cells,)`` on the device, as host arrays
        (``gprx_pca_member_verify_dev``, csrc/verify.h): ``crps (cells,)``, ``below`` and ``equal`` ``(cells,)`` int32 and
        ``order (n_rank, cells)``, the sorted members at ``ranks``.  A cell whose observation or any member is NaN: ``crps`` NaN,
        ``below = equal = -1``; infinities follow the formula (``|inf - inf|`` makes the CRPS a NaN, the counts stay counts)."""
        rk = check_verify_args(members, ranks)
        pr, dev = self.projector, self.device
        cells, members, n_rk = pr.n_cells, int(members), int(rk.size)
        # one block: crps | order | below, equal (int32)
        o_order, o_int = cells, (1 + n_rk) * cells
        out = DeviceBuffer(8 * (o_int + cells), dev)
        try:
            below_ptr = out.at(o_int)
            equal_ptr = C.c_void_p(below_ptr.value + 4 * cells)
            rc = self._lib.gprx_pca_member_verify_dev(pr.handle, peak_dev.ptr if hasattr(peak_dev, "ptr") else peak_dev,
                                                      obs_dev.ptr if hasattr(obs_dev, "ptr") else obs_dev, members, n_rk, ptr(rk), out.ptr, below_ptr,
                                                      equal_ptr, out.at(o_order) if n_rk else None)
            if rc == _lib.GPRX_EINVAL:
                raise ValueError((self._lib.gprx_pca_last_error(pr.handle) or b"").decode())
            check(rc)
            ms = C.c_double()
            check(self._lib.gprx_pca_member_verify_ms(pr.handle, C.byref(ms)))
            self.last_device_verify_ms = ms.value
            host = out.to_array((o_int + cells,))
        finally:
            out.free()
        counts = host[o_int:].view(np.int32)
        return {"crps": host[:cells].copy(), "below": counts[:cells].copy(), "equal": counts[cells:].copy(),
                "order": host[o_order:o_int].reshape(n_rk, cells).copy()}

    # ---- the whole chain ------------------------------------------------------------------------------------------------------------------
    def evaluate(self, x_test, ranges, members: int, thresholds=(0.5,), quantiles=(0.05, 0.5, 0.95), seed=0, normals=None, cell_areas=None,
                 include_noise: bool = True, route: str | None = None, rng: str = DEFAULT_RNG, stream=0, antithetic: bool = False,
                 observed=None, timing: bool = False, durations=(), arrive_by=(), frequency=None, weights=None) -> EnsembleResult:
        """``x_test (rows, d)``; ``ranges``: the events' ``(lo, hi)`` row ranges, ascending and disjoint; ``members``: S.  ``normals``: one
        ``(K, S, rows_e)`` array per event instead of the generator seeded with ``seed``.  ``rng="host"``: ``np.random.default_rng(seed)``, one
        sequential stream over the events; ``rng="device"``: event ``e`` takes ``normals_dev(e, members, rows_e, seed, stream, antithetic)`` --
        every draw a function of ``(seed, stream, e, mode, member, row)`` alone, so the members of a smaller ensemble are the first members
        of a larger one; ``antithetic`` (device only, ``members`` even): member ``s + S / 2`` draws the negation of member ``s``.
        ``observed``: the truth ``(rows, cells)``, row-aligned with ``x_test`` and in the peaks' units, a host array (sent up event by event, every row once) or a
        ``DeviceBuffer``: every event's peaks are then also scored against its observed peak (``observed_peak_dev``, ``verify_peaks``) in a
        ``"verify"`` stage of the timer and the result carries a ``PeakVerification``; ``None`` launches nothing more and leaves
        ``verification`` None.
        ``timing=True`` (at least one threshold): the walk over the members' rows is ``member_timing_dev`` in place of ``member_peaks_dev`` -- one
        walk, the same ``peak`` bit for bit, so every other field of the result keeps its bits -- and a ``"timing"`` stage reduces the members'
        maps (``timing_stats``) to ``result.timing``, an ``EventTiming`` at ``thresholds`` and ``quantiles``: ``durations`` (rows, at most 8) are the
        ``D`` of ``p_duration_at_least``, ``arrive_by`` (rows, at most 8) the ``t`` of ``p_arrival_by``; with ``observed=`` it carries the observed maps
        (``observed_timing_dev``) and the members below and equal to them.  ``timing=False`` launches nothing more and leaves ``timing`` None.
        ``frequency``: a ``gpras_amd.frequency.FrequencyMaps`` over the same projector, with ``weights`` one per event (finite, not negative: the
        annual rate of the stratum the event stands for): after an event's peaks ``frequency.add_peaks(peak, members, weights[e])`` runs in a
        ``"frequency"`` stage of the timer and ``last_timings_ms["device_frequency"]`` sums its device time; every other field of the result keeps
        its bits.  ``frequency=None`` launches nothing more (``weights`` must then be None too)."""
        route = DEFAULT_ROUTE if route is None else route
        if route not in ROUTES:
            raise ValueError(f"route must be one of {ROUTES}")
        if rng not in RNGS:
            raise ValueError(f"rng must be one of {RNGS}")
        if rng == "device" and normals is not None:
            raise ValueError('normals were given: rng="device" would draw its own')
        # (the host generator keeps taking whatever np.random.default_rng takes -- None, a sequence --; an integer is held to the key's range)
        if rng == "device" or isinstance(seed, (int, np.integer)):
            seed = check_seed(seed, "seed")
        stream = check_seed(stream, "stream")
        if antithetic and rng != "device":
            raise ValueError('antithetic=True needs rng="device": the host stream has no member addressing to pair')
        if antithetic and int(members) % 2:
            raise ValueError("antithetic=True needs an even number of members")
        x = np.asarray(x_test)
        if x.ndim != 2:
            raise ValueError("x_test must be (rows, d)")
        lo, hi = check_event_ranges(ranges, x.shape[0])
        members = int(members)
        thr, _ = check_stats_args(members, thresholds, ())
        dur, by = check_timing_args(timing, thr, durations, arrive_by)
        q = np.atleast_1d(np.asarray(quantiles, dtype=np.float64))
        _, rk = check_stats_args(members, (), quantile_ranks(q, members))
        if normals is not None and len(normals) != lo.size:
            raise ValueError("one array of normals per event")
        k, cells, ne = self.projector.spatial_mode_count, self.projector.n_cells, int(lo.size)
        host_rng = np.random.default_rng(seed) if rng == "host" and normals is None else None
        if frequency is not None:
            from .frequency import check_weights

            weights = check_weights(weights, ne)
            if frequency.cells != cells:
                raise ValueError(f"the frequency maps are over {frequency.cells} cells, the projector over {cells}")
        elif weights is not None:
            raise ValueError("weights were given without frequency maps to add to")
        verify = observed is not None
        if verify:
            observed = check_observed(observed, x.shape[0], cells)
        timer = StageTimer(STAGES + (("verify",) if verify else ()) + (("timing",) if timing else ()) + (("frequency",) if frequency is not None else ()))
        counts = np.zeros((ne, thr.size, cells), dtype=np.int32)
        mean, std = np.zeros((ne, cells)), np.zeros((ne, cells))
        order = np.zeros((ne, rk.size, cells))
        wet = np.zeros((ne, members, thr.size))
        device_peaks = device_verify = device_frequency = 0.0
        if verify:
            crps, obs_peak = np.zeros((ne, cells)), np.zeros((ne, cells))
            below, equal = np.zeros((ne, cells), dtype=np.int32), np.zeros((ne, cells), dtype=np.int32)
        if timing:
            n_thr, n_q, n_maps = int(thr.size), int(rk.size), timing_maps(thr.size)
            tm = EventTiming(np.zeros((ne, cells), dtype=np.int64), np.zeros((ne, n_q, cells), dtype=np.int32),
                             np.zeros((ne, n_thr, cells), dtype=np.int64), np.zeros((ne, n_thr, n_q, cells), dtype=np.int32),
                             np.zeros((ne, n_thr, dur.size, cells), dtype=np.int32), np.zeros((ne, n_thr, cells), dtype=np.int32),
                             np.zeros((ne, n_thr, cells), dtype=np.int64), np.zeros((ne, n_thr, n_q, cells), dtype=np.int32),
                             np.zeros((ne, n_thr, by.size, cells), dtype=np.int32), (hi - lo).astype(np.int64), members, thr, q, dur, by)
            if verify:
                tm.observed, tm.below, tm.equal = (np.zeros((ne, n_maps, cells), dtype=np.int32) for _ in range(3))
        for e, (a, b) in enumerate(zip(lo.tolist(), hi.tolist())):
            rows = b - a
            mean_dev = lc_dev = scores = peak = zn = truth_peak = maps_dev = truth_maps = None
            try:
                mean_dev, lc_dev, _ = self.joint_dev(x[a:b], include_noise=include_noise)
                timer.lap("joint")
                # (timed with its upload, where there is one: "draw_upload")
                if rng == "device":
                    zn = self.normals_dev(e, members, rows, seed, stream, bool(antithetic))
                else:
                    zn = host_rng.standard_normal((k, members, rows)) if host_rng is not None else normals[e]
                scores = self.scores_dev(mean_dev, lc_dev, zn, members, rows, timer=timer)
                if timing:
                    peak, maps_dev = self.member_timing_dev(scores, members, rows, thr, route=route)
                else:
                    peak = self.member_peaks_dev(scores, members, rows, route=route)
                timer.lap("peaks")
                device_peaks += (self.last_device_timing_ms if timing else self.last_device_peaks_ms) if route == "fused" else 0.0
                st = self.member_stats(peak, members, thr, rk, cell_areas)
                timer.lap("stats")
                if verify:
                    # (a host truth goes up event by event, every row once: the events are disjoint)
                    truth_peak = self.observed_peak_dev(observed, a, b)
                    if not isinstance(observed, DeviceBuffer):
                        timer.link_bytes += 8 * rows * cells
                    vr = self.verify_peaks(peak, truth_peak, members)
                    device_verify += self.last_device_verify_ms
                    crps[e], below[e], equal[e], obs_peak[e] = vr["crps"], vr["below"], vr["equal"], truth_peak.to_array((cells,))
                    timer.lap("verify")
                if timing:
                    if verify:
                        truth_maps = self.observed_timing_dev(observed, a, b, thr)
                        if not isinstance(observed, DeviceBuffer):
                            timer.link_bytes += 8 * rows * cells
                        tm.observed[e] = self.timing_to_array(truth_maps, 1, n_maps)[0]
                    # the row of the peak | the durations | the arrivals (sentinel: the row count; a level at or past it would count it)
                    parts = ((0, 1, -1, ()), (1, n_thr, -1, dur - 1), (1 + n_thr, n_thr, rows, np.minimum(by, rows - 1)))
                    st_t, st_d, st_a = (self.timing_stats(maps_dev, members, n_maps, m0, n_sel, rows, sentinel, levels, rk,
                                                          None if truth_maps is None else C.c_void_p(truth_maps.ptr.value + 4 * m0 * cells))
                                        for m0, n_sel, sentinel, levels in parts)
                    tm.t_peak_sum[e], tm.t_peak_quantiles[e] = st_t["sum"][0], st_t["order"][0]
                    tm.duration_sum[e], tm.duration_quantiles[e], tm.duration_below_counts[e] = st_d["sum"], st_d["order"], st_d["cdf"]
                    tm.arrival_counts[e], tm.arrival_sum[e], tm.arrival_quantiles[e] = st_a["n_valid"], st_a["sum"], st_a["order"]
                    tm.arrival_by_counts[e] = st_a["cdf"]
                    if verify:
                        tm.below[e] = np.concatenate([st_t["below"], st_d["below"], st_a["below"]])
                        tm.equal[e] = np.concatenate([st_t["equal"], st_d["equal"], st_a["equal"]])
                    timer.lap("timing")
                if frequency is not None:
                    frequency.add_peaks(peak, members, weights[e])
                    device_frequency += frequency.last_device_ms
                    timer.lap("frequency")
            finally:
                for buf in (mean_dev, lc_dev, scores, peak, zn if rng == "device" else None, truth_peak, maps_dev, truth_maps):
                    if buf is not None:
                        buf.free()
            counts[e], mean[e], std[e], order[e], wet[e] = st["exceed"], st["mean"], st["std"], st["order"], st["wet_area"]
        timings = timer.finish()
        if route == "fused":
            timings["device_peaks"] = device_peaks
        if frequency is not None:
            timings["device_frequency"] = device_frequency
        verification = None
        if verify:
            timings["device_verify"] = device_verify
            verification = PeakVerification(crps, below, equal, obs_peak, members, thr, counts)
        return EnsembleResult(counts / members, mean, std, order, wet, counts, thr, q, list(zip(lo.tolist(), hi.tolist())), members, route, timings,
                              rng=rng, verification=verification, timing=tm if timing else None)
