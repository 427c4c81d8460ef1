"""Storm-event selection, the first stage of the reference's workflow (``production/pre_processing/event_selection.py:13-257``, class
``EventSelection``), with its numerics on the device (``gprx_ev_*``, ``csrc/events.h``):

* ``_calculate_return_periods`` (event_selection.py:34-67): per-event maxima, block maxima, their sort, the knots and scipy's linear
  ``interp1d`` -- ``event_max`` equals the reference's bit for bit;
* ``_select_diverse_storms`` (event_selection.py:148-185): the two pivots, an exact PCA of each, the standardised scores and the
  farthest-point loop, which runs incrementally and without a host round trip;
* ``_select_aep_storms`` (event_selection.py:73-146) and ``_select_test_storms`` (event_selection.py:187-237) work on the small
  ``event_max`` table and stay on the host.

Two documented differences from the reference.  On an exact tie between candidates the reference takes whichever comes first in the
iteration order of a Python ``set`` (event_selection.py:177); here the lowest event id wins.  The PCA here is always exact; the
reference's ``PCA(n_components)`` turns to scikit-learn's randomized solver with an unseeded generator when neither
``E >= 10 H`` (with ``H <= 1000``) nor ``max(E, H) <= 500`` holds, and then does not reproduce itself from run to run.
"""

from __future__ import annotations

import ctypes as C
import time

import numpy as np
import pandas as pd

from . import _lib
from ._device import DeviceHandle
from ._lib import check, ptr

MAX_HOURS = 4096  # csrc/abi_events.hip: EV_MAX_H
MAX_CELLS = 1 << 28  # csrc/abi_events.hip: EV_MAX_CELLS, events x (hours rounded up to 16)
MAX_EVENTS = (1 << 31) - 1
MAX_COMPONENTS = 32  # 2k <= 64 columns of the score matrix
COLUMNS = ("event_id", "datetime", "precip-excess", "precip-cum", "inflow")
TIMING_NAMES = ("pivot_maxima", "return_periods", "cov_precip", "cov_inflow", "scores", "standardise", "farthest", "device_eigh")


def rank_and_hour(event_id, datetime):
    """One ``np.lexsort`` by ``(event_id, datetime)``: ``(ids, rank, hour, order)`` with ``ids`` the sorted unique event ids, ``rank``
    (int32) the position of each row's event in ``ids`` and ``hour`` (int32) the position of each row inside its event -- the
    reference's ``sort_values(["event_id", "datetime"])`` and ``cumcount`` (event_selection.py:153-155) -- both in the ORIGINAL row
    order.  ``ValueError`` when an ``(event_id, datetime)`` pair repeats: its ``(event, hour)`` would not be unique."""
    event_id, datetime = np.asarray(event_id), np.asarray(datetime)
    if event_id.ndim != 1 or event_id.shape != datetime.shape or event_id.size == 0:
        raise ValueError("event_id and datetime must be one-dimensional arrays of one length, not empty")
    order = np.lexsort((datetime, event_id))
    ev_sorted, dt_sorted = event_id[order], datetime[order]
    new_event = np.empty(order.size, dtype=bool)
    new_event[0] = True
    new_event[1:] = ev_sorted[1:] != ev_sorted[:-1]
    repeats = int(np.count_nonzero(~new_event[1:] & (dt_sorted[1:] == dt_sorted[:-1])))
    if repeats:
        raise ValueError(f"(event, hour) pairs must be unique: {repeats} rows repeat the (event_id, datetime) of another row")
    starts = np.flatnonzero(new_event)
    ids = ev_sorted[starts]
    if ids.size > MAX_EVENTS:
        raise ValueError(f"need fewer than 2^31 events, got {ids.size}")
    rank_sorted = np.cumsum(new_event, dtype=np.int64) - 1
    rank = np.empty(order.size, dtype=np.int32)
    hour = np.empty(order.size, dtype=np.int32)
    rank[order] = rank_sorted
    hour[order] = np.arange(order.size, dtype=np.int64) - starts[rank_sorted]
    return ids, rank, hour, order


def check_shape(n_events: int, n_hours: int) -> None:
    """The bounds of the device path on the number of events E and the longest event H."""
    if n_events > MAX_EVENTS:
        raise ValueError(f"need fewer than 2^31 events, got {n_events}")
    if n_hours > MAX_HOURS:
        raise ValueError(f"the longest event has {n_hours} hours; the device path takes at most {MAX_HOURS}")
    if n_events * (-(-n_hours // 16) * 16) > MAX_CELLS:
        raise ValueError(f"events x hours (rounded up to 16) = {n_events} x {-(-n_hours // 16) * 16} exceeds 2^28 elements per pivot")


def sign_convention(components: np.ndarray) -> np.ndarray:
    """scikit-learn's ``svd_flip(u, vt, u_based_decision=False)`` on the rows of ``components`` (k, H): the entry of largest magnitude of
    every component (the first on ties) becomes positive."""
    components = np.array(components, dtype=np.float64)
    pos = np.argmax(np.abs(components), axis=1)
    signs = np.sign(components[np.arange(components.shape[0]), pos])
    return components * signs[:, None]


class EventSelector(DeviceHandle):
    """``EventSelection`` of the reference on five long-format columns; see the module text."""

    destroy_symbol = "gprx_ev_destroy"

    def __init__(self, event_id, datetime, precip_excess, precip_cum, inflow, arrival_rate: int = 10, window_ratio: float = 0.2, test_rp_range=None,
                 tol: float = 0.15, device: int = 0, eigensolver: str = "host"):
        super().__init__()
        self._set_parameters(arrival_rate, window_ratio, test_rp_range, tol, device, eigensolver)
        t0 = time.perf_counter()
        datetime = pd.to_datetime(pd.Series(np.asarray(datetime))).to_numpy()
        self.ids, self._rank, self._hour, _ = rank_and_hour(event_id, datetime)
        self.host_sort_ms = 1e3 * (time.perf_counter() - t0)
        cols = []
        for name, col in (("precip-excess", precip_excess), ("precip-cum", precip_cum), ("inflow", inflow)):
            col = np.ascontiguousarray(col, dtype=np.float64)
            if col.shape != self._rank.shape:
                raise ValueError(f"column {name!r} has shape {col.shape}, event_id has {self._rank.shape}")
            bad = int(np.count_nonzero(~np.isfinite(col)))
            if bad:
                raise ValueError(f"values must be finite: column {name!r} holds {bad} non-finite values")
            cols.append(col)
        self._cols = cols
        self.n_events = int(self.ids.size)
        self.n_hours = int(self._hour.max()) + 1
        check_shape(self.n_events, self.n_hours)
        self._event_max = None
        self._scores = {}
        self.diverse_order_ = None
        self.diverse_distance_ = None
        self.last_timings_ms: dict[str, float] = {}

    def _set_parameters(self, arrival_rate, window_ratio, test_rp_range, tol, device, eigensolver):
        if int(arrival_rate) != arrival_rate or arrival_rate < 1:
            raise ValueError("arrival_rate must be a positive integer")
        if eigensolver not in ("host", "device"):
            raise ValueError(f"eigensolver must be 'host' or 'device', not {eigensolver!r}")
        self.arrival_rate = int(arrival_rate)
        self.window_ratio = window_ratio
        self.tol = tol
        self.test_rp_range = test_rp_range or [5, 2000]
        self.device = device
        self.eigensolver = eigensolver
        self.last_eig_sweeps = None

    # ---- other constructors -----------------------------------------------------------------------------------------------------------
    @classmethod
    def from_frame(cls, df, **kwargs) -> "EventSelector":
        """From a long frame with the reference's columns ``event_id, datetime, precip-excess, precip-cum, inflow``."""
        missing = [c for c in COLUMNS if c not in df.columns]
        if missing:
            raise ValueError(f"the frame lacks the columns {missing}")
        return cls(df["event_id"].to_numpy(), df["datetime"].to_numpy(), df["precip-excess"].to_numpy(), df["precip-cum"].to_numpy(),
                   df["inflow"].to_numpy(), **kwargs)

    @classmethod
    def from_parquet(cls, path, **kwargs) -> "EventSelector":
        """``EventSelection(pq_file, ...)`` (event_selection.py:31)."""
        return cls.from_frame(pd.read_parquet(path, columns=list(COLUMNS)), **kwargs)

    @classmethod
    def from_event_max(cls, frame, arrival_rate: int = 10, window_ratio: float = 0.2, test_rp_range=None, tol: float = 0.15) -> "EventSelector":
        """Around a given ``event_max`` table (columns ``event_id, precip-cum, inflow, RP_precip-cum, RP_inflow``): ``select_aep`` and
        ``select_test`` work, nothing touches the device, the methods that need the long frame raise."""
        self = cls.__new__(cls)
        DeviceHandle.__init__(self)
        self._set_parameters(arrival_rate, window_ratio, test_rp_range, tol, 0, "host")
        need = ["event_id", "precip-cum", "inflow", "RP_precip-cum", "RP_inflow"]
        missing = [c for c in need if c not in frame.columns]
        if missing:
            raise ValueError(f"the table lacks the columns {missing}")
        self._event_max = frame[need].reset_index(drop=True).copy()
        self.ids = self._event_max["event_id"].to_numpy()
        self.n_events, self.n_hours = int(self.ids.size), 0
        self._cols = None
        self._scores = {}
        self.diverse_order_ = self.diverse_distance_ = None
        self.last_timings_ms = {}
        return self

    # ---- device state -----------------------------------------------------------------------------------------------------------------
    def _create(self):
        """The columns go up in their original row order and are pivoted on the device."""
        if self._cols is None:
            raise RuntimeError("this EventSelector was built from an event_max table: it has no long frame")
        t0 = time.perf_counter()
        check(_lib.load().gprx_ev_create(self.device, self._rank.size, self.n_events, self.n_hours, ptr(self._rank), ptr(self._hour), ptr(self._cols[0]),
                                         ptr(self._cols[1]), ptr(self._cols[2]), C.byref(self._h)))
        self.upload_pivot_wall_ms = 1e3 * (time.perf_counter() - t0)

    def _released(self):
        """``close()`` releases the device memory; ``event_max`` stays, the scores (whose device copy the selection reads) are computed
        again when they are next needed."""
        self._scores = {}

    def stage_timings_ms(self) -> dict[str, float]:
        """Device milliseconds of the last call of each stage (``gprx_ev_timings``)."""
        out = np.zeros(8)
        check(_lib.load().gprx_ev_timings(self.handle, out.ctypes.data_as(C.POINTER(C.c_double))))
        self.last_timings_ms = dict(zip(TIMING_NAMES, (float(v) for v in out)))
        return self.last_timings_ms

    # ---- event_selection.py:34-67 -------------------------------------------------------------------------------------------------------
    @property
    def event_max(self) -> pd.DataFrame:
        """The reference's ``event_max``: one row per event in id order, the maxima of ``precip-cum`` and ``inflow`` over the event's own
        rows and their return periods."""
        if self._event_max is None:
            lib, E = _lib.load(), self.n_events
            mx_pc, mx_q, rp_pc, rp_q = np.empty(E), np.empty(E), np.empty(E), np.empty(E)
            knots = np.zeros(2, dtype=np.int64)
            if -(-E // self.arrival_rate) < 2:
                raise ValueError(f"the return-period function needs at least two distinct block maxima: {E} events in blocks of "
                                 f"{self.arrival_rate} give one block")
            check(lib.gprx_ev_maxima(self.handle, ptr(mx_pc), ptr(mx_q), None))
            check(lib.gprx_ev_return_periods(self.handle, self.arrival_rate, ptr(rp_pc), ptr(rp_q), ptr(knots)))
            self.n_knots_ = (int(knots[0]), int(knots[1]))
            self._event_max = pd.DataFrame({"event_id": self.ids, "precip-cum": mx_pc, "inflow": mx_q, "RP_precip-cum": rp_pc, "RP_inflow": rp_q})
        return self._event_max

    def return_period(self, which: str, values) -> np.ndarray:
        """The fitted return-period function of ``"precip-cum"`` or ``"inflow"`` at arbitrary values, extrapolating below the lowest and
        above the highest knot as scipy's ``interp1d(..., fill_value="extrapolate")`` does."""
        if which not in ("precip-cum", "inflow"):
            raise ValueError("which must be 'precip-cum' or 'inflow'")
        self.event_max  # (fits the functions)
        values = np.ascontiguousarray(values, dtype=np.float64)
        out = np.empty(values.size)
        if values.size:
            check(_lib.load().gprx_ev_rp_eval(self.handle, int(which == "inflow"), ptr(values.reshape(-1)), values.size, ptr(out)))
        return out.reshape(values.shape)

    # ---- event_selection.py:69-146 ------------------------------------------------------------------------------------------------------
    def _is_close(self, a, b) -> bool:
        with np.errstate(all="ignore"):
            return bool(abs(a - b) / max(a, b) < self.tol)

    def select_aep(self, target_rps) -> pd.DataFrame:
        """The three "Max" events (largest return period of either variable, largest joint normalised magnitude) and, per target
        return period and variable, the event of the window ``rp (1 -+ window_ratio)`` nearest to ``(rp, rp)`` in joint log distance that
        is not yet taken and not close (``tol``) to a taken one in both return periods.  An event with a negative (extrapolated)
        return period has a NaN log distance and sorts last."""
        em = self.event_max
        pc, q, rp_pc, rp_q = em["precip-cum"], em["inflow"], em["RP_precip-cum"], em["RP_inflow"]
        joint = (pc - pc.min()) / (pc.max() - pc.min()) + (q - q.min()) / (q.max() - q.min())
        rows, sets, taken = [], [], set()

        def take(label, row):
            rows.append(row)
            sets.append(label)
            taken.add(row["event_id"])

        for idx in (rp_pc.idxmax(), rp_q.idxmax(), joint.idxmax()):
            row = em.loc[idx]
            if row["event_id"] not in taken:
                take("Max", row)
        for rp in target_rps:
            lo, hi = rp * (1 - self.window_ratio), rp * (1 + self.window_ratio)
            for field in (rp_pc, rp_q):
                window = em[field.between(lo, hi)]
                if window.empty:
                    continue
                with np.errstate(all="ignore"):
                    log_dist = np.sqrt(np.log10(window["RP_precip-cum"] / rp) ** 2 + np.log10(window["RP_inflow"] / rp) ** 2)
                for idx in log_dist.sort_values().index:
                    row = em.loc[idx]
                    if row["event_id"] in taken:
                        continue
                    if any(self._is_close(row["RP_precip-cum"], x["RP_precip-cum"]) and self._is_close(row["RP_inflow"], x["RP_inflow"]) for x in rows):
                        continue
                    take("AEP", row)
                    break
        df = pd.DataFrame(rows).copy()
        df["Set"] = sets
        df["Type"] = "Train"
        return df

    # ---- event_selection.py:148-185 -----------------------------------------------------------------------------------------------------
    def _pca_components(self, which: int, k: int) -> np.ndarray:
        """(k, H) components of pivot ``which`` with scikit-learn's signs; the eigenvalue gaps of the leading k + 1 are kept."""
        lib, H, E = _lib.load(), self.n_hours, self.n_events
        mean, cov = np.empty(H), np.empty((H, H))
        check(lib.gprx_ev_cov(self.handle, which, ptr(mean), ptr(cov)))
        if self.eigensolver == "device":
            lam, v, sweeps = np.empty(H), np.empty((H, H)), C.c_int()
            check(lib.gprx_ev_eigh(self.handle, ptr(lam), ptr(v), C.byref(sweeps)))
            self.last_eig_sweeps = sweeps.value
        else:
            t0 = time.perf_counter()
            lam, v = np.linalg.eigh(cov)
            self.host_eigh_ms = getattr(self, "host_eigh_ms", 0.0) + 1e3 * (time.perf_counter() - t0)
        top = np.argsort(lam, kind="stable")[::-1][:k]
        self.explained_variance_[which] = lam[top] / (E - 1)
        return sign_convention(v[:, top].T)

    def diverse_scores(self, n_components: int = 5) -> np.ndarray:
        """The standardised ``(E, 2 n_components)`` score matrix of event_selection.py:157-167: the leading principal-component scores of
        the zero-filled precip-excess and inflow pivots side by side, every column scaled to zero mean and unit population variance."""
        k = int(n_components)
        if k < 1 or k > MAX_COMPONENTS:
            raise ValueError(f"need 1 <= n_components <= {MAX_COMPONENTS}")
        if self._cols is None:
            raise RuntimeError("this EventSelector was built from an event_max table: it has no long frame")
        if k > min(self.n_events, self.n_hours):
            raise ValueError(f"n_components = {k} exceeds min(E, H) = min({self.n_events}, {self.n_hours})")
        if self.n_events < 2:
            raise ValueError("the PCA needs at least two events")
        if k not in self._scores:
            lib = _lib.load()
            self.explained_variance_ = {}
            self.host_eigh_ms = 0.0
            comps = [np.ascontiguousarray(self._pca_components(which, k)) for which in (0, 1)]
            for which in (0, 1):
                check(lib.gprx_ev_scores(self.handle, which, k, ptr(comps[which])))
            out = np.empty((self.n_events, 2 * k))
            check(lib.gprx_ev_standardise(self.handle, ptr(out)))
            self._scores = {k: out}  # (the device holds the matrix of one k)
        return self._scores[k]

    def select_diverse(self, selected_event_ids, num_to_select: int, n_components: int = 5) -> pd.DataFrame:
        """``num_to_select`` further events, each the one farthest (in the standardised score space) from everything selected so far;
        the rows of ``event_max`` in id order with ``Set="Diverse"``.  ``diverse_order_``: the ids in pick order; ``diverse_distance_``:
        the distance of each pick to its nearest selected event when it was picked."""
        selected = list(selected_event_ids)
        if not selected:
            raise ValueError("the initial selected set must be non-empty")
        pos = np.searchsorted(self.ids, np.asarray(selected))
        pos = np.minimum(pos, self.n_events - 1)
        if np.any(self.ids[pos] != np.asarray(selected)):
            raise ValueError("a selected event id is not among the events")
        rows = np.unique(pos).astype(np.int32)
        num = int(num_to_select)
        if num > self.n_events - rows.size:
            raise ValueError(f"num_to_select = {num} exceeds the number of candidates ({self.n_events - rows.size})")
        if num < 1:
            raise ValueError("num_to_select must be at least 1")
        self.diverse_scores(n_components)
        picks, dist = np.empty(num, dtype=np.int32), np.empty(num)
        check(_lib.load().gprx_ev_farthest(self.handle, None, self.n_events, 2 * int(n_components), ptr(rows), rows.size, num, ptr(picks), ptr(dist)))
        self.diverse_order_ = self.ids[picks]
        self.diverse_distance_ = dist
        em = self.event_max
        df = em[em["event_id"].isin(self.diverse_order_)].copy()
        df["Set"] = "Diverse"
        df["Type"] = "Train"
        return df

    # ---- event_selection.py:187-237 -----------------------------------------------------------------------------------------------------
    def select_test(self, test_rp_range, n_test_storms: int, excluded_ids=None) -> pd.DataFrame:
        """Test events from logarithmic return-period bins of either variable inside ``test_rp_range`` (one seeded draw per non-empty
        bin), topped up by a seeded sample of the remaining eligible events; ``pandas.DataFrame.sample`` is the sampler, with the
        reference's seeds."""
        rp_min, rp_max = test_rp_range
        n_bins = n_test_storms // 2
        rng = np.random.default_rng(seed=42)
        em = self.event_max
        eligible = em[em["RP_precip-cum"].between(rp_min, rp_max) & em["RP_inflow"].between(rp_min, rp_max)].copy()
        if excluded_ids:
            eligible = eligible[~eligible["event_id"].isin(excluded_ids)]
        if eligible.empty:
            raise ValueError("No eligible storms found in the specified test RP range.")
        edges = np.logspace(np.log10(rp_min), np.log10(rp_max), n_bins + 1)

        def one_per_bin(column):
            chosen = set()
            for i in range(n_bins):
                in_bin = eligible[(eligible[column] >= edges[i]) & (eligible[column] <= edges[i + 1])]
                if not in_bin.empty:
                    chosen.add(in_bin.sample(1, random_state=rng.integers(0, 10000)).iloc[0]["event_id"])
            return chosen

        test_ids = one_per_bin("RP_precip-cum") | one_per_bin("RP_inflow")
        if len(test_ids) < n_test_storms:
            rest = eligible[~eligible["event_id"].isin(test_ids)]
            test_ids.update(rest.sample(n=n_test_storms - len(test_ids), random_state=42)["event_id"].tolist())
        df = em[em["event_id"].isin(test_ids)].copy()
        df["Set"] = "Test"
        df["Type"] = "Test"
        return df

    # ---- event_selection.py:239-257 -----------------------------------------------------------------------------------------------------
    def run_selection(self, n_train_storms: int, n_test_storms: int, target_rps):
        """``(selected, event_max)`` as ``EventSelection.run_selection``."""
        aep = self.select_aep(target_rps)
        diverse = self.select_diverse(aep["event_id"].tolist(), n_train_storms - len(aep))
        train = pd.concat([aep, diverse], ignore_index=True)
        train["Type"] = "Train"
        test = self.select_test(self.test_rp_range, n_test_storms, train["event_id"].tolist())
        return pd.concat([train, test], ignore_index=True), self.event_max
