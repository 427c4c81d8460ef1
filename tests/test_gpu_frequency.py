"""The depth-frequency maps on the GPU (gpras_amd.frequency, csrc/frequency.h) against the numpy mirror (frequency_numpy.py): the rate bit
for bit and the NaN counts exactly at every shape where the kernel takes another path, every kind of column content, the counts against
``gprx_pca_member_stats_dev``, the invariances (member order, a weight-0 event, position and neighbours, repetition), the inversion, a
catalogue saved and continued, ``evaluate(frequency=...)`` end to end, and the refusals of the C ABI.  Every comparison is an equality: a NaN
must stand where the mirror has one, every other value must have the mirror's bits."""

import ctypes as C

import numpy as np
import pytest

import frequency_numpy as fq
import sweep_numpy as sn
from gpras_amd._lib import GPRX_EINVAL, GPRX_OK, DeviceBuffer, ptr
from gpras_amd.synth import make_regression

pytestmark = pytest.mark.gpu

KINDS = 10
# (members of the events, levels, cells): every member count, level count and cell count of the kernel's branches -- one lane, one wave short
# of and past a tile of 64 cells, several workgroups; the 64-level and the 256-level instance and their border; members below, at and past
# the four waves' stride, and the most a 16-bit bin holds
CASES = (
    ((1, 2, 63), 1, 1),
    ((2, 64, 65), 2, 63),
    ((63, 64, 1), 8, 64),
    ((65, 256, 2, 257), 9, 65),
    ((256, 257, 64), 63, 257),
    ((257, 1, 4096), 64, 1000),
    ((4096, 65, 63), 65, 64),
    ((64, 2, 256, 1, 65), 255, 1000),
    ((4096, 63, 257), 256, 65),
    ((1, 256, 64), 256, 257),
    ((2, 4096, 3), 1, 1000),
)


def _projector(state):
    from gpras_amd.preprocess import EOFProjector

    return EOFProjector(state["dry"], state["elevations"], state["input_mean"], state["weights"], state["eofs"], state["x_mean"], state["x_std"], state["hp"])


def _bare_projector(cells):
    state, *_ = sn.make_case(cells, 1, [1], "wse", seed=1)
    return _projector(state)


class _Bare:
    """What ``PeakEnsemble`` reads of a ``GPRAS`` when only the projector side is exercised."""

    def __init__(self, k):
        self.models = [None] * k


def _same(got, want):
    """Equal bits, a NaN exactly where the other has one."""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype != np.float64:
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]))


def _levels(n):
    """``d_0 = 0.0`` and quarter steps: the integers among them meet the integer-valued peaks."""
    return np.arange(n) * 0.25


def _contents(members, cells, levels, shift, seed):
    """``peak (S, cells)``: column c holds the content of kind ``(c + shift) % KINDS``."""
    rng = np.random.default_rng(seed)
    S, top = members, float(levels[-1])
    peak = rng.uniform(-0.5, top + 0.5, size=(S, cells))
    pick = rng.integers(0, S, size=cells)
    for c in range(cells):
        kind = (c + shift) % KINDS
        col = peak[:, c]
        if kind == 1:  # dry everywhere
            col[:] = 0.0
        elif kind == 2:  # +0 and -0 mixed among positive depths: neither exceeds d_0 = 0.0
            col[:] = np.where(rng.uniform(size=S) < 0.4, 0.0, np.abs(col))
            col[rng.uniform(size=S) < 0.3] = -0.0
            col[pick[c]] = -0.0 if c % 2 else 0.0
        elif kind == 3:  # members equal to a level: the strict compare must not count them there
            col[rng.uniform(size=S) < 0.5] = levels[rng.integers(0, levels.size)]
            col[pick[c]] = levels[rng.integers(0, levels.size)]
        elif kind == 4:  # all above the top level
            col[:] = top + rng.uniform(0.1, 2.0, size=S)
        elif kind == 5:  # all below the bottom level
            col[:] = float(levels[0]) - rng.uniform(0.1, 2.0, size=S)
        elif kind == 6:  # infinite members
            col[pick[c]] = np.inf
            col[(pick[c] + 1) % S] = -np.inf
        elif kind == 7:  # one NaN member
            col[pick[c]] = np.nan
        elif kind == 8:  # all members NaN
            col[:] = np.nan
        elif kind == 9:  # integer-valued peaks with many ties
            col[:] = np.round(rng.uniform(0.0, 5.0, size=S))
    return peak


def _weights(n, seed):
    return np.random.default_rng(seed).uniform(0.001, 0.5, size=n).tolist()


def _run(proj, levels, peaks, weights):
    """``(rate, nan_members)`` of the catalogue on the device, a fresh accumulator."""
    from gpras_amd.frequency import FrequencyMaps

    with FrequencyMaps(proj, levels) as fm:
        for peak, w in zip(peaks, weights):
            fm.add_peaks(peak, peak.shape[0], w)
        assert fm.n_events == len(peaks) and fm.weights == [float(w) for w in weights] and fm.last_device_ms > 0.0
        return fm.rate(), fm.nan_members()


@pytest.mark.parametrize("members,n_levels,cells", CASES)
def test_accumulate_against_the_mirror(lib, members, n_levels, cells):
    proj = _bare_projector(cells)
    try:
        levels = _levels(n_levels)
        peaks = [_contents(s, cells, levels, shift=3 * e, seed=1000 * n_levels + 10 * e + cells) for e, s in enumerate(members)]
        weights = _weights(len(members), seed=n_levels)
        want_rate, want_nan = fq.accumulate(peaks, weights, levels)
        rate, nan_members = _run(proj, levels, peaks, weights)
        assert nan_members.dtype == np.int32 and np.array_equal(nan_members, want_nan)
        assert _same(rate, want_rate) and not np.isnan(rate).any()
        assert np.all(np.diff(rate, axis=0) <= 0.0) and not np.signbit(rate).any()
    finally:
        proj.close()


@pytest.mark.parametrize("members", [3, 64, 257])
def test_column_contents_by_kind(lib, members):
    """One event of weight 1 over columns of every kind: the mirror's bits, and what each kind must show whatever the mirror says."""
    cells, levels = 4 * KINDS, _levels(9)
    proj = _bare_projector(cells)
    try:
        peak = _contents(members, cells, levels, shift=0, seed=members)
        rate, nan_members = _run(proj, levels, [peak], [1.0])
        want_rate, want_nan = fq.accumulate([peak], [1.0], levels)
        assert _same(rate, want_rate) and np.array_equal(nan_members, want_nan)
        kind = np.arange(cells) % KINDS
        assert not rate[:, (kind == 1) | (kind == 5) | (kind == 8)].any()  # dry, below the bottom, all NaN: nothing exceeds
        assert np.all(rate[0, kind == 2] < 1.0)  # the zeros of either sign are not above d_0 = 0.0
        assert np.all(rate[:, kind == 4] == 1.0)
        assert np.array_equal(nan_members[kind == 7], np.ones(4, dtype=np.int32)) and np.array_equal(nan_members[kind == 8], np.full(4, members, dtype=np.int32))
        assert not nan_members[(kind != 7) & (kind != 8)].any()
        ints = peak[:, kind == 9]  # integer peaks against the integer levels 0, 1, 2: exact counts over S
        for value in (0, 1, 2):
            assert np.array_equal(rate[4 * value, kind == 9], (ints > value).sum(axis=0) / np.float64(members))
    finally:
        proj.close()


def test_counts_against_the_member_statistics(lib):
    """One event at weight 1 with S a power of two: ``rate S`` is exactly the exceedance count of ``gprx_pca_member_stats_dev``."""
    from gpras_amd.ensemble import PeakEnsemble

    members, cells, levels = 64, 300, _levels(20)
    proj = _bare_projector(cells)
    try:
        peak = _contents(members, cells, levels, shift=0, seed=7)
        rate, _ = _run(proj, levels, [peak], [1.0])
        sel = np.array([0, 1, 4, 5, 8, 12, 18, 19])
        dpeak = DeviceBuffer.from_array(peak)
        try:
            exceed = PeakEnsemble(_Bare(1), proj).member_stats(dpeak, members, thresholds=levels[sel])["exceed"]
        finally:
            dpeak.free()
        counts = rate[sel] * members
        assert np.array_equal(counts, np.round(counts)) and np.array_equal(counts.astype(np.int32), exceed)
    finally:
        proj.close()


def test_invariances(lib):
    """Permuting an event's members, inserting an event of weight 0, moving columns to another position among other neighbours in a grid of
    another size, and running twice all leave a cell's bits alone."""
    levels, members = _levels(33), (65, 4, 256)
    small, large = _bare_projector(257), _bare_projector(1000)
    try:
        peaks = [_contents(s, 257, levels, shift=e, seed=40 + e) for e, s in enumerate(members)]
        weights = _weights(3, seed=9)
        rate, nan_members = _run(small, levels, peaks, weights)
        again = _run(small, levels, peaks, weights)
        assert _same(again[0], rate) and np.array_equal(again[1], nan_members)
        shuffled = [p[np.random.default_rng(e).permutation(p.shape[0])] for e, p in enumerate(peaks)]
        got = _run(small, levels, shuffled, weights)
        assert _same(got[0], rate) and np.array_equal(got[1], nan_members)
        extra = _contents(7, 257, levels, shift=5, seed=77)
        got = _run(small, levels, peaks[:1] + [extra] + peaks[1:], weights[:1] + [0.0] + weights[1:])
        assert _same(got[0], rate)
        assert np.array_equal(got[1], nan_members + np.isnan(extra).sum(axis=0))  # its NaN members are still counted
        for off in (0, 37, 1000 - 257):
            moved = [_contents(s, 1000, levels, shift=e + 4, seed=90 + e) for e, s in enumerate(members)]
            for m, p in zip(moved, peaks):
                m[:, off:off + 257] = p
            got = _run(large, levels, moved, weights)
            assert _same(np.ascontiguousarray(got[0][:, off:off + 257]), rate) and np.array_equal(got[1][off:off + 257], nan_members), off
    finally:
        small.close()
        large.close()


@pytest.mark.parametrize("n_levels", [1, 2, 40, 256])
def test_invert_against_the_mirror(lib, n_levels):
    from gpras_amd.frequency import FrequencyMaps

    cells, levels = 333, _levels(n_levels)
    proj = _bare_projector(cells)
    try:
        members = (3, 64, 257, 1)
        peaks = [_contents(s, cells, levels, shift=e, seed=500 + e) for e, s in enumerate(members)]
        # (the kinds move one column per event: the flagged cells are those a NaN member ever met)
        with FrequencyMaps(proj, levels) as fm:
            for peak, w in zip(peaks, _weights(4, seed=3)):
                fm.add_peaks(peak, peak.shape[0], w)
            rate, nan_members = fm.rate(), fm.nan_members()
            assert (nan_members > 0).any() and (nan_members == 0).any()
            positive = rate[rate > 0.0]
            stored = np.random.default_rng(1).choice(positive, size=13)  # targets equal to stored rates
            sixteen = np.concatenate([stored, [rate[0].max() * 2.0, rate[0].max() + 1.0, positive.min() / 2.0]])
            for aep in (stored[:1], sixteen, [rate[0].max() * 2.0], [positive.min() / 2.0]):
                for interp in fq.INTERPS:
                    got = fm.depth_at(aep, interp=interp)
                    depth, bracket = fq.invert(rate, nan_members, levels, aep, interp)
                    assert got.bracket.dtype == np.int32 and np.array_equal(got.bracket, bracket), (interp, len(aep))
                    assert _same(got.depth, depth), (interp, len(aep))
                    assert got.interp == interp and np.array_equal(got.aep, np.asarray(aep, dtype=np.float64)) and np.array_equal(got.levels, levels)
                    assert np.array_equal(got.resolved(), (bracket > 0) & (bracket < n_levels))
                    flagged = nan_members > 0
                    assert np.isnan(got.depth[:, flagged]).all() and (got.bracket[:, flagged] == -1).all() and not np.isnan(got.depth[:, ~flagged]).any()
            above = fm.depth_at([rate[0].max() * 2.0]).depth[0, nan_members == 0]
            assert np.all(above == -np.inf)
            if n_levels > 2:
                assert fm.depth_at(sixteen).resolved().any()
    finally:
        proj.close()


def test_save_and_load_in_the_middle_of_a_catalogue(lib, tmp_path):
    from gpras_amd.frequency import FrequencyMaps

    cells, levels = 130, _levels(17)
    proj = _bare_projector(cells)
    try:
        members = (5, 64, 1, 300)
        peaks = [_contents(s, cells, levels, shift=e, seed=700 + e) for e, s in enumerate(members)]
        weights = _weights(4, seed=5)
        rate, nan_members = _run(proj, levels, peaks, weights)
        path = tmp_path / "maps.npz"
        with FrequencyMaps(proj, levels) as first:
            for peak, w in zip(peaks[:2], weights[:2]):
                first.add_peaks(peak, peak.shape[0], w)
            first.to_file(path)
        with FrequencyMaps.from_file(path, proj) as second:
            assert second.n_events == 2 and second.weights == weights[:2] and np.array_equal(second.levels, levels)
            for peak, w in zip(peaks[2:], weights[2:]):
                resident = DeviceBuffer.from_array(peak)  # (a resident block stays the caller's)
                try:
                    second.add_peaks(resident, peak.shape[0], w)
                finally:
                    resident.free()
            assert second.n_events == 4 and second.weights == weights
            assert _same(second.rate(), rate) and np.array_equal(second.nan_members(), nan_members)
        other = _bare_projector(cells + 1)
        try:
            with pytest.raises(ValueError):
                FrequencyMaps.from_file(path, other)
        finally:
            other.close()
    finally:
        proj.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
FIELDS = ("p_exceed", "peak_mean", "peak_std", "peak_quantiles", "wet_area", "exceed_counts", "thresholds", "quantiles")


def test_evaluate_with_frequency(lib):
    """A small fitted sparse GPRAS (N = 300, M = 16, K = 3) over 300 cells, three events of 5, 7 and 9 rows, 64 members."""
    from gpras_amd.ensemble import PeakEnsemble
    from gpras_amd.frequency import FrequencyMaps
    from gpras_amd.gpr import GPRAS

    k, cells, d, members = 3, 300, 4, 64
    ranges = [(0, 5), (5, 12), (12, 21)]
    state, *_ = sn.make_case(cells, k, [5], "wse", seed=21)
    x, y, xs = make_regression(300, d, n_outputs=k, n_test=21, config=9)
    gpr = GPRAS("RBF")
    gpr.fit(x, y, 16, "kmeans", "adam", max_iter=5)
    rng = np.random.default_rng(5)
    normals = [rng.standard_normal((k, members, hi - lo)) for lo, hi in ranges]
    weights = [0.1, 0.02, 0.004]
    levels = np.linspace(0.0, 2.0, 21)
    proj = _projector(state)
    try:
        ens = PeakEnsemble(gpr, proj)
        kw = dict(thresholds=(0.5, 1.0), quantiles=(0.05, 0.5, 0.95), normals=normals)
        plain = ens.evaluate(xs, ranges, members, **kw)
        assert "frequency" not in plain.last_timings_ms and "device_frequency" not in plain.last_timings_ms
        with FrequencyMaps(proj, levels) as fm:
            fed = ens.evaluate(xs, ranges, members, **kw, frequency=fm, weights=weights)
            assert {"frequency", "device_frequency"} <= set(fed.last_timings_ms) and fed.last_timings_ms["device_frequency"] > 0.0
            for name in FIELDS:
                assert np.array_equal(getattr(plain, name), getattr(fed, name)), name
            assert plain.ranges == fed.ranges and plain.members == fed.members and plain.route == fed.route
            peaks = []
            for e, (lo, hi) in enumerate(ranges):
                mean_dev, lc_dev, _ = ens.joint_dev(xs[lo:hi])
                scores_dev = peak_dev = None
                try:
                    scores_dev = ens.scores_dev(mean_dev, lc_dev, normals[e], members, hi - lo)
                    peak_dev = ens.member_peaks_dev(scores_dev, members, hi - lo)
                    peaks.append(peak_dev.to_array((members, cells)))
                finally:
                    for buf in (mean_dev, lc_dev, scores_dev, peak_dev):
                        if buf is not None:
                            buf.free()
            want_rate, want_nan = fq.accumulate(peaks, weights, levels)
            assert fm.n_events == 3 and fm.weights == weights
            assert _same(fm.rate(), want_rate) and np.array_equal(fm.nan_members(), want_nan) and want_rate.any()
            got = fm.depth_at([0.05, 0.01])
            depth, bracket = fq.invert(want_rate, want_nan, levels, [0.05, 0.01])
            assert _same(got.depth, depth) and np.array_equal(got.bracket, bracket)
        # the deterministic peaks of the mean field, from the host and resident
        field = proj.reverse_transform(gpr.predict(xs)[0])
        det = [np.max(field[lo:hi], axis=0)[None, :] for lo, hi in ranges]
        want_rate, want_nan = fq.accumulate(det, weights, levels)
        dfield = DeviceBuffer.from_array(field)
        try:
            for source in (field, dfield):
                with FrequencyMaps(proj, levels) as fm:
                    fm.add_field(source, ranges, weights)
                    assert fm.n_events == 3 and _same(fm.rate(), want_rate) and np.array_equal(fm.nan_members(), want_nan)
        finally:
            dfield.free()
    finally:
        proj.close()


# ---- the C ABI's refusals -------------------------------------------------------------------------------------------------------------------
def test_abi_refusals(lib):
    cells, n_lev = 40, 3
    proj = _bare_projector(cells)
    levels, aep = np.array([0.0, 0.5, 1.0]), np.array([0.5])
    state = np.zeros(n_lev * cells + cells // 2)
    state[: n_lev * cells] = 0.75
    peak, block, out = DeviceBuffer.from_array(np.ones((4, cells))), DeviceBuffer.from_array(state), DeviceBuffer.from_array(np.full(2 * cells, 7.0))
    ph = proj.handle

    def accumulate(members=4, n_levels=n_lev, lv=levels, weight=1.0, peak_ptr=peak.ptr, rate=block.ptr, nan=block.at(n_lev * cells)):
        return lib.gprx_pca_freq_accumulate_dev(ph, peak_ptr, members, n_levels, None if lv is None else ptr(lv), weight, rate, nan)

    def invert(n_levels=n_lev, lv=levels, n_aep=1, p=aep, interp=0, rate=block.ptr, nan=block.at(n_lev * cells), depth=out.ptr, bracket=out.at(cells)):
        return lib.gprx_pca_freq_invert_dev(ph, rate, nan, n_levels, None if lv is None else ptr(lv), n_aep, None if p is None else ptr(p), interp, depth, bracket)

    def refused(rc, word):
        message = lib.gprx_pca_last_error(ph) or b""
        return rc == GPRX_EINVAL and word in message

    try:
        assert refused(accumulate(members=0), b"members") and refused(accumulate(members=4097), b"members")
        assert refused(accumulate(n_levels=0), b"n_levels") and refused(accumulate(n_levels=257, lv=np.arange(257.0)), b"n_levels")
        assert refused(accumulate(lv=np.array([0.0, 1.0, 0.5])), b"increasing") and refused(accumulate(lv=np.array([0.0, 0.5, 0.5])), b"increasing")
        assert refused(accumulate(lv=np.array([0.0, 0.5, np.inf])), b"finite") and refused(accumulate(lv=np.array([0.0, np.nan, 1.0])), b"finite")
        assert refused(accumulate(lv=None), b"null")
        for weight in (-1.0, np.nan, np.inf, -np.inf):
            assert refused(accumulate(weight=weight), b"weight")
        assert refused(accumulate(peak_ptr=None), b"null") and refused(accumulate(rate=None), b"null") and refused(accumulate(nan=None), b"null")
        assert lib.gprx_pca_freq_accumulate_dev(None, peak.ptr, 4, n_lev, ptr(levels), 1.0, block.ptr, block.at(n_lev * cells)) == GPRX_EINVAL
        assert refused(invert(n_aep=0), b"targets") and refused(invert(n_aep=17, p=np.full(17, 0.5)), b"targets") and refused(invert(p=None), b"targets")
        for bad in (0.0, -0.5, np.nan, np.inf):
            assert refused(invert(p=np.array([bad])), b"targets")
        assert refused(invert(interp=2), b"interp") and refused(invert(interp=-1), b"interp")
        assert refused(invert(n_levels=0), b"n_levels") and refused(invert(lv=np.array([0.0, 1.0, 0.5])), b"increasing") and refused(invert(lv=None), b"null")
        for name in ("rate", "nan", "depth", "bracket"):
            assert refused(invert(**{name: None}), b"null"), name
        ms = C.c_double()
        assert lib.gprx_pca_freq_ms(ph, None) == GPRX_EINVAL and lib.gprx_pca_freq_ms(None, C.byref(ms)) == GPRX_EINVAL
        # nothing was written: the state and the output block hold what they held
        assert np.array_equal(block.to_array(state.shape), state) and np.array_equal(out.to_array((2 * cells,)), np.full(2 * cells, 7.0))
        # the handle is still usable: all members 1.0 exceed the levels 0.0 and 0.5, not 1.0
        assert accumulate(weight=0.5) == GPRX_OK and lib.gprx_pca_freq_ms(ph, C.byref(ms)) == GPRX_OK and ms.value > 0.0
        rate = block.to_array((n_lev, cells))
        assert np.all(rate[:2] == 1.25) and np.all(rate[2] == 0.75)
        assert invert(p=np.array([1.0])) == GPRX_OK
        assert np.all(out.to_array((cells,)) == 0.75)  # between the levels 0.5 (rate 1.25) and 1.0 (rate 0.75): halfway
    finally:
        for b in (peak, block, out):
            b.free()
        proj.close()
