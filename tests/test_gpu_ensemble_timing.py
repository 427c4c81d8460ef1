"""The event timing of a peak ensemble on the GPU (gpras_amd.ensemble.member_timing_dev / timing_stats / evaluate(timing=True), csrc/timing.h)
against the numpy mirror (ensemble_timing_numpy.py).  The maps are integers and the peak is the peaks kernel's own, so every assertion is
an equality.  The shapes are those of ``PEAK_CASES`` (test_gpu_ensemble.py): a partial last workgroup, both ``KMAX``, ``K = KMAX`` and
``K = KMAX + 1``, an event that ends on, before and after a 32-row block of the walk, a third block, members not divisible by the group."""

import ctypes as C

import numpy as np
import pytest

import ensemble_numpy as en
import ensemble_timing_numpy as et
import sweep_numpy as sn
from gpras_amd._lib import GPRX_EINVAL, GPRX_OK, DeviceBuffer, ptr
from test_gpu_ensemble import PEAK_CASES, _ensemble, _index, _peak_case, _projector
from test_gpu_ensemble import fitted  # noqa: F401  (the fixture of test_pipeline_peak_ensemble)

pytestmark = pytest.mark.gpu

GROUPS = [0, *range(1, 17), 64]
LARGER = ("k16_depth", "k17_velocity", "k64_depth")  # (257, 16, 32, 5), (300, 17, 33, 17), (300, 64, 65, 5)
_CASES = {}


def _case(name):
    """The case's state and scores, the mirror's fields and its eight thresholds -- the 0.2, 0.5, 0.9 and 0.999 lower quantiles of the finite
    field values, 0.0, one field value verbatim (the strict compare), +inf and -inf -- computed once and shared."""
    if name not in _CASES:
        state, scores, members, rows = _peak_case(name)
        y = en.member_fields(state, scores)
        finite = y[np.isfinite(y)]
        thr = np.array([*np.quantile(finite, (0.2, 0.5, 0.9, 0.999), method="lower"), 0.0, y[members // 2, rows // 2, y.shape[2] // 3], np.inf, -np.inf])
        for a in (y, thr):
            a.setflags(write=False)
        _CASES[name] = (state, scores, members, rows, y, thr)
    return _CASES[name]


def _download(ens, bufs, members, n_maps):
    peak_dev, timing_dev = bufs
    try:
        return peak_dev.to_array((members, ens.projector.n_cells)), ens.timing_to_array(timing_dev, members, n_maps)
    finally:
        peak_dev.free()
        timing_dev.free()


def _upload_i32(a) -> DeviceBuffer:
    flat = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    return DeviceBuffer.from_array(np.concatenate([flat, np.zeros(flat.size % 2, dtype=np.int32)]).view(np.float64))


def _check_consistency(peak, timing, thr, rows):
    n_thr = len(thr)
    for j, th in enumerate(thr):
        dur, arr = timing[:, 1 + j], timing[:, 1 + n_thr + j]
        assert np.array_equal(arr < rows, dur > 0) and np.array_equal(dur > 0, peak > th), j
        assert np.all(dur <= rows - arr) and np.all(dur >= 0) and np.all(arr >= 0), j
    assert np.all((timing[:, 0] >= 0) & (timing[:, 0] < rows))


# ---- 1. the inputs cannot go vacuous -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LARGER)
def test_the_thresholds_separate_the_members(name):
    """On the mirror: members that never exceed, members that exceed from row 0 and members that arrive later all occur, and in the 65-row
    case arrivals fall in each of the three 32-row blocks of the walk."""
    state, scores, members, rows, y, thr = _case(name)
    _, timing = et.field_timing(y, thr)
    arr = timing[:, 1 + len(thr):]
    assert np.any(arr == rows) and np.any(arr == 0) and np.any((arr > 0) & (arr < rows))
    print(f"{name}: at the 0.9 and 0.999 quantiles never {np.mean(arr[:, 2:4] == rows):.2f}; at the six finite thresholds from row 0 "
          f"{np.mean(arr[:, :6] == 0):.2f}, later {np.mean((arr[:, :6] > 0) & (arr[:, :6] < rows)):.2f}")
    if rows == 65:
        for lo in (0, 32, 64):
            assert np.any((arr >= lo) & (arr < min(lo + 32, rows))), lo
        assert np.any(timing[:, 0] >= 32) and np.any(timing[:, 0] < 32)


# ---- 2. fused = refield = mirror, the peak the peaks kernel's -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PEAK_CASES))
def test_fused_equals_refield_equals_mirror(lib, name):
    state, scores, members, rows, y, thr = _case(name)
    proj = _projector(state)
    ens = _ensemble(proj)
    try:
        want_peak, want = et.field_timing(y, thr)
        assert np.array_equal(want_peak, en.member_peaks(state, scores))
        n_maps = want.shape[1]
        buf = ens.member_peaks_dev(scores, members, rows, route="fused")
        plain_peak = buf.to_array(want_peak.shape)
        buf.free()
        assert np.array_equal(plain_peak, want_peak)
        peak, timing = _download(ens, ens.member_timing_dev(scores, members, rows, thr, route="refield"), members, n_maps)
        assert timing.dtype == np.int32 and np.array_equal(timing, want) and np.array_equal(peak, plain_peak)
        _check_consistency(peak, timing, thr, rows)
        for group in GROUPS:  # 0: the launcher's choice; nothing is carried between members, so every grouping gives the same maps
            peak, timing = _download(ens, ens.member_timing_dev(scores, members, rows, thr, route="fused", member_group=group), members, n_maps)
            assert np.array_equal(timing, want), group
            assert np.array_equal(peak, plain_peak), group
            _check_consistency(peak, timing, thr, rows)
        for n_thr in (0, 1):  # (8 above)
            sub = thr[:n_thr]
            want_sub = et.field_timing(y, sub)[1]
            for route in ("fused", "refield"):
                peak, timing = _download(ens, ens.member_timing_dev(scores, members, rows, sub, route=route), members, 1 + 2 * n_thr)
                assert timing.shape[1] == 1 + 2 * n_thr and np.array_equal(timing, want_sub) and np.array_equal(peak, plain_peak), (route, n_thr)
    finally:
        proj.close()


def test_refield_slabs_of_members(lib, monkeypatch):
    """The refield route in slabs of one and of two members: a slab's maps land at the member's place in the block."""
    import gpras_amd.ensemble as ge

    state, scores, members, rows, y, thr = _case("k17_velocity")
    proj = _projector(state)
    ens = _ensemble(proj)
    try:
        want_peak, want = et.field_timing(y, thr[:3])
        for forced in (rows, 2 * rows + 1):
            monkeypatch.setattr(ge, "slab_rows", lambda pr, most_rows=None, forced=forced: forced)
            peak, timing = _download(ens, ens.member_timing_dev(scores, members, rows, thr[:3], route="refield"), members, 7)
            assert np.array_equal(timing, want) and np.array_equal(peak, want_peak)
    finally:
        proj.close()


# ---- 3. a NaN row -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,row", [("k17_velocity", 32), ("k64_depth", 40), ("k64_depth", 64)])
def test_a_nan_row_is_the_peak_and_is_not_counted(lib, name, row):
    """One NaN score in the second (or third) row block of one member: every cell of that member has its peak there, the durations skip
    the row, and the other members are untouched."""
    state, scores, members, rows, y, thr = _case(name)
    who = members - 2
    scores = scores.copy()
    scores[who, row, 0] = np.nan
    y = y.copy()
    y[who, row, :] = np.nan  # (a NaN mode value makes the row's sum a NaN in every cell, dry ones included: 0 * NaN)
    want_peak, want = et.field_timing(y, thr)
    proj = _projector(state)
    ens = _ensemble(proj)
    try:
        for route in ("fused", "refield"):
            peak, timing = _download(ens, ens.member_timing_dev(scores, members, rows, thr, route=route), members, want.shape[1])
            assert np.all(timing[who, 0] == row) and np.all(np.isnan(peak[who])), route
            assert np.array_equal(timing, want) and np.array_equal(peak, want_peak, equal_nan=True), route
            clean = et.field_timing(np.delete(y[who:who + 1], row, axis=1), thr)[1]
            assert np.array_equal(timing[who, 1:9], clean[0, 1:9]), route  # the durations of the member without that row
            assert np.all(timing[who, 8] == rows - 1)  # above -inf: every row but the NaN one
    finally:
        proj.close()


# ---- 4. statistics ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_e", [1, 33, 1024])  # bisection depths 1, 6 and 11
@pytest.mark.parametrize("members,cells", [(1, 5), (17, 300), (64, 257), (255, 40)])
def test_timing_statistics(lib, members, cells, rows_e):
    state, *_ = sn.make_case(cells, 2, [2], "wse", seed=1)
    proj = _projector(state)
    ens = _ensemble(proj)
    rng = np.random.default_rng(members + rows_e)
    n_maps = 5
    v = rng.integers(0, rows_e + 1, size=(members, n_maps, cells)).astype(np.int32)
    v[:, :, 0] = rows_e  # every member at the sentinel
    v[:, :, 1] = 0
    v[::2, :, 2] = rows_e  # half of them
    v[:, :, 3] = np.repeat(rng.integers(0, rows_e + 1, size=(members + 2) // 3), 3)[:members, None]  # ties
    v[0, :, 4] = rows_e // 2
    obs = rng.integers(0, rows_e + 1, size=(n_maps, cells)).astype(np.int32)
    obs[:, 3] = v[0, :, 3]
    levels = np.array(sorted({-1, 0, rows_e // 3, rows_e - 1, rows_e}), dtype=np.int32)
    ranks = np.array(sorted({0, members // 4, members // 2, members - 1}), dtype=np.int32)
    dv, dobs = _upload_i32(v), _upload_i32(obs)
    try:
        for map0, n_sel, sentinel, with_obs in ((0, 5, rows_e, True), (0, 1, -1, False), (1, 2, -1, True), (3, 2, rows_e, True), (4, 1, 0, False)):
            got = ens.timing_stats(dv, members, n_maps, map0, n_sel, rows_e, sentinel, levels, ranks,
                                   C.c_void_p(dobs.ptr.value + 4 * map0 * cells) if with_obs else None)
            sel = v[:, map0:map0 + n_sel]
            want = et.timing_stats(sel, sentinel, levels, ranks, obs[map0:map0 + n_sel] if with_obs else None)
            for key in ("cdf", "n_valid", "sum", "order", "below", "equal"):
                if want[key] is None:
                    assert got[key] is None, key
                else:
                    assert got[key].dtype == (np.int64 if key == "sum" else np.int32) and np.array_equal(got[key], want[key]), (key, map0, n_sel, sentinel)
            assert np.array_equal(got["order"], np.transpose(np.sort(sel, axis=0)[ranks], (1, 0, 2)))
            if sentinel == rows_e:
                assert not got["n_valid"][:, 0].any() and not got["sum"][:, 0].any() and np.all(got["order"][:, :, 0] == rows_e)
        bare = ens.timing_stats(dv, members, n_maps, 2, 1, rows_e)
        assert bare["cdf"].shape == (1, 0, cells) and bare["order"].shape == (1, 0, cells) and np.array_equal(bare["sum"][0], v[:, 2].sum(axis=0, dtype=np.int64))
    finally:
        dv.free()
        dobs.free()
        proj.close()


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------------
FIELDS = ("p_exceed", "peak_mean", "peak_std", "peak_quantiles", "wet_area", "exceed_counts", "thresholds", "quantiles")


def test_evaluate_with_timing(lib, fitted):  # noqa: F811
    import pandas as pd

    from gpras_amd.ensemble import EventTiming, PeakEnsemble, quantile_ranks
    from gpras_amd.pipeline import DevicePipeline

    gpr, state, xs, ranges = fitted
    members, thr, quantiles, durations, arrive_by = 8, (0.5, 1.0), (0.0, 0.5, 1.0), (0, 1, 5, 40), (0, 3, 100)
    k, cells, n_thr = len(gpr.models), 40, 2
    rng = np.random.default_rng(5)
    normals = [rng.standard_normal((k, members, hi - lo)) for lo, hi in ranges]
    truth = np.maximum(rng.normal(size=(60, cells)) + 0.6, 0.0)  # depths, a share of them exactly zero
    ranks = quantile_ranks(quantiles, members)
    proj = _projector(state)
    try:
        ens = PeakEnsemble(gpr, proj)
        pipe = DevicePipeline(gpr, proj)
        kw = dict(thresholds=thr, quantiles=quantiles, normals=normals)
        for route in ("fused", "refield"):
            plain = ens.evaluate(xs, ranges, members, **kw, route=route)
            timed = ens.evaluate(xs, ranges, members, **kw, route=route, timing=True, durations=durations, arrive_by=arrive_by, observed=truth)
            assert plain.timing is None and "timing" not in plain.last_timings_ms and "timing" in timed.last_timings_ms
            for name in FIELDS:
                assert np.array_equal(getattr(plain, name), getattr(timed, name)), (route, name)
            tm = timed.timing
            assert isinstance(tm, EventTiming) and tm.rows.tolist() == [hi - lo for lo, hi in ranges] and tm.members == members
            assert np.array_equal(tm.arrival_counts, timed.exceed_counts) and np.array_equal(tm.p_arrival * members, timed.exceed_counts)
            for e, (lo, hi) in enumerate(ranges):
                rows = hi - lo
                mean_dev, lc_dev, _ = ens.joint_dev(xs[lo:hi])
                scores_dev = None
                try:
                    scores_dev = ens.scores_dev(mean_dev, lc_dev, normals[e], members, rows)
                    scores = scores_dev.to_array((members, rows, k))
                finally:
                    for buf in (mean_dev, lc_dev, scores_dev):
                        if buf is not None:
                            buf.free()
                _, maps = et.member_timing(state, scores, thr)
                t_st = et.timing_stats(maps[:, :1], -1, (), ranks)
                d_st = et.timing_stats(maps[:, 1:3], -1, np.array(durations) - 1, ranks)
                a_st = et.timing_stats(maps[:, 3:5], rows, np.minimum(arrive_by, rows - 1), ranks)
                assert np.array_equal(tm.t_peak_sum[e], t_st["sum"][0]) and np.array_equal(tm.t_peak_quantiles[e], t_st["order"][0])
                assert np.array_equal(tm.t_peak_mean[e], maps[:, 0].sum(axis=0) / members)
                assert np.array_equal(tm.t_peak_quantiles[e], np.quantile(maps[:, 0], quantiles, axis=0, method="lower"))
                assert np.array_equal(tm.duration_sum[e], d_st["sum"]) and np.array_equal(tm.duration_quantiles[e], d_st["order"])
                assert np.array_equal(tm.duration_below_counts[e], d_st["cdf"])
                want_p = np.stack([(maps[:, 1:3] >= d).sum(axis=0) for d in durations], axis=1) / members
                assert np.array_equal(tm.p_duration_at_least[e], want_p)
                assert np.array_equal(tm.arrival_counts[e], a_st["n_valid"]) and np.array_equal(tm.arrival_sum[e], a_st["sum"])
                assert np.array_equal(tm.arrival_quantiles[e], a_st["order"]) and np.array_equal(tm.arrival_by_counts[e], a_st["cdf"])
                arrived = maps[:, 3:5] < rows
                assert np.array_equal(tm.p_arrival_by[e], np.stack([(arrived & (maps[:, 3:5] <= t)).sum(axis=0) for t in arrive_by], axis=1) / members)
                with np.errstate(invalid="ignore"):
                    assert np.array_equal(tm.arrival_mean[e], np.where(arrived, maps[:, 3:5], 0).sum(axis=0) / arrived.sum(axis=0), equal_nan=True)
                # the observed maps: observed_timing_dev's, and the truth's own by the mirror
                obs_dev = ens.observed_timing_dev(truth, lo, hi, thr)
                obs = ens.timing_to_array(obs_dev, 1, 5)[0]
                obs_dev.free()
                assert np.array_equal(tm.observed[e], obs) and np.array_equal(obs, et.field_timing(truth[None, lo:hi], thr)[1][0])
                assert np.array_equal(tm.below[e], (maps < obs[None]).sum(axis=0)) and np.array_equal(tm.equal[e], (maps == obs[None]).sum(axis=0))
            assert np.all(tm.below + tm.equal <= members) and tm.below.dtype == np.int32
        # through the pipeline, the truth as water-surface elevations converted on the device
        wse = truth + state["elevations"][None, :]
        depth = wse - state["elevations"][None, :]
        depth = np.where(depth < 0.0, 0.0, depth)
        df = pd.DataFrame(wse, index=_index(ranges))
        piped = pipe.peak_ensemble(xs, df, members, verify=True, timing=True, durations=durations, arrive_by=arrive_by, **kw)
        direct = ens.evaluate(xs, ranges, members, **kw, timing=True, durations=durations, arrive_by=arrive_by, observed=depth)
        assert piped.timing.names == piped.names == [f"event{e}" for e in range(len(ranges))] and piped.verification is not None
        for name in ("t_peak_sum", "t_peak_quantiles", "duration_sum", "duration_quantiles", "duration_below_counts", "arrival_counts", "arrival_sum",
                     "arrival_quantiles", "arrival_by_counts", "observed", "below", "equal"):
            assert np.array_equal(getattr(piped.timing, name), getattr(direct.timing, name)), name
        assert pipe.peak_ensemble(xs, df, members, **kw).timing is None
        unobserved = pipe.peak_ensemble(xs, df, members, timing=True, **kw).timing
        assert unobserved.observed is None and unobserved.below is None and np.array_equal(unobserved.arrival_sum, direct.timing.arrival_sum)
        # rng="device": a draw is a function of its address, so the maps of an 8-member run are the first 8 of a 16-member run
        lo, hi = ranges[1]
        rows = hi - lo
        mean_dev, lc_dev, _ = ens.joint_dev(xs[lo:hi])
        got = {}
        try:
            for s in (8, 16):
                zn = ens.normals_dev(1, s, rows, seed=3)
                scores_dev = ens.scores_dev(mean_dev, lc_dev, zn, s, rows)
                zn.free()
                got[s] = _download(ens, ens.member_timing_dev(scores_dev, s, rows, thr), s, 5)
                scores_dev.free()
        finally:
            mean_dev.free()
            lc_dev.free()
        assert np.array_equal(got[8][1], got[16][1][:8]) and np.array_equal(got[8][0], got[16][0][:8])
        small = ens.evaluate(xs, ranges, 8, thresholds=thr, quantiles=quantiles, rng="device", seed=3, timing=True)
        st = et.timing_stats(got[8][1][:, 3:5], rows, (), ranks)
        assert np.array_equal(small.timing.arrival_counts[1], st["n_valid"]) and np.array_equal(small.timing.arrival_quantiles[1], st["order"])
        # the refusals of evaluate
        for bad in (dict(timing=True, thresholds=()), dict(timing=True, durations=np.arange(9)), dict(timing=True, arrive_by=(-1,)),
                    dict(timing=True, durations=(1.5,)), dict(durations=(1,)), dict(arrive_by=(1,))):
            with pytest.raises(ValueError):
                ens.evaluate(xs, ranges, members, **{**dict(thresholds=thr), **bad})
    finally:
        proj.close()


# ---- 6. the C ABI's refusals -----------------------------------------------------------------------------------------------------------------
def test_abi_refusals(lib):
    cells = 40
    state, *_ = sn.make_case(cells, 2, [2], "wse", seed=1)
    proj = _projector(state)
    scores, field, out = DeviceBuffer.from_array(np.zeros((4, 3, 2))), DeviceBuffer.from_array(np.zeros((4 * 3, cells))), DeviceBuffer(8 * cells * 64)
    ph = proj.handle
    thr9, nan = np.zeros(9), np.array([np.nan])
    zero4, rank4, i9 = np.zeros(4, dtype=np.int32), np.array([4], dtype=np.int32), np.zeros(9, dtype=np.int32)
    timing = _upload_i32(np.zeros((4, 3, cells), dtype=np.int32))

    def fused(scores_p=scores.ptr, members=4, rows=3, mode=1, group=0, n_thr=1, thr=thr9, peak=out.ptr, maps=out.at(1000)):
        return lib.gprx_pca_ensemble_timing_dev(ph, scores_p, members, rows, mode, group, n_thr, ptr(thr) if thr is not None else None, peak, maps)

    def refield(field_p=field.ptr, members=4, rows=3, n_thr=1, thr=thr9, peak=None, maps=out.at(1000)):
        return lib.gprx_pca_member_timing_dev(ph, field_p, members, rows, n_thr, ptr(thr) if thr is not None else None, peak, maps)

    def stats(timing_p=timing.ptr, members=4, n_maps=3, map0=0, n_sel=3, rows=3, sentinel=-1, n_lev=1, levels=zero4, n_rank=1, ranks=zero4, obs=None,
              cdf=out.at(0), valid=out.at(500), total=out.at(1000), order=out.at(1500), below=None, equal=None):
        return lib.gprx_pca_timing_stats_dev(ph, timing_p, members, n_maps, map0, n_sel, rows, sentinel, n_lev, ptr(levels), n_rank, ptr(ranks), obs, cdf, valid,
                                             total, order, below, equal)

    def refused(rc, word):
        msg = lib.gprx_pca_last_error(ph) or b""
        assert rc == GPRX_EINVAL and word in msg, (rc, msg)

    try:
        assert fused() == GPRX_OK and refield() == GPRX_OK and stats() == GPRX_OK
        for call in (fused, refield):
            refused(call(n_thr=9), b"thresholds")
            refused(call(thr=nan), b"NaN")
            refused(call(thr=None), b"thresholds")
            refused(call(maps=None), b"null")
            refused(call(rows=0), b"positive")
            refused(call(members=0), b"positive")
        refused(fused(scores_p=None), b"null")
        refused(fused(peak=None), b"null")
        refused(fused(mode=3), b"depth mode")
        refused(fused(group=65), b"member_group")
        refused(refield(field_p=None), b"null")
        refused(refield(members=65536, rows=1), b"65535")
        refused(lib.gprx_pca_ensemble_timing_ms(ph, None), b"null")
        refused(stats(timing_p=None), b"null")
        refused(stats(valid=None), b"null")
        refused(stats(total=None), b"null")
        refused(stats(members=0), b"members")
        refused(stats(members=4097), b"members")
        refused(stats(rows=0), b"rows")
        refused(stats(rows=2**31 - 1), b"rows")
        refused(stats(n_sel=0), b"maps")
        refused(stats(map0=1), b"maps")
        refused(stats(n_maps=18, n_sel=1), b"maps")
        refused(stats(sentinel=4), b"sentinel")
        refused(stats(sentinel=-2), b"sentinel")
        refused(stats(n_lev=9, levels=i9), b"levels")
        refused(stats(cdf=None), b"levels")
        refused(stats(n_rank=9, ranks=i9), b"ranks")
        refused(stats(order=None), b"ranks")
        refused(stats(ranks=rank4), b"ranks must lie")
        refused(stats(ranks=np.array([-1], dtype=np.int32)), b"ranks must lie")
        refused(stats(obs=timing.ptr), b"below")
        assert stats(n_lev=0, cdf=None, n_rank=0, order=None) == GPRX_OK and fused(n_thr=0, thr=None) == GPRX_OK  # still usable
        ms = C.c_double(-1.0)
        assert lib.gprx_pca_ensemble_timing_ms(ph, C.byref(ms)) == GPRX_OK and ms.value >= 0.0
    finally:
        for b in (scores, field, out, timing):
            b.free()
        proj.close()
