"""The ensemble verification on the GPU (gpras_amd.ensemble.verify_peaks, csrc/verify.h) against the numpy mirror (ensemble_verify_numpy.py):
the CRPS bit for bit, the rank counts exactly, the order statistics bit for bit against the mirror and against
``gprx_pca_member_stats_dev``; the invariances (permutation of the members, the neighbours and the position in the tile, repetition);
``evaluate(observed=...)`` end to end against the composition of its stages; and the refusals of the C ABI.  Every comparison is an equality:
a NaN must stand where the mirror has one (its payload is the machine's), every other value must have the mirror's bits."""

import ctypes as C

import numpy as np
import pytest

import ensemble_verify_numpy as ev
import sweep_numpy as sn
from gpras_amd._lib import GPRX_EINVAL, GPRX_OK, DeviceBuffer, ptr
from gpras_amd.synth import make_regression

pytestmark = pytest.mark.gpu

MEMBERS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 4096)
# the consecutive cells one workgroup sorts: 4096 keys over Sp = the members rounded up to a power of two (at least 32); 8192 keys at Sp = 4096
TILE = {1: 128, 2: 128, 3: 128, 63: 64, 64: 64, 65: 32, 255: 16, 256: 16, 257: 8, 1000: 4, 4096: 2}
CELLS = ("1", "C-1", "C", "C+1", "257", "1000")
KINDS = 12


def _projector(state):
    from gpras_amd.preprocess import EOFProjector

    return EOFProjector(state["dry"], state["elevations"], state["input_mean"], state["weights"], state["eofs"], state["x_mean"], state["x_std"], state["hp"])


class _Bare:
    """What ``PeakEnsemble`` reads of a ``GPRAS`` when only the projector side is exercised."""

    def __init__(self, k):
        self.models = [None] * k


def _ensemble(proj):
    from gpras_amd.ensemble import PeakEnsemble

    return PeakEnsemble(_Bare(proj.spatial_mode_count), proj)


def _bare_projector(cells):
    state, *_ = sn.make_case(cells, 1, [1], "wse", seed=1)
    return _projector(state)


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want):
    """Equal bits, a NaN exactly where the other has one."""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype != np.float64:
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]))


def _contents(members, cells, shift, seed):
    """``peak (S, cells)`` and ``obs (cells,)``: column c holds the content of kind ``(c + shift) % KINDS``."""
    rng = np.random.default_rng(seed)
    S = members
    peak = rng.normal(size=(S, cells)) * 2.0 + 1.0
    obs = rng.normal(size=cells) * 2.0 + 1.0
    pick = rng.integers(0, S, size=cells)
    for c in range(cells):
        kind = (c + shift) % KINDS
        col = peak[:, c]
        if kind == 1:  # integer-valued peaks with many duplicates, the observation one of the integers
            col[:] = np.round(rng.uniform(0.0, 5.0, size=S))
            obs[c] = 2.0
        elif kind == 2:  # dry everywhere
            col[:] = 0.0
            obs[c] = 0.0
        elif kind == 3:
            obs[c] = col.min() - 1.0
        elif kind == 4:
            obs[c] = col.max() + 1.0
        elif kind == 5:  # equal to a member
            obs[c] = col[pick[c]]
        elif kind == 6:  # +0 and -0 mixed among positive depths, the observation a zero
            col[:] = np.where(rng.uniform(size=S) < 0.4, 0.0, np.abs(col))
            col[rng.uniform(size=S) < 0.3] = -0.0
            col[pick[c]] = -0.0 if c % 2 else 0.0
            obs[c] = 0.0 if c % 2 else -0.0
        elif kind == 7:  # one NaN member
            col[pick[c]] = np.nan
        elif kind == 8:  # a NaN observation
            obs[c] = np.nan
        elif kind == 9:  # infinite members, a finite observation
            col[pick[c]] = np.inf
            col[(pick[c] + 1) % S] = -np.inf
        elif kind == 10:  # an infinite member and the same infinity observed: |inf - inf|
            col[pick[c]] = np.inf
            obs[c] = np.inf
        elif kind == 11:  # clamped depths: a share at exactly zero, the observation wet
            col[:] = np.maximum(col - 1.0, 0.0)
            obs[c] = abs(obs[c])
    return peak, obs


def _ranks(members):
    return np.array(sorted({0, members // 4, members // 2, members - 1}), dtype=np.int32)


def _stats_order(lib, proj, dpeak, members, ranks, cells):
    """``order`` of ``gprx_pca_member_stats_dev`` for the same ranks: the independent yardstick on the device."""
    out = DeviceBuffer(8 * (2 + ranks.size) * cells)
    try:
        rc = lib.gprx_pca_member_stats_dev(proj.handle, dpeak.ptr, members, 0, None, int(ranks.size), ptr(ranks), None, None, out.ptr, out.at(cells),
                                           out.at(2 * cells), None)
        assert rc == GPRX_OK
        return out.to_array((2 + ranks.size, cells))[2:]
    finally:
        out.free()


@pytest.mark.parametrize("cells_key", CELLS)
@pytest.mark.parametrize("members", MEMBERS)
def test_kernel_against_the_mirror(lib, members, cells_key):
    tile = C.c_int()
    assert lib.gprx_pca_member_verify_tile(members, C.byref(tile)) == GPRX_OK and tile.value == TILE[members]
    cells = {"1": 1, "C-1": max(1, tile.value - 1), "C": tile.value, "C+1": tile.value + 1, "257": 257, "1000": 1000}[cells_key]
    proj = _bare_projector(cells)
    ens = _ensemble(proj)
    ranks = _ranks(members)
    try:
        for shift in range(0, KINDS, min(cells, KINDS)):  # every kind of content at every shape, also where the cells are fewer than the kinds
            peak, obs = _contents(members, cells, shift, seed=members + shift)
            want = ev.verify_peaks(peak, obs, ranks)
            dpeak, dobs = DeviceBuffer.from_array(peak), DeviceBuffer.from_array(obs)
            try:
                got = ens.verify_peaks(dpeak, dobs, members, ranks)
                assert got["below"].dtype == np.int32 and got["equal"].dtype == np.int32
                assert np.array_equal(got["below"], want["below"]) and np.array_equal(got["equal"], want["equal"])
                assert _same(got["crps"], want["crps"])
                assert np.array_equal(_bits(got["order"]), _bits(want["order"]))
                assert np.array_equal(_bits(got["order"]), _bits(_stats_order(lib, proj, dpeak, members, ranks, cells)))
                bare = ens.verify_peaks(dpeak, dobs, members)  # no ranks: order_dev NULL
                assert bare["order"].shape == (0, cells) and _same(bare["crps"], got["crps"]) and np.array_equal(bare["below"], got["below"])
            finally:
                dpeak.free()
                dobs.free()
    finally:
        proj.close()


@pytest.mark.parametrize("members", [3, 64, 257, 1000])
def test_invariances(lib, members):
    """Permuting the members, changing the neighbours and the position in the tile, and calling twice all leave a cell's bits alone."""
    cells = 100
    proj = _bare_projector(cells)
    ens = _ensemble(proj)
    ranks = _ranks(members)

    def run(peak, obs):
        dpeak, dobs = DeviceBuffer.from_array(peak), DeviceBuffer.from_array(obs)
        try:
            return ens.verify_peaks(dpeak, dobs, members, ranks)
        finally:
            dpeak.free()
            dobs.free()

    def same(a, b, ca=slice(None), cb=slice(None)):
        return all(_same(np.ascontiguousarray(a[key][..., ca]), np.ascontiguousarray(b[key][..., cb])) for key in a)

    try:
        peak, obs = _contents(members, cells, 0, seed=members)
        first = run(peak, obs)
        assert same(first, run(peak, obs))  # two calls
        for seed in range(2):
            assert same(first, run(peak[np.random.default_rng(seed).permutation(members)], obs)), seed
        # the columns 0 .. KINDS - 1 again at another offset -- another tile, another position in it -- among other neighbours
        other, other_obs = _contents(members, cells, 5, seed=members + 99)
        for off in (KINDS + 1, 61):
            moved, moved_obs = other.copy(), other_obs.copy()
            moved[:, off:off + KINDS], moved_obs[off:off + KINDS] = peak[:, :KINDS], obs[:KINDS]
            assert same(first, run(moved, moved_obs), slice(0, KINDS), slice(off, off + KINDS)), off
    finally:
        proj.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    """A small fitted sparse GPRAS (N = 300, M = 20, K = 3), its projector over 70 cells, test inputs of two events of 5 and 65 rows."""
    from gpras_amd.gpr import GPRAS

    k, cells, d = 3, 70, 4
    state, *_ = sn.make_case(cells, k, [5], "wse", seed=21)
    x, y, xs = make_regression(300, d, n_outputs=k, n_test=70, config=9)
    gpr = GPRAS("RBF")
    gpr.fit(x, y, 20, "kmeans", "adam", max_iter=5)
    return gpr, state, xs, [(0, 5), (5, 70)]


def _index(ranges):
    import pandas as pd

    return pd.MultiIndex.from_tuples([(f"event{e}", t) for e, (lo, hi) in enumerate(ranges) for t in range(hi - lo)], names=["event", "timestep"])


FIELDS = ("p_exceed", "peak_mean", "peak_std", "peak_quantiles", "wet_area", "exceed_counts", "thresholds", "quantiles")


def test_evaluate_with_observed(lib, fitted):
    import pandas as pd

    from gpras_amd.ensemble import PeakEnsemble, PeakVerification
    from gpras_amd.pipeline import DevicePipeline

    gpr, state, xs, ranges = fitted
    members, thr, quantiles = 64, (0.5, 1.0), (0.05, 0.5, 0.95)
    k, cells, rows = len(gpr.models), 70, 70
    rng = np.random.default_rng(5)
    normals = [rng.standard_normal((k, members, hi - lo)) for lo, hi in ranges]
    truth = np.maximum(rng.normal(size=(rows, cells)) + 0.8, 0.0)  # depths, a share of them exactly zero
    truth[7, 3] = np.nan
    proj = _projector(state)
    try:
        ens = PeakEnsemble(gpr, proj)
        kw = dict(thresholds=thr, quantiles=quantiles, normals=normals)
        plain = ens.evaluate(xs, ranges, members, **kw)
        with_obs = ens.evaluate(xs, ranges, members, **kw, observed=truth)
        assert plain.verification is None and "verify" not in plain.last_timings_ms
        v = with_obs.verification
        assert isinstance(v, PeakVerification) and {"verify", "device_verify"} <= set(with_obs.last_timings_ms)
        for name in FIELDS:
            assert np.array_equal(getattr(plain, name), getattr(with_obs, name)), name
        assert plain.ranges == with_obs.ranges and plain.members == with_obs.members == v.members and plain.route == with_obs.route
        assert np.array_equal(v.exceed_counts, plain.exceed_counts) and np.array_equal(v.thresholds, plain.thresholds)
        assert v.below.dtype == np.int32 and v.equal.dtype == np.int32 and v.crps.shape == (2, cells)
        dtruth = DeviceBuffer.from_array(truth)
        try:
            resident = ens.evaluate(xs, ranges, members, **kw, observed=dtruth).verification
            for e, (lo, hi) in enumerate(ranges):
                mean_dev, lc_dev, _ = ens.joint_dev(xs[lo:hi])
                scores_dev = peak_dev = obs_dev = None
                try:
                    scores_dev = ens.scores_dev(mean_dev, lc_dev, normals[e], members, hi - lo)
                    peak_dev = ens.member_peaks_dev(scores_dev, members, hi - lo)
                    obs_dev = ens.observed_peak_dev(dtruth, lo, hi)
                    peak, obs = peak_dev.to_array((members, cells)), obs_dev.to_array((cells,))
                    obs_host = ens.observed_peak_dev(truth, lo, hi)
                    assert _same(obs_host.to_array((cells,)), obs)
                    obs_host.free()
                finally:
                    for buf in (mean_dev, lc_dev, scores_dev, peak_dev, obs_dev):
                        if buf is not None:
                            buf.free()
                arg = np.argmax(truth[lo:hi], axis=0)  # the first maximum, a NaN taken as the maximum
                assert _same(obs, truth[lo:hi][arg, np.arange(cells)])
                want = ev.verify_peaks(peak, obs)
                for got in (v, resident):
                    assert _same(got.crps[e], want["crps"]) and _same(got.observed_peak[e], obs)
                    assert np.array_equal(got.below[e], want["below"]) and np.array_equal(got.equal[e], want["equal"])
            assert np.isnan(v.crps[1, 3]) and v.below[1, 3] == -1 and not v.valid[1, 3] and v.valid[0].all()
        finally:
            dtruth.free()
        # the aggregations run on what came back
        assert np.array_equal(v.rank_histogram().sum(axis=1).round(), (v.valid & (v.equal < members)).sum(axis=1))
        assert v.mean_crps().shape == (2,) and v.brier().shape == (2, 2) and v.reliability().sum(axis=2)[:, :, 0].tolist() == [[70, 70], [69, 69]]
        # the pipeline: the truth as water-surface elevations, sent up once and converted on the device
        pipe = DevicePipeline(gpr, proj)
        wse = truth + state["elevations"][None, :]
        depth = wse - state["elevations"][None, :]
        depth = np.where(depth < 0.0, 0.0, depth)
        df = pd.DataFrame(wse, index=_index(ranges))
        piped = pipe.peak_ensemble(xs, df, members, verify=True, **kw)
        direct = ens.evaluate(xs, ranges, members, **kw, observed=depth).verification
        pv = piped.verification
        assert pv.names == piped.names == ["event0", "event1"]
        assert _same(pv.crps, direct.crps) and np.array_equal(pv.below, direct.below) and np.array_equal(pv.equal, direct.equal)
        assert _same(pv.observed_peak, direct.observed_peak)
        assert pipe.peak_ensemble(xs, df, members, **kw).verification is None
        with pytest.raises(ValueError):
            pipe.peak_ensemble(xs, df.index, members, verify=True, **kw)
        for bad in (truth[:-1], truth[:, :-1]):
            with pytest.raises(ValueError):
                ens.evaluate(xs, ranges, members, **kw, observed=bad)
    finally:
        proj.close()


# ---- the C ABI's refusals -------------------------------------------------------------------------------------------------------------------
def test_abi_refusals(lib):
    cells = 40
    proj = _bare_projector(cells)
    peak, obs, out = DeviceBuffer.from_array(np.zeros((4, cells))), DeviceBuffer.from_array(np.zeros(cells)), DeviceBuffer(8 * cells * 8)
    ph = proj.handle
    one = np.array([0], dtype=np.int32)

    def verify(members, n_rank, ranks, crps=out.ptr, below=out.at(cells), equal=out.at(2 * cells), order=out.at(3 * cells), peak_ptr=peak.ptr,
               obs_ptr=obs.ptr):
        return lib.gprx_pca_member_verify_dev(ph, peak_ptr, obs_ptr, members, n_rank, ptr(ranks), crps, below, equal, order)

    def refused(rc, word):
        message = lib.gprx_pca_last_error(ph) or b""
        return rc == GPRX_EINVAL and word in message

    try:
        assert refused(verify(0, 0, one), b"members")
        assert refused(verify(4097, 0, one), b"members")
        assert refused(verify(4, 1, np.array([4], dtype=np.int32)), b"ranks")
        assert refused(verify(4, 1, np.array([-1], dtype=np.int32)), b"ranks")
        assert refused(verify(4, 9, np.zeros(9, dtype=np.int32)), b"ranks")
        assert refused(verify(4, 1, one, order=None), b"ranks")  # ranks without their output block
        assert refused(verify(4, 0, one, crps=None), b"null")
        assert refused(verify(4, 0, one, below=None), b"null")
        assert refused(verify(4, 0, one, equal=None), b"null")
        assert refused(verify(4, 0, one, peak_ptr=None), b"null")
        assert refused(verify(4, 0, one, obs_ptr=None), b"null")
        assert lib.gprx_pca_member_verify_dev(None, peak.ptr, obs.ptr, 4, 0, None, out.ptr, out.at(cells), out.at(2 * cells), None) == GPRX_EINVAL
        tile = C.c_int()
        assert lib.gprx_pca_member_verify_tile(0, C.byref(tile)) == GPRX_EINVAL and lib.gprx_pca_member_verify_tile(4097, C.byref(tile)) == GPRX_EINVAL
        assert verify(4, 0, one, order=None) == GPRX_OK and verify(4, 1, np.array([3], dtype=np.int32)) == GPRX_OK  # still usable
        assert np.array_equal(out.to_array((cells,)), np.zeros(cells))  # all members and the observation 0: CRPS 0
    finally:
        for b in (peak, obs, out):
            b.free()
        proj.close()
