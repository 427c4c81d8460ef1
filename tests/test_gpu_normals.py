"""The device generator of ``PeakEnsemble`` on the GPU (``gprx_pca_normals_dev``, ``gprx_pca_normal_transform_dev``; csrc/normals.h,
csrc/ensemble.h) against the numpy mirror (normals_numpy.py): the words bit for bit, the normals bit for bit on the central branch of AS 241
and within 16 eps relative in the tails (``px_log`` against ``np.log``: test_normals.py has the argument), the padding columns exact zeros,
the stream a function of its address alone, antithetic members, ``PeakEnsemble.evaluate(rng="device")`` end to end and the argument
checks of the two exports."""

import ctypes as C

import numpy as np
import pytest

import normals_numpy as nn
import sweep_numpy as sn
from gpras_amd._lib import GPRX_EINVAL, GPRX_OK, DeviceBuffer, check, ptr
from gpras_amd.synth import make_regression

pytestmark = pytest.mark.gpu

SEED, STREAM = 2**63 + 12345, 2**64 - 7  # both above 2^63
EVENT, K, MEMBER0, MEMBERS = 7, 3, 2, 5
ROWS = (1, 63, 65, 130)
OUTPUTS = ("exceed_counts", "p_exceed", "peak_mean", "peak_std", "peak_quantiles", "wet_area")


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


@pytest.fixture(scope="module")
def ens3(lib):
    state, *_ = sn.make_case(40, K, [5], "wse", seed=3)
    proj = _projector(state)
    yield _ensemble(proj)
    proj.close()


@pytest.fixture(scope="module")
def ens1(lib):
    state, *_ = sn.make_case(40, 1, [5], "wse", seed=4)
    proj = _projector(state)
    yield _ensemble(proj)
    proj.close()


def _tp(rows):
    return (rows + 63) // 64 * 64


def _draw(ens, event, members, rows, raw=False, **kw):
    """The ``(K, members, Tp)`` block of ``normals_dev`` on the host: float64, or uint64 when ``raw``."""
    kw.setdefault("seed", SEED)
    kw.setdefault("stream", STREAM)
    buf = ens.normals_dev(event, members, rows, raw=raw, **kw)
    try:
        out = buf.to_array((ens.projector.spatial_mode_count, members, _tp(rows)))
    finally:
        buf.free()
    return out.view(np.uint64) if raw else out


# ---- words and normals against the mirror -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS)
def test_raw_words(ens3, rows):
    got = _draw(ens3, EVENT, MEMBERS, rows, raw=True, member0=MEMBER0)
    want = nn.words(SEED, STREAM, EVENT, K, MEMBER0, MEMBERS, rows, _tp(rows))
    assert np.array_equal(got[:, :, :rows], want[:, :, :rows])
    assert not got[:, :, rows:].any()  # exact zero words
    assert np.array_equal(got, want)


def test_normals(ens3):
    seen_central = seen_tail = 0
    for rows in ROWS:
        tp = _tp(rows)
        got = _draw(ens3, EVENT, MEMBERS, rows, member0=MEMBER0)
        w = nn.words(SEED, STREAM, EVENT, K, MEMBER0, MEMBERS, rows, tp)
        central, _ = nn.assert_normals_match(got[:, :, :rows], w[:, :, :rows], f"rows={rows}")
        seen_central += int(central.sum())
        seen_tail += int((~central).sum())
        pad = got[:, :, rows:]
        assert not pad.any() and not np.signbit(pad).any()  # exact +0.0
        if rows >= 63:
            assert central.any() and (~central).any()
    assert seen_central > 0 and seen_tail > 0  # both branches occurred


def test_transform_of_chosen_words(lib, ens3):
    rnd = nn.philox4x64_10(np.arange(1024, dtype=np.uint64), 9, 8, 7, 6, 5).ravel()  # 4096 random words
    w = np.ascontiguousarray(np.concatenate([nn.boundary_words(), rnd, rnd[:512] >> np.uint64(40), ~(rnd[512:1024] >> np.uint64(40))]))
    ph = ens3.projector.handle
    dw, dz = DeviceBuffer.from_array(w.view(np.float64)), DeviceBuffer(8 * w.size)
    try:
        check(lib.gprx_pca_normal_transform_dev(ph, dw.ptr, w.size, dz.ptr))
        check(lib.gprx_pca_synchronize(ph))
        z = dz.to_array((w.size,))
    finally:
        dw.free()
        dz.free()
    central, far = nn.assert_normals_match(z, w, "chosen words")  # (every word: the r > 5 words are within the same 16 eps)
    assert central.any() and (~central & ~far).any() and far.sum() >= 1000
    z0, z1 = z[np.flatnonzero(w == 0)[0]], z[np.flatnonzero(w == np.uint64(nn.MASK64))[0]]
    assert np.isfinite(z0) and z0 < -8.2 and z1 == -z0
    # the antisymmetry on the device, exactly
    dw, dz = DeviceBuffer.from_array((~w).view(np.float64)), DeviceBuffer(8 * w.size)
    try:
        check(lib.gprx_pca_normal_transform_dev(ph, dw.ptr, w.size, dz.ptr))
        check(lib.gprx_pca_synchronize(ph))
        assert np.array_equal(dz.to_array((w.size,)), -z)
    finally:
        dw.free()
        dz.free()


# ---- the stream is a function of its address ---------------------------------------------------------------------------------------------------------
def test_stream_is_a_function_of_its_address(ens3, ens1):
    rows = 65
    first8 = _draw(ens3, EVENT, 8, rows)
    halves = np.concatenate([_draw(ens3, EVENT, 4, rows, member0=0), _draw(ens3, EVENT, 4, rows, member0=4)], axis=1)
    assert np.array_equal(halves, first8)
    assert np.array_equal(_draw(ens3, EVENT, 16, rows)[:, :8], first8)
    # K = 1 is mode 0 of K = 3
    assert np.array_equal(_draw(ens1, EVENT, 8, rows)[0], first8[0])
    # the same event index with other row counts: the same leading draws
    for other in (1, 63, 130):
        lead = min(other, rows)
        assert np.array_equal(_draw(ens3, EVENT, 8, other)[:, :, :lead], first8[:, :, :lead])
    # another event, seed or stream: other draws
    assert not np.array_equal(_draw(ens3, EVENT + 1, 8, rows), first8)
    assert not np.array_equal(_draw(ens3, EVENT, 8, rows, seed=SEED + 1), first8)
    assert not np.array_equal(_draw(ens3, EVENT, 8, rows, stream=STREAM - 1), first8)
    # raw words obey the same addressing
    assert np.array_equal(_draw(ens3, EVENT, 2, rows, raw=True, member0=5), _draw(ens3, EVENT, 16, rows, raw=True)[:, 5:7])


def test_antithetic_members(ens3):
    for rows in (63, 130):
        plain = _draw(ens3, EVENT, 8, rows)
        anti = _draw(ens3, EVENT, 8, rows, antithetic=True)  # pair_offset = 4
        assert np.array_equal(anti[:, :4], plain[:, :4])
        assert np.array_equal(anti[:, 4:, :rows].view(np.uint64), plain[:, :4, :rows].view(np.uint64) ^ np.uint64(1 << 63))  # -z bit for bit
        assert not anti[:, :, rows:].any() and not np.signbit(anti[:, :, rows:]).any()
        part = _draw(ens3, EVENT, 3, rows, antithetic=4, member0=3)  # members 3, 4, 5 of that ensemble
        assert np.array_equal(part.view(np.uint64), anti[:, 3:6].view(np.uint64))
        raw = _draw(ens3, EVENT, 8, rows, raw=True, antithetic=True)
        assert np.array_equal(raw[:, 4:], raw[:, :4]) and np.array_equal(raw, nn.words(SEED, STREAM, EVENT, K, 0, 8, rows, _tp(rows), 4))


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted(lib):
    """The fitted fixture of test_gpu_ensemble.py: a small GPRAS (N = 200, K = 3, M = 10), a projector state over 40 cells, 3 events."""
    from gpras_amd.gpr import GPRAS

    k, cells, d = 3, 40, 4
    state, *_ = sn.make_case(cells, k, [5], "wse", seed=21)
    x, y, xs = make_regression(200, d, n_outputs=k, n_test=60, config=9)
    gpr = GPRAS("RBF")
    gpr.fit(x, y, 10, "kmeans", "adam", max_iter=5)
    return gpr, state, xs, [(0, 7), (7, 40), (40, 60)]


def _same(a, b):
    return all(np.array_equal(getattr(a, n), getattr(b, n)) for n in OUTPUTS)


def test_evaluate_with_the_device_generator(lib, fitted):
    from gpras_amd._device import StageTimer
    from gpras_amd.ensemble import STAGES, PeakEnsemble, padded_rows

    gpr, state, xs, ranges = fitted
    k, members = len(gpr.models), 8
    kw = dict(thresholds=(0.5, 1.0), quantiles=(0.0, 0.5, 1.0))
    proj = _projector(state)
    try:
        ens = PeakEnsemble(gpr, proj)
        downloaded = [_draw(ens, e, members, hi - lo, seed=5, stream=0) for e, (lo, hi) in enumerate(ranges)]
        by_route = {}
        for route in ("fused", "refield"):
            dev = ens.evaluate(xs, ranges, members, seed=5, rng="device", route=route, **kw)
            given = ens.evaluate(xs, ranges, members, normals=downloaded, route=route, **kw)
            assert dev.rng == "device" and given.rng == "host" and dev.route == route
            assert _same(dev, given), route  # every output, bit for bit
            assert _same(dev, ens.evaluate(xs, ranges, members, seed=5, rng="device", route=route, **kw)), route  # the same bits again
            assert dev.last_timings_ms["host_link_bytes"] == 0 and given.last_timings_ms["host_link_bytes"] == sum(8 * z.size for z in downloaded)
            by_route[route] = dev
        assert _same(by_route["fused"], by_route["refield"])
        dev = by_route["fused"]
        host = ens.evaluate(xs, ranges, members, seed=5, rng="host", **kw)
        assert host.rng == "host" and not np.array_equal(host.peak_mean, dev.peak_mean)
        assert _same(host, ens.evaluate(xs, ranges, members, seed=5, **kw))  # "host" is the default
        assert not np.array_equal(ens.evaluate(xs, ranges, members, seed=6, rng="device", **kw).peak_mean, dev.peak_mean)
        assert not np.array_equal(ens.evaluate(xs, ranges, members, seed=5, stream=1, rng="device", **kw).peak_mean, dev.peak_mean)
        # members are nested: the first 8 of 16 are the 8
        big = ens.evaluate(xs, ranges, 16, seed=5, rng="device", **kw)
        assert np.array_equal(big.wet_area[:, :8], dev.wet_area)
        # antithetic runs; every statistic stays finite (cells of zero variance included)
        anti = ens.evaluate(xs, ranges, members, seed=5, rng="device", antithetic=True, **kw)
        assert np.array_equal(anti.wet_area[:, :4], dev.wet_area[:, :4]) and not np.array_equal(anti.peak_mean, dev.peak_mean)
        assert np.all(np.isfinite(anti.peak_mean)) and np.all(np.isfinite(anti.peak_std)) and np.all(np.isfinite(anti.peak_quantiles))
        # scores_dev with a resident block: no link traffic, the same scores as from the host copy, the caller's buffer left alone
        lo, hi = ranges[1]
        rows, tp = hi - lo, padded_rows(hi - lo)
        mean_dev, lc_dev, _ = ens.joint_dev(xs[lo:hi])
        zbuf = ens.normals_dev(1, members, rows, seed=5)
        try:
            timer = StageTimer(STAGES)
            s_dev = ens.scores_dev(mean_dev, lc_dev, zbuf, members, rows, timer=timer)
            assert timer.link_bytes == 0 and zbuf.ptr is not None
            assert np.array_equal(zbuf.to_array((k, members, tp)), downloaded[1])
            timer = StageTimer(STAGES)
            s_host = ens.scores_dev(mean_dev, lc_dev, downloaded[1], members, rows, timer=timer)
            assert timer.link_bytes == 8 * k * members * tp
            assert np.array_equal(s_dev.to_array((members, rows, k)), s_host.to_array((members, rows, k)))
            s_dev.free()
            s_host.free()
            with pytest.raises(ValueError):
                ens.scores_dev(mean_dev, lc_dev, zbuf, members + 1, rows)  # a buffer too small for the block
        finally:
            for b in (mean_dev, lc_dev, zbuf):
                b.free()
    finally:
        proj.close()


def test_pipeline_passes_the_generator_through(lib, fitted):
    import pandas as pd

    from gpras_amd.ensemble import PeakEnsemble
    from gpras_amd.pipeline import DevicePipeline

    gpr, state, xs, ranges = fitted
    index = pd.MultiIndex.from_tuples([(f"event{e}", t) for e, (lo, hi) in enumerate(ranges) for t in range(hi - lo)], names=["event", "timestep"])
    proj = _projector(state)
    try:
        res = DevicePipeline(gpr, proj).peak_ensemble(xs, index, 8, seed=5, rng="device", stream=2)
        assert res.rng == "device" and res.names == ["event0", "event1", "event2"]
        assert _same(res, PeakEnsemble(gpr, proj).evaluate(xs, ranges, 8, seed=5, rng="device", stream=2))
    finally:
        proj.close()


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks(lib, ens3):
    ph = ens3.projector.handle
    out = DeviceBuffer(8 * K * 8 * 128)
    wbuf = DeviceBuffer(8 * 16)
    try:
        def normals(seed=1, stream=2, event=0, member0=0, members=8, pair=0, rows=65, tp=128, raw=0, zn=out.ptr):
            return lib.gprx_pca_normals_dev(ph, seed, stream, event, member0, members, pair, rows, tp, raw, zn)

        bad = {
            b"null": dict(zn=None),
            b"aligned": dict(zn=out.at(1)),
            b"positive": dict(members=0),
            b"positive ": dict(rows=0),
            b"below 2^31": dict(members=4096, rows=2**19, tp=2**19),
            b"smaller": dict(rows=65, tp=64),
            b"multiple of 64": dict(rows=65, tp=100),
            b"members must lie": dict(member0=-1),
            b"members must lie ": dict(member0=4090, members=7),
            b"event": dict(event=-1),
            b"pair_offset": dict(pair=-1),
            b"2 pair_offset": dict(pair=3, members=7),
            b"2 pair_offset ": dict(pair=4, member0=3, members=6),
        }
        for word, kw in bad.items():
            assert normals(**kw) == GPRX_EINVAL, kw
            assert word.strip() in lib.gprx_pca_last_error(ph), (kw, lib.gprx_pca_last_error(ph))
        assert lib.gprx_pca_normals_dev(None, 1, 2, 0, 0, 8, 0, 65, 128, 0, out.ptr) == GPRX_EINVAL
        tr = lib.gprx_pca_normal_transform_dev
        assert tr(ph, None, 16, out.ptr) == GPRX_EINVAL and tr(ph, wbuf.ptr, 16, None) == GPRX_EINVAL
        assert tr(ph, wbuf.ptr, 0, out.ptr) == GPRX_EINVAL and tr(ph, wbuf.ptr, 2**31, out.ptr) == GPRX_EINVAL
        assert tr(None, wbuf.ptr, 16, out.ptr) == GPRX_EINVAL
        # the handle is still usable: the limits themselves pass and give the mirror's words
        assert normals(member0=4088, members=8, pair=2048, raw=1) == GPRX_OK
        check(lib.gprx_pca_synchronize(ph))
        assert np.array_equal(out.to_array((K, 8, 128)).view(np.uint64), nn.words(1, 2, 0, K, 4088, 8, 65, 128, 2048))
        # the Python wrapper turns the same refusals into ValueError
        for kw in (dict(member0=-1), dict(members=0), dict(rows=0), dict(seed=-1), dict(stream=2**64), dict(antithetic=True, members=3),
                   dict(antithetic=True, member0=2), dict(antithetic=2, members=5), dict(member0=4095, members=2)):
            args = {"members": 4, "rows": 5, **kw}
            with pytest.raises(ValueError):
                ens3.normals_dev(0, args.pop("members"), args.pop("rows"), **args)
        assert _draw(ens3, 0, 4, 5).shape == (K, 4, 64)
    finally:
        out.free()
        wbuf.free()
