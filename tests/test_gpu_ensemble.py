"""Peak ensembles on the GPU (gpras_amd.ensemble, csrc/ensemble.h, csrc/gp_joint.h) against the numpy mirror (ensemble_numpy.py): the joint
predictive covariance and its padded Cholesky factor, the draws, the fused peak kernel against ``route="refield"`` and the mirror bit for
bit, the tie to ``gprx_pca_sweep_dev``, the statistics over the members, ``DevicePipeline.peak_ensemble`` end to end and the argument checks.

Bounds.  ``U = 2**-53``, ``gamma(m) = m U / (1 - m U)`` (Higham, Accuracy and Stability, section 3.1).  A product ``Zn Lc^T`` of inner length
``Tp`` summed in any order satisfies ``|fl(Zn Lc^T) - Zn Lc^T| <= gamma(Tp) |Zn| |Lc^T|`` (section 3.5); adding the mean is one more
rounding, granted as ``eps |mean|`` with ``eps = 2 U``.  A Cholesky factor satisfies ``|C - Lc Lc^T| <= gamma(Tp + 1) |Lc| |Lc^T|`` (theorem 10.3), the
bound test_gpu_potrf_batched.py uses.  The covariance bound ``1e-8 (variance + noise)`` is the relative bound test_gpu_sgpr.py puts on the predict."""

import ctypes as C

import numpy as np
import pytest

import ensemble_numpy as en
import sweep_numpy as sn
from gpras_amd._lib import GPRX_EINVAL, GPRX_OK, DeviceBuffer, check, ptr
from gpras_amd.synth import make_regression
from oracle import kernels as okn
from oracle import sgpr as osg
from oracle import transforms as otr

pytestmark = pytest.mark.gpu

U = 2.0**-53
EVENT_LENGTHS = (1, 63, 64, 65, 130)


def gamma(m: int):
    return np.longdouble(m * U) / (1 - np.longdouble(m * U))


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


# ---- 1. joint covariance ---------------------------------------------------------------------------------------------------------------
def _cells(n, d, m, count):
    """One synthetic fit-free state: data, and per cell a unit, hyperparameters and inducing inputs of its own."""
    x, y, xs = make_regression(n, d, n_outputs=3, n_test=max(EVENT_LENGTHS), config=5, unit=m)
    rng = np.random.default_rng(100 + m)
    cells = []
    for c in range(count):
        z = np.ascontiguousarray(x[rng.choice(n, m, replace=False)] + 1e-3 * rng.standard_normal((m, d)))
        variance, ls, noise = 1.2 - 0.2 * c, 0.85 + 0.1 * c, 0.08 + 0.02 * c
        wv, wl, wn = otr.unconstrain(variance, ls, noise)
        cells.append({"unit": c, "z": z, "variance": variance, "ls": ls, "noise": noise, "theta": np.array([wv, float(wl), wn])})
    return x, y, xs, cells


@pytest.mark.parametrize("kernel", okn.KERNEL_NAMES)
@pytest.mark.parametrize("m", [20, 64, 100])
def test_joint_covariance(lib, kernel, m):
    n, d = 300, 3
    x, y, xs_all, cells = _cells(n, d, m, 3)
    h = C.c_void_p()
    check(lib.gprx_create(0, n, d, m, okn.KERNEL_IDS[kernel], 0, C.byref(h)))
    bufs = []
    try:
        check(lib.gprx_set_data(h, ptr(x), ptr(y), y.shape[1]), h)
        for ns in EVENT_LENGTHS:
            xs = np.ascontiguousarray(xs_all[:ns])
            tp = (ns + 63) // 64 * 64
            dxs = DeviceBuffer.from_array(xs)
            bufs.append(dxs)
            for count in (1, 3):
                units = np.array([c["unit"] for c in cells[:count]], dtype=np.int32)
                thetas = np.ascontiguousarray(np.stack([c["theta"] for c in cells[:count]]))
                zs = np.ascontiguousarray(np.stack([c["z"] for c in cells[:count]]))
                dmean, dlc, dm2, dvar = (DeviceBuffer(8 * count * ns), DeviceBuffer(8 * count * tp * tp), DeviceBuffer(8 * count * ns),
                                         DeviceBuffer(8 * count * ns))
                bufs += [dmean, dlc, dm2, dvar]
                for include_noise in (1, 0):
                    check(lib.gprx_predict_joint_batch_dev(h, count, ptr(units), ptr(thetas), ptr(zs), dxs.ptr, ns, dmean.ptr, dlc.ptr, include_noise), h)
                    mean, lc = dmean.to_array((count, ns)), dlc.to_array((count, tp, tp))
                    check(lib.gprx_predict_batch_dev(h, count, ptr(units), ptr(thetas), ptr(zs), dxs.ptr, ns, dm2.ptr, dvar.ptr, include_noise), h)
                    check(lib.gprx_synchronize(h), h)
                    mean2, var = dm2.to_array((count, ns)), dvar.to_array((count, ns))
                    assert np.array_equal(mean, mean2)  # the same launches produce it
                    for c, cell in enumerate(cells[:count]):
                        _, cov = en.joint_covariance(kernel, x, y[:, cell["unit"]], cell["z"], cell["variance"], cell["ls"], cell["noise"], xs, bool(include_noise))
                        assert np.array_equal(lc[c], np.tril(lc[c]))
                        assert np.array_equal(lc[c, ns:, ns:], np.eye(tp - ns)) and not np.any(lc[c, ns:, :ns])
                        got = lc[c, :ns, :ns] @ lc[c, :ns, :ns].T
                        err = np.max(np.abs(got - cov))
                        print(f"{kernel} m={m} ns={ns} count={count} noise={include_noise} cell={c}: max |LcLc^T - C| = {err:.3e}")
                        assert err <= 1e-8 * (cell["variance"] + cell["noise"])
                        want = var[c] + (0.0 if include_noise else osg.JITTER * cell["variance"])
                        assert np.max(np.abs(np.diag(got) - want) / want) <= 1e-8
    finally:
        for b in bufs:
            b.free()
        lib.gprx_destroy(h)


def test_joint_covariance_many_cells(lib):
    """32 cells at Tp = 128: from 32 cells on a matrix of at most 256 rows is factorised by one workgroup per cell (``potrf_cells``), the
    branch a production call (one cell per mode) takes; the smaller batches above take the launch sequence."""
    kernel, n, d, m, ns, count = "Matern32", 300, 3, 20, 65, 32
    tp = 128
    x, y, xs_all, _ = _cells(n, d, m, 1)
    xs = np.ascontiguousarray(xs_all[:ns])
    rng = np.random.default_rng(9)
    cells = []
    for c in range(count):
        variance, ls, noise = 0.8 + 0.02 * c, 0.7 + 0.015 * c, 0.05 + 0.003 * c
        wv, wl, wn = otr.unconstrain(variance, ls, noise)
        cells.append({"unit": c % 3, "variance": variance, "ls": ls, "noise": noise, "theta": np.array([wv, float(wl), wn]),
                      "z": np.ascontiguousarray(x[rng.choice(n, m, replace=False)] + 1e-3 * rng.standard_normal((m, d)))})
    units = np.array([c["unit"] for c in cells], dtype=np.int32)
    thetas = np.ascontiguousarray(np.stack([c["theta"] for c in cells]))
    zs = np.ascontiguousarray(np.stack([c["z"] for c in cells]))
    h = C.c_void_p()
    check(lib.gprx_create(0, n, d, m, okn.KERNEL_IDS[kernel], 0, C.byref(h)))
    bufs = [DeviceBuffer.from_array(xs), DeviceBuffer(8 * count * ns), DeviceBuffer(8 * count * tp * tp), DeviceBuffer(8 * count * ns), DeviceBuffer(8 * count * ns)]
    dxs, dmean, dlc, dm2, dvar = bufs
    try:
        check(lib.gprx_set_data(h, ptr(x), ptr(y), y.shape[1]), h)
        for include_noise in (1, 0):
            check(lib.gprx_predict_joint_batch_dev(h, count, ptr(units), ptr(thetas), ptr(zs), dxs.ptr, ns, dmean.ptr, dlc.ptr, include_noise), h)
            mean, lc = dmean.to_array((count, ns)), dlc.to_array((count, tp, tp))
            check(lib.gprx_predict_batch_dev(h, count, ptr(units), ptr(thetas), ptr(zs), dxs.ptr, ns, dm2.ptr, dvar.ptr, include_noise), h)
            check(lib.gprx_synchronize(h), h)
            assert np.array_equal(mean, dm2.to_array((count, ns)))
            var = dvar.to_array((count, ns))
            worst = 0.0
            for c, cell in enumerate(cells):
                _, cov = en.joint_covariance(kernel, x, y[:, cell["unit"]], cell["z"], cell["variance"], cell["ls"], cell["noise"], xs, bool(include_noise))
                assert np.array_equal(lc[c], np.tril(lc[c]))
                assert np.array_equal(lc[c, ns:, ns:], np.eye(tp - ns)) and not np.any(lc[c, ns:, :ns])
                got = lc[c, :ns, :ns] @ lc[c, :ns, :ns].T
                worst = max(worst, float(np.max(np.abs(got - cov))))
                assert np.max(np.abs(got - cov)) <= 1e-8 * (cell["variance"] + cell["noise"])
                want = var[c] + (0.0 if include_noise else osg.JITTER * cell["variance"])
                assert np.max(np.abs(np.diag(got) - want) / want) <= 1e-8
            print(f"32 cells, noise={include_noise}: max |LcLc^T - C| = {worst:.3e}")
    finally:
        for b in bufs:
            b.free()
        lib.gprx_destroy(h)


# ---- 2. draws ----------------------------------------------------------------------------------------------------------------------------
def _random_factors(k, rows, seed):
    """Per mode a mean (rows,), a random correlated covariance (rows, rows) and its padded lower factor (Tp, Tp)."""
    rng = np.random.default_rng(seed)
    tp = (rows + 63) // 64 * 64
    mean = rng.normal(size=(k, rows))
    cov = np.zeros((k, rows, rows))
    lc = np.zeros((k, tp, tp))
    for kk in range(k):
        a = rng.normal(size=(rows, rows + 3))
        cov[kk] = a @ a.T / rows + 0.05 * np.eye(rows)
        lc[kk] = en.padded_cholesky(cov[kk], tp)
    return mean, cov, lc, tp


@pytest.mark.parametrize("rows", [1, 63, 65, 130])
def test_draws(lib, rows):
    k = 3
    state, *_ = sn.make_case(40, k, [rows], "wse", seed=3)
    proj = _projector(state)
    ens = _ensemble(proj)
    mean, cov, lc, tp = _random_factors(k, rows, seed=rows)
    dmean, dzero, dlc = DeviceBuffer.from_array(mean), DeviceBuffer.from_array(np.zeros_like(mean)), DeviceBuffer.from_array(lc)
    try:
        def scores_of(zn, mean_dev=dmean):
            buf = ens.scores_dev(mean_dev, dlc, zn, zn.shape[1], rows)
            try:
                return buf.to_array((zn.shape[1], rows, k))
            finally:
                buf.free()

        # Zn = I per mode, S = T_e, zero mean: member s is w_s = column s of Lc, and the sum of w_s w_s^T reproduces C to the componentwise
        # bound of the factorisation (the sum itself is taken in longdouble here)
        eye = np.ascontiguousarray(np.broadcast_to(np.eye(rows), (k, rows, rows)))
        w = scores_of(eye, dzero)
        for kk in range(k):
            lk = lc[kk, :rows, :rows]
            wk = w[:, :, kk].astype(np.longdouble)  # wk[s, t] = Lc[t, s]
            got = wk.T @ wk
            bound = gamma(tp + 1) * (np.abs(lk) @ np.abs(lk.T)).astype(np.longdouble)
            assert np.all(np.abs(got - cov[kk]) <= bound)
        # Zn = 0: every member's scores are the mean, bit for bit
        got = scores_of(np.zeros((k, 5, rows)))
        assert np.array_equal(got, np.broadcast_to(mean.T[None, :, :], got.shape))
        # random Zn against numpy in longdouble: gamma(Tp) |Zn| |Lc^T| + eps |mean|, eps = 2 U
        zn = np.random.default_rng(rows + 1).standard_normal((k, 7, rows))
        got = scores_of(zn)
        for kk in range(k):
            lk = lc[kk, :rows, :rows].astype(np.longdouble)
            prod = zn[kk].astype(np.longdouble) @ lk.T
            want = mean[kk].astype(np.longdouble)[None, :] + prod
            bound = gamma(tp) * (np.abs(zn[kk]) @ np.abs(lc[kk, :rows, :rows].T)) + 2 * U * np.abs(mean[kk])[None, :]
            assert np.all(np.abs(got[:, :, kk] - want) <= bound)
    finally:
        for b in (dmean, dzero, dlc):
            b.free()
        proj.close()


# ---- 3. fused equals refield equals the mirror, bit for bit ----------------------------------------------------------------------------------
PEAK_CASES = {
    # cells, K, rows, S, hp, weighted, dry
    "one_cell_one_mode": (1, 1, 1, 1, "wse", False, ()),
    "k7_wse": (255, 7, 31, 2, "wse", True, (3, 200)),
    "k16_depth": (257, 16, 32, 5, "depth", True, (0, 256)),
    "k17_velocity": (300, 17, 33, 17, "velocity", False, ()),
    "k64_depth": (300, 64, 65, 5, "depth", True, (7, 8, 299)),
    "k64_wse_unweighted": (257, 64, 33, 2, "wse", False, (100,)),
}


def _peak_case(name):
    cells, k, rows, members, hp, weighted, dry = PEAK_CASES[name]
    state, *_ = sn.make_case(cells, k, [rows], hp, weighted=weighted, dry=dry, seed=len(name))
    scores = np.random.default_rng(cells + k).normal(size=(members, rows, k))
    return state, scores, members, rows


@pytest.mark.parametrize("name", list(PEAK_CASES))
def test_fused_equals_refield_equals_mirror(lib, name):
    state, scores, members, rows = _peak_case(name)
    proj = _projector(state)
    ens = _ensemble(proj)
    try:
        want = en.member_peaks(state, scores)

        def peaks(route, group=0):
            buf = ens.member_peaks_dev(scores, members, rows, route=route, member_group=group)
            try:
                return buf.to_array(want.shape)
            finally:
                buf.free()

        refield = peaks("refield")
        assert np.array_equal(refield, want)
        auto = C.c_int()
        check(lib.gprx_pca_ensemble_group(proj.handle, members, C.byref(auto)))
        assert 1 <= auto.value <= 16
        for group in [0, *range(1, 17), 64]:  # 0: the launcher's choice, one of 1 .. 16; every grouping gives the same bits
            assert np.array_equal(peaks("fused", group), refield), group
    finally:
        proj.close()


def test_refield_slabs_of_members(lib, monkeypatch):
    """The refield route in slabs of one and of two members (the slab size of ``gprx_pca_slab_rows`` forced down) gives the same bits."""
    import gpras_amd.ensemble as ge

    state, scores, members, rows = _peak_case("k17_velocity")
    proj = _projector(state)
    ens = _ensemble(proj)
    try:
        want = en.member_peaks(state, scores)
        for forced in (rows, 2 * rows + 1):
            monkeypatch.setattr(ge, "slab_rows", lambda pr, most_rows=None, forced=forced: forced)
            buf = ens.member_peaks_dev(scores, members, rows, route="refield")
            assert np.array_equal(buf.to_array(want.shape), want)
            buf.free()
    finally:
        proj.close()


@pytest.mark.parametrize("hp", ["wse", "depth", "velocity"])
def test_zero_draws_tie_to_the_sweep(lib, hp):
    """With zero draws every member's peak is the ``max_t y`` that ``gprx_pca_sweep_dev`` reports for the mean prediction at the full mode count."""
    from gpras_amd.sweep import ModeCountSweep

    k, rows = 17, 33
    state, mean, var, truth, ranges = sn.make_case(257, k, [rows], hp, seed=11)
    proj = _projector(state)
    ens = _ensemble(proj)
    res = ModeCountSweep(proj, [k]).evaluate(mean, None, sn.truth_in_metric_space(state, truth), ranges, route="fused")
    try:
        y_peak = res.summary(k, 0).y_peak
        scores = np.ascontiguousarray(np.broadcast_to(mean[None, :, :], (3, rows, k)))
        for route in ("fused", "refield"):
            buf = ens.member_peaks_dev(scores, 3, rows, route=route)
            peak = buf.to_array((3, 257))
            buf.free()
            assert np.array_equal(peak, np.broadcast_to(y_peak, peak.shape))
    finally:
        res.close()
        proj.close()


# ---- 4. statistics ---------------------------------------------------------------------------------------------------------------------------
def _stats_peaks(members, cells, seed=0):
    rng = np.random.default_rng(seed)
    peak = rng.uniform(0.0, 1.0, size=(members, cells))
    peak[:, 1] = 0.5  # every member exactly on the threshold
    peak[::2, 2] = 0.5  # half of them
    peak[:, 3] = np.repeat(rng.uniform(0.0, 1.0, size=(members + 2) // 3), 3)[:members]  # ties
    peak[:, 4] = 0.0
    peak[1:, 5] = np.round(peak[1:, 5], 1)  # many ties
    return peak


@pytest.mark.parametrize("members,cells", [(1, 5), (17, 300), (64, 257), (255, 40)])
def test_member_statistics(lib, members, cells):
    state, *_ = sn.make_case(cells, 2, [2], "wse", seed=1)
    proj = _projector(state)
    ens = _ensemble(proj)
    peak = _stats_peaks(members, max(cells, 6))[:, :cells]
    thr = np.array([0.5, 0.0, 0.25, 0.9, 2.0])
    ranks = np.array(sorted({0, members // 4, members // 2, members - 1}), dtype=np.int32)
    areas = np.random.default_rng(7).uniform(10.0, 400.0, size=cells)
    dpeak = DeviceBuffer.from_array(peak)
    try:
        got = ens.member_stats(dpeak, members, thr, ranks)
        want = en.member_stats(peak, thr, ranks)
        assert np.array_equal(got["exceed"], want["exceed"]) and got["exceed"].dtype == np.int32
        assert np.array_equal(got["order"], want["order"])
        assert np.array_equal(got["order"], np.sort(peak, axis=0)[ranks])
        assert np.array_equal(got["mean"], want["mean"]) and np.array_equal(got["std"], want["std"])
        np.testing.assert_allclose(got["mean"], np.mean(peak, axis=0), rtol=1e-13, atol=0)
        np.testing.assert_allclose(got["std"], np.std(peak, axis=0), rtol=1e-13, atol=0)
        counts = np.stack([(peak > t).sum(axis=1) for t in thr], axis=1)
        assert np.array_equal(got["wet_area"], counts.astype(np.float64))  # area = NULL: exact cell counts
        with_area = ens.member_stats(dpeak, members, thr, ranks, cell_areas=areas)
        again = ens.member_stats(dpeak, members, thr, ranks, cell_areas=areas)
        ref = np.stack([((peak > t) * areas).sum(axis=1) for t in thr], axis=1)
        np.testing.assert_allclose(with_area["wet_area"], ref, rtol=1e-12, atol=0)
        assert np.array_equal(with_area["wet_area"], again["wet_area"])
        assert np.array_equal(with_area["exceed"], got["exceed"])
        # no thresholds, no ranks: the moments alone
        bare = ens.member_stats(dpeak, members)
        assert np.array_equal(bare["mean"], got["mean"]) and bare["exceed"].shape == (0, cells) and bare["order"].shape == (0, cells)
    finally:
        dpeak.free()
        proj.close()


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    """A small fitted GPRAS (N = 200, K = 3, M = 10), its projector over 40 cells and test inputs of 3 events."""
    from gpras_amd.gpr import GPRAS

    k, cells, d = 3, 40, 4
    state, *_ = sn.make_case(cells, k, [5], "wse", seed=21)
    x, y, xs = make_regression(200, d, n_outputs=k, n_test=60, config=9)
    gpr = GPRAS("RBF")
    gpr.fit(x, y, 10, "kmeans", "adam", max_iter=5)
    ranges = [(0, 7), (7, 40), (40, 60)]
    return gpr, state, xs, ranges


def _index(ranges):
    import pandas as pd

    return pd.MultiIndex.from_tuples([(f"event{e}", t) for e, (lo, hi) in enumerate(ranges) for t in range(hi - lo)], names=["event", "timestep"])


def test_pipeline_peak_ensemble(lib, fitted):
    """Every output of ``DevicePipeline.peak_ensemble`` against the mirror run on the same normals, stage by stage on what the device leaves:
    the factor against the mirror's covariance at the covariance bound; the scores against the mirror's packing of the DOWNLOADED mean and
    factor at the draw bound ``gamma(Tp) |Zn| |Lc^T| + eps |mean|``; the peaks bit for bit against the mirror's chain on the downloaded
    scores; the statistics on the downloaded peaks exactly (counts, order statistics, mean and std bit for bit, the wet area an exact count
    without areas and within 1e-12 with them).  The pipeline's own outputs are then those statistics, bit for bit, for both routes."""
    from gpras_amd.ensemble import PeakEnsemble, padded_rows
    from gpras_amd.pipeline import DevicePipeline

    gpr, state, xs, ranges = fitted
    members, thr, quantiles = 8, (0.5, 1.0), (0.0, 0.5, 1.0)
    k, cells = len(gpr.models), 40
    rng = np.random.default_rng(5)
    normals = [rng.standard_normal((k, members, hi - lo)) for lo, hi in ranges]
    areas = np.random.default_rng(6).uniform(50.0, 150.0, size=cells)
    ranks = en.quantile_ranks(quantiles, members)
    proj = _projector(state)
    try:
        pipe = DevicePipeline(gpr, proj)
        ens = PeakEnsemble(gpr, proj)
        res = {(route, with_areas): pipe.peak_ensemble(xs, _index(ranges), members, thresholds=thr, quantiles=quantiles, normals=normals,
                                                       cell_areas=areas if with_areas else None, route=route)
               for route in ("fused", "refield") for with_areas in (True, False)}
        a = res[("fused", True)]
        assert a.route == "fused" and res[("refield", True)].route == "refield" and a.names == [f"event{e}" for e in range(len(ranges))]
        assert set(a.last_timings_ms) >= {"joint", "draw_upload", "draws", "peaks", "stats", "total", "device_peaks"}
        for e, (lo, hi) in enumerate(ranges):
            rows, tp = hi - lo, padded_rows(hi - lo)
            # 1. the joint prediction the pipeline runs, downloaded, against the mirror
            mean_dev, lc_dev, _ = ens.joint_dev(xs[lo:hi])
            scores_dev = peak_dev = None
            try:
                mean, lc = mean_dev.to_array((k, rows)), lc_dev.to_array((k, tp, tp))
                for kk, mod in enumerate(gpr.models):
                    mu, cov = en.joint_covariance(gpr.kernel_str, gpr.x, gpr.y[:, mod.unit], mod.Z, mod.variance, mod.lengthscales, mod.noise, xs[lo:hi], True)
                    assert np.max(np.abs(mean[kk] - mu)) <= 1e-8 * np.max(np.abs(mu))
                    got = lc[kk, :rows, :rows] @ lc[kk, :rows, :rows].T
                    assert np.max(np.abs(got - cov)) <= 1e-8 * (mod.variance + mod.noise)
                    assert np.array_equal(lc[kk], np.tril(lc[kk])) and np.array_equal(lc[kk, rows:, rows:], np.eye(tp - rows))
                # 2. the draws from the downloaded mean and factor
                scores_dev = ens.scores_dev(mean_dev, lc_dev, normals[e], members, rows)
                scores = scores_dev.to_array((members, rows, k))
                for kk in range(k):
                    lk = lc[kk, :rows, :rows].astype(np.longdouble)
                    want = mean[kk].astype(np.longdouble)[None, :] + normals[e][kk].astype(np.longdouble) @ lk.T
                    bound = gamma(tp) * (np.abs(normals[e][kk]) @ np.abs(lc[kk, :rows, :rows].T)) + 2 * U * np.abs(mean[kk])[None, :]
                    assert np.all(np.abs(scores[:, :, kk] - want) <= bound)
                # 3. the peaks of the downloaded scores, bit for bit, both routes
                want_peak = en.member_peaks(state, scores)
                for route in ("fused", "refield"):
                    peak_dev = ens.member_peaks_dev(scores_dev, members, rows, route=route)
                    assert np.array_equal(peak_dev.to_array((members, cells)), want_peak), route
                    peak_dev.free()
                    peak_dev = None
            finally:
                for buf in (mean_dev, lc_dev, scores_dev, peak_dev):
                    if buf is not None:
                        buf.free()
            # 4. every output of the pipeline is the mirror's statistic of those peaks
            st = en.member_stats(want_peak, thr, ranks, areas)
            st_unit = en.member_stats(want_peak, thr, ranks, None)
            for (route, with_areas), r in res.items():
                assert np.array_equal(r.exceed_counts[e], st["exceed"]) and np.array_equal(r.p_exceed[e], st["exceed"] / members), route
                assert np.array_equal(r.peak_quantiles[e], st["order"]), route
                assert np.array_equal(r.peak_quantiles[e], np.quantile(want_peak, quantiles, axis=0, method="lower")), route
                assert np.array_equal(r.peak_mean[e], st["mean"]) and np.array_equal(r.peak_std[e], st["std"]), route
                if with_areas:
                    np.testing.assert_allclose(r.wet_area[e], st["wet_area"], rtol=1e-12, atol=0)
                else:
                    assert np.array_equal(r.wet_area[e], st_unit["wet_area"]), route  # exact cell counts
            assert np.array_equal(res[("fused", True)].wet_area[e], res[("refield", True)].wet_area[e])
        pipe_kw = dict(thresholds=thr, quantiles=quantiles)
        # seeds: the same seed gives the same bits, another seed other peaks
        s1 = pipe.peak_ensemble(xs, _index(ranges), members, **pipe_kw, seed=3)
        s2 = pipe.peak_ensemble(xs, _index(ranges), members, **pipe_kw, seed=3)
        s3 = pipe.peak_ensemble(xs, _index(ranges), members, **pipe_kw, seed=4)
        assert np.array_equal(s1.peak_mean, s2.peak_mean) and np.array_equal(s1.peak_quantiles, s2.peak_quantiles) and np.array_equal(s1.wet_area, s2.wet_area)
        assert not np.array_equal(s1.peak_mean, s3.peak_mean)
        from gpras_amd.ensemble import DEFAULT_ROUTE

        assert s1.route == DEFAULT_ROUTE == "fused"  # the route profiles/ensemble_peaks.json shows faster
    finally:
        proj.close()


# ---- 6. argument checks ----------------------------------------------------------------------------------------------------------------------
def test_argument_checks(lib, fitted):
    from gpras_amd.ensemble import PeakEnsemble
    from gpras_amd.pipeline import DevicePipeline

    gpr, state, xs, ranges = fitted
    proj = _projector(state)
    ens = PeakEnsemble(gpr, proj)
    pipe = DevicePipeline(gpr, proj)
    try:
        # event ranges
        for bad in ([(7, 40), (0, 7)], [(0, 10), (5, 20)], [(0, 0)], [(0, 61)], []):
            with pytest.raises(ValueError):
                ens.evaluate(xs, bad, 4)
        with pytest.raises(ValueError):
            pipe.peak_ensemble(xs, _index(ranges)[:-1], 4)  # one index entry per row of x_test
        with pytest.raises(ValueError):
            ens.evaluate(xs, ranges, 4097)  # S > 4096
        with pytest.raises(ValueError):
            ens.evaluate(xs, ranges, 4, thresholds=np.arange(9.0))
        with pytest.raises(ValueError):
            ens.evaluate(xs, ranges, 4, quantiles=np.linspace(0, 1, 9))
        with pytest.raises(ValueError):
            ens.evaluate(xs, ranges, 4, route="other")
        with pytest.raises(ValueError):
            ens.evaluate(np.zeros((1100, xs.shape[1])), [(0, 1100)], 4)  # ns > 1024
        with pytest.raises(ValueError):
            ens.evaluate(xs, ranges, 4, normals=[np.zeros((3, 4, 2))] * 3)
        # the statistics' C checks, the handle still usable afterwards
        peak = DeviceBuffer.from_array(np.zeros((4, 40)))
        out = DeviceBuffer(8 * 40 * 64)
        thr9, rk = np.zeros(9), np.array([4], dtype=np.int32)
        ph = proj.handle

        def stats(members, n_thr, thr, n_rank, ranks):
            return lib.gprx_pca_member_stats_dev(ph, peak.ptr, members, n_thr, ptr(thr), n_rank, ptr(ranks), None, out.ptr, out.at(2000), out.at(2100),
                                                 out.at(2200), out.at(2400))

        assert stats(4097, 1, thr9, 0, rk) == GPRX_EINVAL
        assert stats(0, 1, thr9, 0, rk) == GPRX_EINVAL
        assert stats(4, 9, thr9, 0, rk) == GPRX_EINVAL
        assert stats(4, 1, thr9, 9, np.zeros(9, dtype=np.int32)) == GPRX_EINVAL
        assert stats(4, 1, thr9, 1, rk) == GPRX_EINVAL  # rank >= S
        assert stats(4, 1, np.array([np.nan]), 0, rk) == GPRX_EINVAL
        assert b"rank" in lib.gprx_pca_last_error(ph) or b"NaN" in lib.gprx_pca_last_error(ph)
        assert lib.gprx_pca_ensemble_peaks_dev(ph, peak.ptr, 0, 1, 1, 0, out.ptr) == GPRX_EINVAL
        assert lib.gprx_pca_ensemble_peaks_dev(ph, peak.ptr, 1, 1, 3, 0, out.ptr) == GPRX_EINVAL
        assert lib.gprx_pca_ensemble_peaks_dev(ph, peak.ptr, 1, 1, 1, 65, out.ptr) == GPRX_EINVAL
        assert lib.gprx_pca_ensemble_peaks_dev(ph, None, 1, 1, 1, 0, out.ptr) == GPRX_EINVAL
        assert lib.gprx_pca_member_peaks_dev(ph, peak.ptr, 65536, 1, out.ptr) == GPRX_EINVAL
        assert stats(4, 1, thr9, 1, np.array([3], dtype=np.int32)) == GPRX_OK  # still usable
        peak.free()
        out.free()
        # K > 64: no projector takes it
        big, *_ = sn.make_case(80, 65, [2], "wse", seed=2)
        with pytest.raises(ValueError):
            _projector(big)
    finally:
        proj.close()


def test_joint_argument_checks(lib):
    """GPRX_EINVAL before any device work, with its reason, and the handle still usable: exact model, ns > 1024, M > 320."""
    from gpras_amd.ensemble import joint_applies

    n, d = 400, 3
    x, y, xs = make_regression(n, d, n_outputs=1, n_test=8, config=2)
    theta = np.ascontiguousarray(np.array([*otr.unconstrain(1.0, 0.9, 0.1)], dtype=np.float64))
    units = np.zeros(1, dtype=np.int32)
    dxs, dmean, dlc = DeviceBuffer.from_array(xs), DeviceBuffer(8 * 1100), DeviceBuffer(8 * 64 * 64)
    try:
        for m, ns, word in ((0, 8, b"exact model"), (321, 8, b"320 inducing"), (10, 1025, b"1024"), (10, 0, b"1024")):
            h = C.c_void_p()
            check(lib.gprx_create(0, n, d, m, 0, 0, C.byref(h)))
            try:
                check(lib.gprx_set_data(h, ptr(x), ptr(y), 1), h)
                z = np.ascontiguousarray(x[: max(m, 1)])
                rc = lib.gprx_predict_joint_batch_dev(h, 1, ptr(units), ptr(theta), ptr(z), dxs.ptr, ns, dmean.ptr, dlc.ptr, 1)
                assert rc == GPRX_EINVAL and word in lib.gprx_last_error(h)
                if m == 10:  # still usable
                    assert lib.gprx_predict_joint_batch_dev(h, 1, ptr(units), ptr(theta), ptr(z), dxs.ptr, 8, dmean.ptr, dlc.ptr, 1) == GPRX_OK
            finally:
                lib.gprx_destroy(h)
        assert joint_applies(None, 3, 8) and joint_applies(321, 3, 8) and joint_applies(10, 65, 8) and joint_applies(10, 3, 1025)
        assert joint_applies(320, 64, 1024) is None
    finally:
        for b in (dxs, dmean, dlc):
            b.free()
