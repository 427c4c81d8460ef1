"""CPU pins of the ensemble verification: the numpy mirror (ensemble_verify_numpy.py) against the definition of the CRPS, the mirror's
invariants, the host aggregations of ``gpras_amd.ensemble.PeakVerification`` on hand-built integer maps, and the host-side argument checks.

The bound.  ``U = 2**-53``, ``gamma(m) = m U / (1 - m U)`` (Higham, Accuracy and Stability, section 3.1), as in test_gpu_ensemble.py.  The
mirror's CRPS is ``(2 acc) / (S S)`` with ``acc`` a sum of S non-negative terms, each a rounded difference times an exact weight, rounded:
two roundings per term, S - 1 for the additions, none for the doubling and for ``S S``, one for the division -- S + 2 roundings on a sum
without cancellation, so ``|crps - exact| <= gamma(S + 4) exact`` holds with room."""

import numpy as np
import pytest

import ensemble_verify_numpy as ev
from gpras_amd import ensemble as ge

U = 2.0**-53


def gamma(m: int):
    return np.longdouble(m * U) / (1 - np.longdouble(m * U))


def _members(S, kind, rng):
    if kind == "continuous":
        return rng.normal(size=S) * 3.0
    if kind == "ties":
        return np.round(rng.uniform(0.0, 4.0, size=S))  # integers 0 .. 4: many duplicates
    return np.maximum(rng.normal(size=S), 0.0)  # a dry share at exactly zero


@pytest.mark.parametrize("S", [1, 2, 3, 64, 257])
@pytest.mark.parametrize("kind", ["continuous", "ties", "clamped"])
def test_mirror_against_the_definition(S, kind):
    rng = np.random.default_rng(S * 7 + len(kind))
    x = _members(S, kind, rng)
    srt = np.sort(x)
    # below all, above all, between, equal to a member (the smallest, a middle one, the largest), zero
    ys = [srt[0] - 1.5, srt[-1] + 2.25, 0.5 * (srt[0] + srt[-1]) + 0.0123, srt[0], srt[S // 2], srt[-1], 0.0]
    peak = np.repeat(x[:, None], len(ys), axis=1)
    got = ev.verify_peaks(peak, np.array(ys))
    for c, y in enumerate(ys):
        exact = ev.crps_definition(x, y)
        err = abs(np.longdouble(got["crps"][c]) - exact)
        print(f"S={S} {kind} y={y:+.4f}: crps {got['crps'][c]:.17g}, |err| / exact = {float(err / exact) if exact else 0.0:.3e}")
        assert exact >= 0 and err <= gamma(S + 4) * exact
        assert got["below"][c] == np.sum(x < y) and got["equal"][c] == np.sum(x == y)
    assert got["equal"][3] >= 1 and got["equal"][4] >= 1 and got["equal"][5] >= 1
    assert got["below"][0] == 0 and got["below"][1] == S and got["equal"][0] == got["equal"][1] == 0


def test_mirror_nan_cells_and_infinities():
    S = 5
    rng = np.random.default_rng(1)
    peak = rng.normal(size=(S, 6))
    obs = np.zeros(6)
    peak[2, 1] = np.nan  # a NaN member
    obs[2] = np.nan  # a NaN observation
    peak[0, 3] = np.inf  # an infinite member, a finite observation
    peak[1, 4], obs[4] = np.inf, np.inf  # inf - inf
    peak[4, 5] = -np.inf
    ranks = np.array([0, S - 1])
    got = ev.verify_peaks(peak, obs, ranks)
    assert np.isnan(got["crps"][[1, 2]]).all() and got["below"][[1, 2]].tolist() == [-1, -1] and got["equal"][[1, 2]].tolist() == [-1, -1]
    assert np.isnan(got["order"][1, 1]) and got["order"][0, 1] == np.nanmin(peak[:, 1])  # the order statistics keep the key order, NaN last
    assert np.isfinite(got["crps"][0]) and got["below"][0] >= 0
    assert got["crps"][3] == np.inf and got["below"][3] == np.sum(peak[:, 3] < 0.0) and got["equal"][3] == 0
    assert np.isnan(got["crps"][4]) and got["below"][4] == S - 1 and got["equal"][4] == 1  # |inf - inf|: a NaN CRPS, the counts stay counts
    assert got["crps"][5] == np.inf and got["order"][0, 5] == -np.inf
    # -0 and +0 compare equal and sort -0 first
    z = ev.verify_peaks(np.array([[0.0], [-0.0], [0.0], [-0.0]]), np.array([-0.0]), np.arange(4))
    assert z["equal"][0] == 4 and z["below"][0] == 0 and z["crps"][0] == 0.0
    assert np.signbit(z["order"][:, 0]).tolist() == [True, True, False, False]


@pytest.mark.parametrize("S", [2, 3, 64, 257])
def test_mirror_permutation_gives_equal_bits(S):
    rng = np.random.default_rng(S)
    peak = rng.normal(size=(S, 9))
    peak[:, 1] = np.round(peak[:, 1])
    peak[::2, 2] = 0.0
    obs = rng.normal(size=9)
    obs[1], obs[2] = 1.0, 0.0
    ranks = np.array([0, S // 2, S - 1])
    want = ev.verify_peaks(peak, obs, ranks)
    for seed in range(3):
        got = ev.verify_peaks(peak[np.random.default_rng(seed).permutation(S)], obs, ranks)
        for key in want:
            assert np.array_equal(got[key].view(np.uint64) if got[key].dtype == np.float64 else got[key],
                                  want[key].view(np.uint64) if want[key].dtype == np.float64 else want[key]), key


# ---- PeakVerification on hand-built maps -----------------------------------------------------------------------------------------------
def _verification(below, equal, members, observed=None, thresholds=(), exceed=None, crps=None):
    below, equal = np.asarray(below, dtype=np.int32), np.asarray(equal, dtype=np.int32)
    ne, cells = below.shape
    thr = np.asarray(thresholds, dtype=np.float64)
    return ge.PeakVerification(np.zeros((ne, cells)) if crps is None else np.asarray(crps, dtype=np.float64), below, equal,
                               np.zeros((ne, cells)) if observed is None else np.asarray(observed, dtype=np.float64), members, thr,
                               np.zeros((ne, thr.size, cells), dtype=np.int32) if exceed is None else np.asarray(exceed, dtype=np.int32))


def test_rank_histogram_without_ties_is_a_bincount():
    S, cells = 7, 200
    rng = np.random.default_rng(0)
    below = rng.integers(0, S + 1, size=(3, cells))
    v = _verification(below, np.zeros_like(below), S)
    hist = v.rank_histogram()
    assert hist.shape == (3, S + 1)
    for e in range(3):
        assert np.array_equal(hist[e], np.bincount(below[e], minlength=S + 1))
    mask = rng.uniform(size=(3, cells)) < 0.5
    for e in range(3):
        assert np.array_equal(v.rank_histogram(mask)[e], np.bincount(below[e][mask[e]], minlength=S + 1))


def test_rank_histogram_with_ties():
    S = 4
    #        cell:   0  1  2  3  4   5   6
    below = np.array([[0, 1, 4, 0, 2, -1, 0]])
    equal = np.array([[0, 1, 0, 4, 2, -1, 3]])  # cell 3: truth and every member coincide (dropped by default); cell 5: NaN
    v = _verification(below, equal, S)
    hist = v.rank_histogram()
    want = np.zeros(S + 1)
    want[0] += 1.0
    want[1:3] += 0.5
    want[4] += 1.0
    want[2:5] += 1.0 / 3.0
    want[0:4] += 0.25
    np.testing.assert_allclose(hist[0], want, rtol=4 * U, atol=0)
    np.testing.assert_allclose(hist.sum(axis=1), [5.0], rtol=8 * U, atol=0)  # the counted cells: 7 less the all-equal and the NaN cell
    every = v.rank_histogram(mask=np.ones(7, dtype=bool))  # an explicit mask keeps the all-equal cell, never the NaN cell
    np.testing.assert_allclose(every.sum(axis=1), [6.0], rtol=8 * U, atol=0)
    np.testing.assert_allclose(every[0] - hist[0], np.full(S + 1, 0.2), rtol=0, atol=8 * U)
    # a larger random case: the rows sum to the counted cells
    rng = np.random.default_rng(2)
    S, cells = 64, 5000
    b = rng.integers(0, S + 1, size=(2, cells))
    q = np.minimum(rng.integers(0, 6, size=(2, cells)) * rng.integers(0, 2, size=(2, cells)), S - b)
    q[0, :10], b[0, :10] = S, 0
    v = _verification(b, q, S)
    counted = (q < S).sum(axis=1)
    np.testing.assert_allclose(v.rank_histogram().sum(axis=1), counted, rtol=cells * U, atol=0)


def test_reliability_brier_coverage_and_mean_crps():
    S = 4
    thr = (0.5, 1.0)
    #         cell:      0    1    2    3    4    5     6
    observed = np.array([[0.0, 0.7, 2.0, 0.5, 1.5, 9.0, 0.2]])
    exceed = np.array([[[0, 1, 2, 3, 4, 4, 2],     # counts of peak > 0.5
                        [0, 0, 4, 0, 2, 4, 2]]])   # counts of peak > 1.0
    below = np.array([[0, 2, 4, 1, 3, -1, 0]])
    equal = np.array([[4, 0, 0, 1, 0, -1, 1]])
    crps = np.array([[0.0, 0.25, 1.0, 0.5, 0.125, np.nan, 2.0]])
    v = _verification(below, equal, S, observed, thr, exceed, crps)
    assert v.valid.tolist() == [[True, True, True, True, True, False, True]]
    # reliability, 2 bins: bin = min(1, count * 2 // 4); the NaN cell 5 is left out
    rel = v.reliability(bins=2)
    assert rel.dtype == np.int64 and rel.shape == (1, 2, 2, 2)
    # threshold 0.5: bins [0, 0, 1, 1, 1, 1] of cells 0-4, 6; observed > 0.5: cells 1, 2, 4 (0.5 itself is not above)
    assert rel[0, 0].tolist() == [[2, 1], [4, 2]]
    # threshold 1.0: bins [0, 0, 1, 0, 1, 1]; observed > 1.0: cells 2, 4
    assert rel[0, 1].tolist() == [[3, 0], [3, 2]]
    rel4 = v.reliability(bins=4)  # bin = min(3, count): the count 4 shares the last bin with 3
    assert rel4[0, 0, :, 0].tolist() == [1, 1, 2, 2] and rel4[0, 0, :, 1].tolist() == [0, 1, 1, 1]
    assert rel4.sum(axis=2)[0, :, 0].tolist() == [6, 6]
    # Brier: p in {0, 1/4, 1/2, 3/4, 1}, all exact
    p = exceed[0][:, [0, 1, 2, 3, 4, 6]] / 4.0
    o = np.array([[0, 1, 1, 0, 1, 0], [0, 0, 1, 0, 1, 0]], dtype=np.float64)
    assert np.array_equal(v.brier()[0], ((p - o) ** 2).mean(axis=1))
    areas = np.array([1.0, 2.0, 1.0, 4.0, 1.0, 100.0, 1.0])
    a = areas[[0, 1, 2, 3, 4, 6]]
    assert np.array_equal(v.brier(cell_areas=areas)[0], ((p - o) ** 2 * a).sum(axis=1) / a.sum())
    # mean CRPS: the NaN cell is not valid and stays out
    assert v.mean_crps()[0] == (0.0 + 0.25 + 1.0 + 0.5 + 0.125 + 2.0) / 6.0
    assert v.mean_crps(cell_areas=areas)[0] == (0.5 + 1.0 + 2.0 + 0.125 + 2.0) / 10.0
    assert v.mean_crps(mask=np.array([True, True, False, False, False, True, False]))[0] == 0.125
    # coverage of [x_(1), x_(2)]: below + equal >= 2 and below <= 2 -> cells 0 (4 equal), 1, 3; of the 6 valid cells
    assert v.coverage(1, 2)[0] == 3.0 / 6.0
    assert v.coverage(0, 3)[0] == 5.0 / 6.0  # the whole range [x_(0), x_(3)]: only cell 2, above every member, lies outside
    with pytest.raises(ValueError):
        v.coverage(2, 1)
    with pytest.raises(ValueError):
        v.coverage(0, 4)
    with pytest.raises(ValueError):
        v.reliability(bins=0)
    with pytest.raises(ValueError):
        v.brier(cell_areas=np.ones(3))


def test_brier_on_zero_half_one():
    S = 2
    exceed = np.array([[[0, 1, 2, 0, 1, 2]]])
    observed = np.array([[0.0, 0.0, 0.0, 1.0, 1.0, 1.0]])
    v = _verification(np.zeros((1, 6)), np.zeros((1, 6)), S, observed, (0.5,), exceed)
    assert v.brier()[0, 0] == (0.0 + 0.25 + 1.0 + 1.0 + 0.25 + 0.0) / 6.0
    assert v.brier(mask=np.array([True, False, False, False, False, True]))[0, 0] == 0.0
    assert v.brier(mask=np.array([False, True, False, False, True, False]))[0, 0] == 0.25


# ---- argument checks ------------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    rk = ge.check_verify_args(17, [0, 16])
    assert rk.dtype == np.int32 and rk.tolist() == [0, 16]
    assert ge.check_verify_args(1, ()).size == 0
    for members, ranks in ((0, ()), (4097, ()), (4, [4]), (4, [-1]), (4, np.arange(9) % 4), (4, [0.5])):
        with pytest.raises(ValueError):
            ge.check_verify_args(members, ranks)
    ok = ge.check_observed(np.zeros((5, 3), dtype=np.float32), 5, 3)
    assert ok.dtype == np.float64 and ok.shape == (5, 3) and ok.flags.c_contiguous
    for bad in (np.zeros((4, 3)), np.zeros((5, 4)), np.zeros(15), np.zeros((1, 5, 3))):
        with pytest.raises(ValueError):
            ge.check_observed(bad, 5, 3)
    res_fields = ge.EnsembleResult.__dataclass_fields__
    assert res_fields["verification"].default is None and "verify" not in ge.STAGES
