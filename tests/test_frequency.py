"""The depth-frequency maps without a device: the numpy mirror (frequency_numpy.py) against an independent definition in exact fractions,
the properties DESIGN.md section 3.26 states -- a rate that never rises with the level, a linear depth inside its bracket, step and linear
agreeing at a level, the edges of the inversion -- and the argument checks of ``gpras_amd.frequency`` and of ``evaluate(frequency=...)``."""

from fractions import Fraction

import numpy as np
import pytest

import frequency_numpy as fq
from gpras_amd import frequency as gf


def _catalogue(seed, members_from, n_events, cells, levels, exact_weights):
    """Peak blocks with ties at the levels, zeros of both signs and depths beyond both ends of the levels; weights ``j / 1024`` or random."""
    rng = np.random.default_rng(seed)
    peaks, weights = [], []
    for e in range(n_events):
        s = int(members_from[e % len(members_from)])
        peak = rng.uniform(levels[0] - 0.5, levels[-1] + 0.5, size=(s, cells))
        ties = rng.uniform(size=peak.shape) < 0.2
        peak[ties] = rng.choice(levels, size=int(ties.sum()))
        peak[rng.uniform(size=peak.shape) < 0.05] = -0.0
        peaks.append(peak)
        weights.append(int(rng.integers(0, 2048)) / 1024.0 if exact_weights else float(rng.uniform(0.0, 0.3)))
    return peaks, weights


def test_mirror_against_exact_fractions():
    """Weights ``j / 1024`` and members a power of two: every product and sum is exact, so the rate IS the rational ``sum w n / S``."""
    levels = np.array([0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0])
    cells = 9
    peaks, weights = _catalogue(0, (1, 2, 64, 256), 7, cells, levels, exact_weights=True)
    rate, nan_members = fq.accumulate(peaks, weights, levels)
    exact = [[Fraction(0) for _ in range(cells)] for _ in levels]
    for peak, w in zip(peaks, weights):
        for l, d in enumerate(levels):
            for c in range(cells):
                n = sum(1 for v in peak[:, c].tolist() if v > d)
                exact[l][c] += Fraction(w) * Fraction(n, peak.shape[0])
    assert all(Fraction(float(rate[l, c])) == exact[l][c] for l in range(levels.size) for c in range(cells))
    assert not nan_members.any()
    aep = np.array([1.0 / 1024, 0.25, 1.0, 3.5, 100.0])
    for interp in fq.INTERPS:
        _, bracket = fq.invert(rate, nan_members, levels, aep, interp)
        for j, p in enumerate(aep.tolist()):
            for c in range(cells):
                assert bracket[j, c] == sum(1 for l in range(levels.size) if exact[l][c] >= Fraction(p))


def test_rate_never_rises_with_the_level():
    levels = np.sort(np.random.default_rng(1).uniform(0.0, 4.0, size=40))
    peaks, weights = _catalogue(2, (1, 2, 3, 63, 64, 65, 257), 14, 50, levels, exact_weights=False)
    rate, _ = fq.accumulate(peaks, weights, levels)
    assert np.all(np.diff(rate, axis=0) <= 0.0) and np.all(rate >= 0.0) and not np.signbit(rate).any()


def test_zero_weight_and_member_order_change_no_bit():
    levels = np.linspace(0.0, 3.0, 13)
    peaks, weights = _catalogue(3, (3, 64, 65), 5, 20, levels, exact_weights=False)
    rate, nan_members = fq.accumulate(peaks, weights, levels)
    extra = np.random.default_rng(4).uniform(0.0, 3.0, size=(7, 20))
    with_zero, _ = fq.accumulate(peaks[:2] + [extra] + peaks[2:], weights[:2] + [0.0] + weights[2:], levels)
    shuffled, _ = fq.accumulate([p[np.random.default_rng(5).permutation(p.shape[0])] for p in peaks], weights, levels)
    assert np.array_equal(rate.view(np.uint64), with_zero.view(np.uint64)) and np.array_equal(rate.view(np.uint64), shuffled.view(np.uint64))
    assert not nan_members.any()


def test_linear_depth_lies_in_its_bracket():
    """Levels on a binary grid, so that ``d_k - d_{k-1}`` is exact: with ``0 <= f <= 1`` the rounded ``d_{k-1} + g f`` cannot leave ``[d_{k-1}, d_k]``."""
    levels = np.arange(0, 48) / 16.0
    peaks, weights = _catalogue(6, (1, 3, 64, 257), 12, 60, levels, exact_weights=False)
    rate, nan_members = fq.accumulate(peaks, weights, levels)
    aep = np.quantile(rate[rate > 0.0], np.linspace(0.02, 0.98, 16))
    depth, bracket = fq.invert(rate, nan_members, levels, aep, "linear")
    inside = (bracket > 0) & (bracket < levels.size)
    assert inside.any()
    k = bracket[inside]
    assert np.all(depth[inside] >= levels[k - 1]) and np.all(depth[inside] <= levels[k])
    step, bracket_step = fq.invert(rate, nan_members, levels, aep, "step")
    assert np.array_equal(bracket, bracket_step) and np.array_equal(step[inside], levels[k - 1])


def test_step_and_linear_agree_at_a_level():
    levels = np.linspace(0.0, 2.0, 9)
    peaks, weights = _catalogue(7, (2, 64), 6, 12, levels, exact_weights=False)
    rate, nan_members = fq.accumulate(peaks, weights, levels)
    hits = 0
    for c in range(12):
        for l in range(levels.size - 1):
            p = rate[l, c]
            if not p > rate[l + 1, c]:
                continue  # (a target equal to a repeated rate brackets at the last level that holds it)
            lin, k_lin = fq.invert(rate[:, c:c + 1], nan_members[c:c + 1], levels, [p], "linear")
            stp, k_stp = fq.invert(rate[:, c:c + 1], nan_members[c:c + 1], levels, [p], "step")
            assert k_lin[0, 0] == k_stp[0, 0] == l + 1 and lin[0, 0] == stp[0, 0] == levels[l]
            hits += 1
    assert hits > 20


def test_edges_of_the_inversion():
    levels = np.array([0.5, 1.0, 2.0])
    peak = np.array([[0.7, 3.0, 0.1, np.nan], [1.5, 2.5, 0.2, 1.0]])
    rate, nan_members = fq.accumulate([peak], [1.0], levels)
    assert rate[:, 0].tolist() == [1.0, 0.5, 0.0] and rate[:, 1].tolist() == [1.0, 1.0, 1.0] and rate[:, 2].tolist() == [0.0, 0.0, 0.0]
    assert nan_members.tolist() == [0, 0, 0, 1] and rate[:, 3].tolist() == [0.5, 0.0, 0.0]  # the NaN member exceeds nothing
    for interp in fq.INTERPS:
        depth, bracket = fq.invert(rate, nan_members, levels, [0.75], interp)
        assert bracket[0].tolist() == [1, 3, 0, -1]
        assert depth[0, 1] == np.inf and depth[0, 2] == -np.inf and np.isnan(depth[0, 3])
    lin, _ = fq.invert(rate, nan_members, levels, [0.75], "linear")
    assert lin[0, 0] == 0.75  # halfway between the rates 1.0 and 0.5: halfway between the levels 0.5 and 1.0
    one, k_one = fq.invert(rate[:1], nan_members, levels[:1], [0.75, 1.0, 2.0], "linear")  # a single level never interpolates
    assert k_one[:, 0].tolist() == [1, 1, 0] and one[:, 0].tolist() == [np.inf, np.inf, -np.inf]
    with pytest.raises(ValueError):
        fq.invert(rate, nan_members, levels, [0.5], "log")


# ---- the argument checks of gpras_amd.frequency ------------------------------------------------------------------------------------------
class _Projector:
    """What ``FrequencyMaps`` and ``PeakEnsemble`` read of a projector before they reach the device."""

    device, n_cells, spatial_mode_count = 0, 12, 2
    hydraulic_parameter, elevations = "velocity", None

    @property
    def handle(self):
        raise AssertionError("the check must come before the device is used")


class _Bare:
    def __init__(self, k):
        self.models = [None] * k


def test_levels_are_checked():
    for bad in ([1.0, 0.5], [0.5, 0.5], [0.0, np.inf], [np.nan], [], np.arange(257.0), np.zeros((2, 2))):
        with pytest.raises(ValueError):
            gf.check_levels(bad)
        with pytest.raises(ValueError):
            gf.FrequencyMaps(_Projector(), bad)
    assert gf.check_levels(np.arange(256.0)).size == 256 and gf.check_levels(0.5).tolist() == [0.5]
    fm = gf.FrequencyMaps(_Projector(), [0.0, 1.0])
    assert fm.n_events == 0 and fm.weights == [] and fm.rate().shape == (2, 12) and fm.nan_members().dtype == np.int32
    fm.close()


def test_weights_members_and_targets_are_checked():
    fm = gf.FrequencyMaps(_Projector(), [0.0, 1.0])
    peak = np.zeros((3, 12))
    for bad in (-1.0, np.nan, np.inf, -np.inf, "x"):
        with pytest.raises(ValueError):
            fm.add_peaks(peak, 3, bad)
    for members in (0, 4097):
        with pytest.raises(ValueError):
            fm.add_peaks(np.zeros((max(members, 1), 12)), members, 1.0)
    with pytest.raises(ValueError):
        fm.add_peaks(np.zeros((3, 11)), 3, 1.0)
    for bad in ([], np.full(17, 0.1), [0.0], [-0.1], [np.nan], [np.inf]):
        with pytest.raises(ValueError):
            fm.depth_at(bad)
    with pytest.raises(ValueError):
        fm.depth_at([0.1], interp="log")
    for bad in (None, [0.1], [0.1, 0.2, 0.3], [0.1, -0.2], [0.1, np.nan]):
        with pytest.raises(ValueError):
            gf.check_weights(bad, 2)
        with pytest.raises(ValueError):
            fm.add_field(np.zeros((4, 12)), [(0, 2), (2, 4)], bad)
    assert gf.check_weights([0.0, 2.5], 2).tolist() == [0.0, 2.5] and fm.n_events == 0 and fm.weights == []


def test_evaluate_checks_the_weights_first():
    from gpras_amd.ensemble import PeakEnsemble

    proj = _Projector()
    ens = PeakEnsemble(_Bare(2), proj)
    fm = gf.FrequencyMaps(proj, [0.0, 1.0])
    x, ranges = np.zeros((6, 3)), [(0, 2), (2, 6)]
    for bad in (None, [0.1], [0.1, 0.2, 0.3], [0.1, -1.0], [np.inf, 0.1]):
        with pytest.raises(ValueError, match="weight"):
            ens.evaluate(x, ranges, 4, frequency=fm, weights=bad)
    with pytest.raises(ValueError, match="weights"):
        ens.evaluate(x, ranges, 4, weights=[0.1, 0.2])  # weights with nothing to add them to

    class _Other(_Projector):
        n_cells = 13

    with pytest.raises(ValueError, match="cells"):
        ens.evaluate(x, ranges, 4, frequency=gf.FrequencyMaps(_Other(), [0.0, 1.0]), weights=[0.1, 0.2])
