"""Row N4: the k-means inducing-point initialisation of ``/root/reference/gpras/gpr.py:312-315``.
CPU: the oracle's restatement of scikit-learn's Lloyd loop against ``KMeans`` itself (the reference's call).
GPU: the device Lloyd iterations (``gprx_kmeans_lloyd``) against the same ``KMeans`` call, centres <= 1e-12.

The kernels' branches one by one are in test_gpu_kmeans_kernels.py: the same end-to-end bound at the shapes where the E-step takes
a second LDS pass, d up to 64 and n > 65536; the Lloyd driver bit for bit against ``oracle.kmeans.lloyd`` on lattice data with exact
ties, each stopping rule alone; the seeding driver index for index against ``kmeans_numpy.kmeans_pp_replay`` on chosen draws; the
empty-cluster flag and the fallback.  What those tests need from their inputs is checked here without a GPU: the replay equals
scikit-learn's own ``kmeans_plusplus`` on the ``RandomState(0)`` draws, the seeding inputs are >= 1e-10 from an outcome decided
by rounding, the lattice inputs converge with no empty cluster, and the oracle equals ``KMeans`` on the new shapes."""

import numpy as np
import pytest
from sklearn.cluster import KMeans

import kmeans_numpy as kn
import test_gpu_kmeans_kernels as gk
from gpras_amd.synth import make_hydrograph_features, make_regression
from oracle import kmeans as okm

CASES = [(256, 4, 32, "reg"), (1000, 8, 50, "reg"), (4096, 10, 50, "reg"), (1500, 10, 300, "reg"), (700, 3, 20, "hydro"), (64, 2, 1, "reg")]


def data(n, d, kind):
    if kind == "hydro":
        return make_hydrograph_features(n, d, n_outputs=1, config=1, unit=n)[0]
    return make_regression(n, d, n_outputs=1, n_test=0, config=8, unit=n)[0]


def reference_centers(x, m):
    km = KMeans(n_clusters=m, random_state=0, n_init="auto").fit(x)  # gpr.py:313
    return km.cluster_centers_, km.labels_, km.n_iter_


@pytest.mark.parametrize("n,d,m,kind", CASES)
def test_oracle_lloyd_reproduces_sklearn(n, d, m, kind):
    x = data(n, d, kind)
    want, labels, n_iter = reference_centers(x, m)
    got, glabels, giter = okm.kmeans_centers(x, m)
    assert giter == n_iter and np.array_equal(glabels, labels)
    assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want)))


@pytest.mark.parametrize("n,d,m", gk.END_TO_END)
def test_oracle_lloyd_reproduces_sklearn_at_the_kernel_branch_shapes(n, d, m):
    want, labels, n_iter = gk.sklearn_fit(n, d, m)
    got, glabels, giter = okm.kmeans_centers(gk.regression(n, d), m)
    assert giter == n_iter and np.array_equal(glabels, labels)
    assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want)))


@pytest.mark.parametrize("n,d,m,kind", CASES + [(5000, 6, 403, "reg")] + [c + ("reg-unit-n",) for c in gk.END_TO_END])
def test_seeding_replay_is_sklearns_kmeans_plusplus(n, d, m, kind):
    """kmeans_numpy.kmeans_pp_replay on the RandomState(0) draws of gpras_amd.kmeans picks exactly scikit-learn's rows."""
    from sklearn.cluster import kmeans_plusplus
    from sklearn.utils.extmath import row_norms

    from gpras_amd.kmeans import _draws

    x = gk.regression(n, d) if kind == "reg-unit-n" else data(n, d, kind)
    xc = np.ascontiguousarray(x - x.mean(axis=0))
    _, want = kmeans_plusplus(xc, m, x_squared_norms=row_norms(xc, squared=True), random_state=0)
    trials, first, uniforms = _draws(n, m)
    got, _, _ = kn.kmeans_pp_replay(xc, m, trials, first, uniforms)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", sorted(gk.SEEDING))
def test_seeding_inputs_are_far_from_a_rounding_decision(name):
    """A condition on the inputs of test_gpu_kmeans_kernels.py (its docstring, part c): a seed that fails here is replaced here."""
    _, gap_search, gap_potential = gk.seeding_replay(name)
    assert gap_search >= gk.MARGIN and gap_potential >= gk.MARGIN, (gap_search, gap_potential)


def test_seeding_replay_of_the_planted_draws():
    """A draw of exactly 0 is row 0; a draw above 1 is clipped to the last row."""
    last = gk.seeding_input("planted_above_one")[0].shape[0] - 1
    assert gk.seeding_replay("planted_zero")[0][list(gk.PLANTED_ALL)].tolist() == [0, 0]
    assert gk.seeding_replay("planted_above_one")[0][list(gk.PLANTED_ALL)].tolist() == [last, last]


@pytest.mark.parametrize("case", gk.LATTICE)
def test_lattice_inputs_converge_with_exact_ties_and_no_empty_cluster(case):
    x, init = gk.lattice(*case)
    assert len(np.unique(init, axis=0)) == case[2] and case[1] * case[2] > 0
    assert gk.tie_share(x, init) >= 0.05
    _, _, n_iter, empty = okm.lloyd(x, init, 0.0, 300)
    assert not empty and 2 < n_iter < 300


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,m,kind", CASES + [(16384, 12, 300, "reg")])
def test_device_lloyd_reproduces_sklearn(n, d, m, kind):
    from gpras_amd.kmeans import kmeans_centers

    x = data(n, d, kind)
    want, labels, n_iter = reference_centers(x, m)
    got, info = kmeans_centers(x, m, return_info=True)
    assert info["device"] and info["n_iter"] == n_iter and np.array_equal(info["labels"], labels)
    assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want)))


@pytest.mark.gpu
def test_gpras_inducing_points_come_from_the_device_kmeans():
    from gpras_amd.gpr import GPRAS

    x, y, _ = make_regression(600, 5, n_outputs=1, n_test=0, config=8, unit=3)
    g = GPRAS("RBF")
    z = g._create_inducing(x, 40, "kmeans")
    want, _, _ = reference_centers(x, 40)
    assert z.shape == (40, 5) and np.max(np.abs(z - want)) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,m,kind", CASES + [(16384, 12, 300, "reg"), (16384, 8, 50, "reg"), (5000, 6, 403, "reg")])
def test_device_kmeans_plusplus_picks_sklearns_points(n, d, m, kind):
    """the k-means++ seeding on the device (gprx_kmeans_pp) against sklearn.cluster.kmeans_plusplus on the same
    centred data and RandomState(0): the same rows, in the same order."""
    from sklearn.cluster import kmeans_plusplus
    from sklearn.utils.extmath import row_norms

    from gpras_amd.kmeans import kmeans_pp_indices

    x = data(n, d, kind)
    xc = np.ascontiguousarray(x - x.mean(axis=0))
    _, want = kmeans_plusplus(xc, m, x_squared_norms=row_norms(xc, squared=True), random_state=0)
    got = kmeans_pp_indices(xc, m)
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_device_kmeans_init_time_at_n16384(capsys):
    import time

    from gpras_amd.kmeans import kmeans_centers

    x = data(16384, 10, "reg")
    kmeans_centers(x, 50)
    t0 = time.perf_counter()
    kmeans_centers(x, 50)
    dt = time.perf_counter() - t0
    with capsys.disabled():
        print(f"\n[kmeans init N=16384 d=10 M=50 on the device: {1e3 * dt:.1f} ms]")
    assert dt < 0.06  # (round 2: 120 ms with the seeding on the host; the verdict's bar is 15 ms on an idle box)


def test_draw_sequence_check_against_the_installed_sklearn(monkeypatch):
    """the device seeding hard-codes how scikit-learn >= 1.3 consumes RandomState(0); the once-per-process check must
    accept the installed release and must notice a release that draws differently (then kmeans_centers seeds through sklearn)."""
    from gpras_amd import kmeans

    monkeypatch.setattr(kmeans, "_DRAWS_MATCH_SKLEARN", None)
    assert kmeans.draws_match_installed_sklearn() is True
    real = kmeans._draws

    def other_release(n, m):  # e.g. an older scikit-learn: randint for the first centre, random_sample for the trials
        trials, _, _ = real(n, m)
        rs = np.random.RandomState(0)
        return trials, int(rs.randint(n)), np.ascontiguousarray(rs.random_sample((max(m - 1, 1), trials)))

    monkeypatch.setattr(kmeans, "_DRAWS_MATCH_SKLEARN", None)
    monkeypatch.setattr(kmeans, "_draws", other_release)
    assert kmeans.draws_match_installed_sklearn() is False
