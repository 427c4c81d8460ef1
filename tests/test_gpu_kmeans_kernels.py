"""Every branch of the device k-means (csrc/kmeans.h: kmeans_assign_kernel, kmeans_update_kernel, kpp_dist_kernel,
kpp_select_kernel; drivers gprx_kmeans_lloyd and gprx_kmeans_pp in csrc/abi_fields.hip), at the shapes where the kernels branch.

a. End to end against ``KMeans`` (the reference's call): m * d on both sides of the 4096 doubles of one LDS pass of the E-step, up
   to five passes, d = 1, 8, 9, 17, 63, 64, short and barely started workgroups, m = n, and n > 65536 (more than 256 partial sums
   and chunks longer than a workgroup in the seeding).  The bound is the project's own (test_kmeans.py): same n_iter, same labels,
   centres <= 1e-12 * max(1, |want|).
b. ``gprx_kmeans_lloyd`` alone on lattice data against ``oracle.kmeans.lloyd``: rows from {0..k-1}^d and distinct rows as initial
   centres make every product, sum and cluster total an exact integer and every mean one correctly rounded division, on both
   sides; the later distances are the same operations in the same order (difference form, no contraction, ascending k).  Labels
   and centres are therefore BIT-identical, with a fifth or more of the points at an exact tie between their two nearest initial
   centres (first index wins).  Each stopping rule alone: strict convergence (tol = 0), shift_tot <= tol (tol = 1e300: one
   iteration and the E-step rerun), the max_iter cap (and the rerun).
c. ``gprx_kmeans_pp`` alone with chosen draws against ``kmeans_numpy.kmeans_pp_replay``: the same rows in the same order.  The
   replay's margins (how far a draw is from a cumulative sum, how far the best candidate's potential from the next) are >= 1e-10
   on every input -- asserted here and, without a GPU, in test_kmeans.py -- where the device's other summation order and fused
   multiply-add move them by a few n 2^-53 (< 1e-11 at n = 70000): a different index is a kernel error, not rounding.
   Trial counts 1 to 16, n < 256 (chunks of one element, most of them empty), n > 65536, a draw of exactly 0, a draw above 1 (the
   clip to n - 1), plateaus of zero distance from duplicate rows, m = 1 (no draws at all), and the argument checks.
d. The empty-cluster flag, directly and through ``kmeans_centers``' fallback to scikit-learn.

Neither this module nor kmeans_numpy.py needs the reference tree.
"""

import ctypes as C
import functools
import warnings

import numpy as np
import pytest
from sklearn.cluster import KMeans
from sklearn.utils.extmath import row_norms

import kmeans_numpy as kn
from gpras_amd import _lib
from gpras_amd._lib import ptr
from gpras_amd.synth import make_regression
from oracle import kmeans as okm

OK, EINVAL = _lib.GPRX_OK, _lib.GPRX_EINVAL
MARGIN = 1e-10  # see (c) above

# ---- a. end to end ---------------------------------------------------------------------------------------------------------------
# (n, d, m): one E-step LDS pass holds 4096 // d centres
END_TO_END = [
    (1024, 32, 128),  # m d = 4096: exactly one pass
    (1024, 32, 129),  # one centre in the second pass
    (1500, 33, 125),  # 4125 doubles, 124 centres per pass
    (600, 64, 65),  # 64 centres per pass, the widest row
    (2000, 16, 300),  # 4800 doubles
    (700, 48, 90),  # 85 centres per pass do not fill the LDS
    (1000, 17, 256),  # tail of 1 in the M-step's blocks of 8
    (300, 64, 300),  # m = n, five passes
    (200, 3, 200),  # m = n, one pass
    (255, 5, 17),  # one short workgroup
    (257, 5, 17),  # one thread in the second workgroup
    (513, 9, 40),  # d = 9
    (1200, 8, 30),  # d = 8: no tail
    (900, 63, 20),  # d = 63
    (500, 1, 6),  # d = 1
    (70000, 2, 8),  # n > 65536 in both seeding kernels
]


def regression(n, d):
    return make_regression(n, d, n_outputs=1, n_test=0, config=8, unit=n)[0]


@functools.lru_cache(maxsize=None)
def sklearn_fit(n, d, m):
    km = KMeans(n_clusters=m, random_state=0, n_init="auto").fit(regression(n, d))  # gpr.py:313
    return km.cluster_centers_, km.labels_, km.n_iter_


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,m", END_TO_END)
def test_end_to_end_reproduces_sklearn(n, d, m):
    from gpras_amd.kmeans import kmeans_centers

    want, labels, n_iter = sklearn_fit(n, d, m)
    got, info = kmeans_centers(regression(n, d), m, return_info=True)
    err = np.max(np.abs(got - want))
    print(f"\n[kmeans end to end n={n} d={d} m={m}: device={info['device']} n_iter={info['n_iter']} (sklearn {n_iter}) centre error {err:.3e}]")
    assert info["device"] and info["n_iter"] == n_iter and np.array_equal(info["labels"], labels)
    assert err <= 1e-12 * max(1.0, np.max(np.abs(want)))


# ---- b. the Lloyd driver on lattice data -------------------------------------------------------------------------------------------
# (n, d, m, k, seed): rows from {0..k-1}^d, m distinct rows as initial centres; each converges with no empty cluster in more than
# two iterations (test_kmeans.py checks that without a GPU)
LATTICE = [
    (1000, 3, 20, 5, 0),
    (400, 64, 65, 2, 0),  # ties in the second LDS pass
    (600, 21, 200, 3, 0),  # 4200 doubles in two passes of 195, d = 2 * 8 + 5
]


@functools.lru_cache(maxsize=None)
def lattice(n, d, m, k, seed):
    g = np.random.default_rng(seed)
    x = np.ascontiguousarray(g.integers(0, k, size=(n, d)).astype(np.float64))
    first = np.sort(np.unique(x, axis=0, return_index=True)[1])  # first occurrence of every distinct row
    init = np.ascontiguousarray(x[g.choice(first, size=m, replace=False)])
    x.setflags(write=False)
    init.setflags(write=False)
    return x, init


def tie_share(x, init):
    """Share of the points whose two nearest initial centres are at exactly the same distance."""
    d2 = np.zeros((x.shape[0], init.shape[0]))
    for k in range(x.shape[1]):
        diff = x[:, k][:, None] - init[:, k][None, :]
        d2 += diff * diff
    two = np.partition(d2, 1, axis=1)[:, :2]
    return float(np.mean(two[:, 0] == two[:, 1]))


@functools.lru_cache(maxsize=None)
def oracle_lloyd(case, tol, max_iter):
    x, init = lattice(*case)
    return okm.lloyd(x, init, tol, max_iter)


def device_lloyd(lib, x, init, tol, max_iter):
    """gprx_kmeans_lloyd on copies: (rc, centres, labels, n_iter, empty)."""
    n, d = x.shape
    centers = np.array(init, dtype=np.float64, order="C")
    labels = np.full(n, -7, dtype=np.int32)
    n_iter, empty = C.c_int(-1), C.c_int(-1)
    rc = lib.gprx_kmeans_lloyd(0, ptr(x), n, d, ptr(centers), centers.shape[0], tol, max_iter, ptr(labels), C.byref(n_iter), C.byref(empty))
    return rc, centers, labels, n_iter.value, empty.value


def bit_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_lattice_run(lib, case, tol, max_iter):
    x, init = lattice(*case)
    assert tie_share(x, init) >= 0.05, "the input no longer holds exact ties"
    want_c, want_l, want_it, want_empty = oracle_lloyd(case, tol, max_iter)
    assert not want_empty
    rc, got_c, got_l, n_iter, empty = device_lloyd(lib, x, init, tol, max_iter)
    assert rc == OK, _lib.last_error()
    assert empty == 0 and n_iter == want_it, (empty, n_iter, want_it)
    assert np.array_equal(got_l, want_l), f"{int(np.sum(got_l != want_l))} labels differ"
    assert bit_equal(got_c, want_c), f"centres differ by up to {np.max(np.abs(got_c - want_c)):.3e}"
    return want_c, want_l, want_it


@pytest.mark.gpu
@pytest.mark.parametrize("case", LATTICE)
def test_lloyd_lattice_strict_convergence(lib, case):
    """tol = 0: only the repeat of the labels stops the loop."""
    _, _, n_iter = _assert_lattice_run(lib, case, 0.0, 300)
    assert 2 < n_iter < 300


@pytest.mark.gpu
@pytest.mark.parametrize("case", LATTICE)
def test_lloyd_lattice_stops_on_the_shift(lib, case):
    """tol = 1e300: one iteration; the centres are the first means, the labels those of the rerun E-step on them."""
    centers, labels, n_iter = _assert_lattice_run(lib, case, 1e300, 300)
    assert n_iter == 1
    x, init = lattice(*case)
    first = okm.assign(x, init)
    means = np.zeros_like(init)
    np.add.at(means, first, x)
    means /= np.bincount(first, minlength=init.shape[0])[:, None]
    assert bit_equal(centers, means) and np.array_equal(labels, okm.assign(x, means))
    assert not np.array_equal(labels, first), "the rerun E-step changes nothing on this input"


@pytest.mark.gpu
@pytest.mark.parametrize("case", LATTICE)
def test_lloyd_lattice_max_iter_cap(lib, case):
    assert oracle_lloyd(case, 0.0, 300)[2] > 2
    _, _, n_iter = _assert_lattice_run(lib, case, 0.0, 2)
    assert n_iter == 2


# ---- c. the seeding driver with chosen draws ---------------------------------------------------------------------------------------
# name -> (n, d, m, trials, seed); the planted draws and the duplicate rows are added in seeding_input
SEEDING = {
    "n200_d3_m30_t1": (200, 3, 30, 1, 0),
    "n777_d5_m60_t16": (777, 5, 60, 16, 0),
    "n255_d2_m12_t7": (255, 2, 12, 7, 0),
    "n1025_d64_m20_t3": (1025, 64, 20, 3, 0),
    "n64_d1_m64_t5": (64, 1, 64, 5, 0),
    "n70000_d2_m6_t3": (70000, 2, 6, 3, 0),
    "planted_zero": (300, 4, 10, 3, 0),
    "planted_above_one": (300, 4, 10, 3, 1),
    "plateaus": (400, 3, 30, 4, 1),
}
# centres whose draws are all the planted value (at the second of them that row is already a centre; row 0 of "planted_zero" is
# the origin, so that its distance is exactly 0 and a draw of 0 EQUALS the first cumulative sum: searchsorted's left-most match),
# and a centre with one planted draw among the others
PLANTED_ALL, PLANTED_ONE = (4, 6), 8


@functools.lru_cache(maxsize=None)
def seeding_input(name):
    """(xc, m, trials, first_id, uniforms): centred normal data and uniforms from default_rng(seed)."""
    n, d, m, trials, seed = SEEDING[name]
    g = np.random.default_rng(seed)
    if name == "plateaus":  # forty distinct rows, each ten times
        x = np.repeat(g.normal(size=(n // 10, d)), 10, axis=0)
    else:
        x = g.normal(size=(n, d))
    xc = np.ascontiguousarray(x - x.mean(axis=0))
    if name == "planted_zero":
        xc[0] = 0.0  # (its distance to itself is then exactly 0 in the expanded form, on both sides: see PLANTED_ALL)
    first_id = int(g.integers(n))
    uniforms = np.ascontiguousarray(g.uniform(size=(m - 1, trials)))
    if name.startswith("planted"):
        value = 0.0 if name == "planted_zero" else 1.0 + 1e-6
        uniforms[[c - 1 for c in PLANTED_ALL], :] = value
        uniforms[PLANTED_ONE - 1, 1] = value
    xc.setflags(write=False)
    uniforms.setflags(write=False)
    return xc, m, trials, first_id, uniforms


@functools.lru_cache(maxsize=None)
def seeding_replay(name):
    return kn.kmeans_pp_replay(*seeding_input(name))


def device_pp(lib, xc, m, trials, first_id, uniforms):
    """gprx_kmeans_pp: (rc, indices)."""
    n, d = xc.shape
    xsq = np.ascontiguousarray(row_norms(xc, squared=True), dtype=np.float64)
    indices = np.full(m, -7, dtype=np.int64)
    rc = lib.gprx_kmeans_pp(0, ptr(xc), n, d, ptr(xsq), m, trials, first_id, None if uniforms is None else ptr(uniforms), ptr(indices))
    return rc, indices


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SEEDING))
def test_seeding_picks_the_replayed_rows(lib, name):
    xc, m, trials, first_id, uniforms = seeding_input(name)
    want, gap_search, gap_potential = seeding_replay(name)
    assert gap_search >= MARGIN and gap_potential >= MARGIN, (gap_search, gap_potential)
    rc, got = device_pp(lib, xc, m, trials, first_id, uniforms)
    assert rc == OK, _lib.last_error()
    assert np.array_equal(got, want), f"first difference at centre {int(np.argmax(got != want))}: {got} against {want}"
    if name == "planted_zero":  # every candidate of that centre is row 0
        assert got[list(PLANTED_ALL)].tolist() == [0, 0]
    if name == "planted_above_one":  # the clip to n - 1
        assert got[list(PLANTED_ALL)].tolist() == [xc.shape[0] - 1] * 2
    if name == "plateaus":
        assert len({xc[i].tobytes() for i in got}) == m  # (a duplicate of a centre has distance 0: it is never drawn)


@pytest.mark.gpu
def test_seeding_of_one_centre_needs_no_draws(lib):
    xc = seeding_input("n255_d2_m12_t7")[0]
    for first_id in (0, 100, 254):
        rc, got = device_pp(lib, xc, 1, 3, first_id, None)
        assert rc == OK, _lib.last_error()
        assert got.tolist() == [first_id]
        assert kn.kmeans_pp_replay(xc, 1, 3, first_id, None)[0].tolist() == [first_id]


@pytest.mark.gpu
def test_bad_arguments_are_refused_and_leave_the_library_usable(lib):
    n, d, m, trials = 64, 3, 5, 2
    g = np.random.default_rng(3)
    wide = np.ascontiguousarray(g.normal(size=(n, 65)))
    xc = np.ascontiguousarray(wide[:, :d])
    xsq, wsq = row_norms(xc, squared=True), row_norms(wide, squared=True)
    uni = np.ascontiguousarray(g.uniform(size=(n, 17)))
    idx = np.zeros(n + 1, dtype=np.int64)
    pp = lib.gprx_kmeans_pp
    refused = {
        "pp d = 65": lambda: pp(0, ptr(wide), n, 65, ptr(wsq), m, trials, 0, ptr(uni), ptr(idx)),
        "pp m = n + 1": lambda: pp(0, ptr(xc), n, d, ptr(xsq), n + 1, trials, 0, ptr(uni), ptr(idx)),
        "pp trials = 17": lambda: pp(0, ptr(xc), n, d, ptr(xsq), m, 17, 0, ptr(uni), ptr(idx)),
        "pp first_id = n": lambda: pp(0, ptr(xc), n, d, ptr(xsq), m, trials, n, ptr(uni), ptr(idx)),
        "pp null x": lambda: pp(0, None, n, d, ptr(xsq), m, trials, 0, ptr(uni), ptr(idx)),
        "pp null uniforms with m > 1": lambda: pp(0, ptr(xc), n, d, ptr(xsq), m, trials, 0, None, ptr(idx)),
    }
    cen = wide.copy()
    lab = np.zeros(n, dtype=np.int32)
    it, em = C.c_int(), C.c_int()
    ll = lib.gprx_kmeans_lloyd
    refused.update({
        "lloyd d = 65": lambda: ll(0, ptr(wide), n, 65, ptr(cen), m, 0.0, 10, ptr(lab), C.byref(it), C.byref(em)),
        "lloyd m > n": lambda: ll(0, ptr(xc), n, d, ptr(cen), n + 1, 0.0, 10, ptr(lab), C.byref(it), C.byref(em)),
        "lloyd max_iter = 0": lambda: ll(0, ptr(xc), n, d, ptr(cen), m, 0.0, 0, ptr(lab), C.byref(it), C.byref(em)),
        "lloyd null n_iter": lambda: ll(0, ptr(xc), n, d, ptr(cen), m, 0.0, 10, ptr(lab), None, C.byref(em)),
    })
    for what, call in refused.items():
        assert call() == EINVAL, what
        assert _lib.last_error(), f"{what}: no message"
    # a valid call of each entry point afterwards
    first_id, uniforms = 7, np.ascontiguousarray(uni[: m - 1, :trials])
    rc, got = device_pp(lib, xc, m, trials, first_id, uniforms)
    assert rc == OK and np.array_equal(got, kn.kmeans_pp_replay(xc, m, trials, first_id, uniforms)[0])
    rc, centers, labels, n_iter, empty = device_lloyd(lib, xc, xc[got], 0.0, 300)
    want = okm.lloyd(xc, xc[got], 0.0, 300)
    assert rc == OK and empty == 0 and not want[3] and n_iter == want[2] and np.array_equal(labels, want[1])
    assert np.max(np.abs(centers - want[0])) <= 1e-12


# ---- d. the empty flag and the fallback --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case,which", [(LATTICE[0], 0), (LATTICE[0], 19), (LATTICE[1], 64)])
def test_lloyd_raises_the_empty_flag(lib, case, which):
    """An initial centre far outside the data gets no member.  Centres, labels and n_iter are unspecified then."""
    x, init = lattice(*case)
    init = init.copy()
    init[which] = 1e6
    assert okm.lloyd(x, init, 0.0, 300)[3]
    rc, _, _, _, empty = device_lloyd(lib, x, init, 0.0, 300)
    assert rc == OK, _lib.last_error()
    assert empty == 1


def repeated_rows():
    """Forty distinct rows, each ten times: fewer distinct rows than the 50 clusters asked for."""
    return np.repeat(np.random.default_rng(5).normal(size=(40, 4)), 10, axis=0)


@pytest.mark.gpu
def test_kmeans_centers_hands_an_emptied_cluster_to_sklearn():
    from gpras_amd.kmeans import kmeans_centers

    x = repeated_rows()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (ConvergenceWarning: fewer distinct points than clusters)
        km = KMeans(n_clusters=50, random_state=0, n_init="auto").fit(x)
        got, info = kmeans_centers(x, 50, return_info=True)
    assert info["device"] is False
    assert info["n_iter"] == km.n_iter_ and np.array_equal(info["labels"], km.labels_) and np.array_equal(got, km.cluster_centers_)


@pytest.mark.gpu
def test_kmeans_centers_beyond_64_features_makes_no_device_call(monkeypatch):
    from gpras_amd import kmeans

    def no_device():
        raise AssertionError("d = 65 reached the library")

    x = regression(300, 65)
    km = KMeans(n_clusters=12, random_state=0, n_init="auto").fit(x)
    monkeypatch.setattr(kmeans._lib, "load", no_device)
    got, info = kmeans.kmeans_centers(x, 12, return_info=True)
    assert info["device"] is False
    assert info["n_iter"] == km.n_iter_ and np.array_equal(info["labels"], km.labels_) and np.array_equal(got, km.cluster_centers_)
