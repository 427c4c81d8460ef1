"""The diagnostics kernels (gpras_amd/csrc/diag.h, gpras_amd/diagnostics.py) on the device against np.sort, the reference's own
recorded outputs (tests/golden/diag_ref_golden.npz) and the numpy restatement of the device's summation order (tests/diag_numpy.py).

Bounds.  None is a tolerance.  The sorted sequence of a multiset is unique: the sort equals np.sort BIT FOR BIT (NaN compared by
count, its payload being free).  Minima, maxima and category codes are exact.  The sum of squares equals the restatement bit for bit
(the same IEEE operations in the same order, contraction off); how far that order is from the exact sum is bounded in
tests/test_diagnostics.py.  ``round(rmse, 2)`` equals the reference's label: the fixture's generator asserts that no rmse lies within
1e-8 of a rounding boundary.  Sizes: around a wave (64), around a tile (DG_TILE) and one that spans many workgroups for the sort;
cells around a wave and a workgroup (256), events of 1, 2 and DG_RT + 1 rows for the detection.
"""

import ctypes as C
import os
import sys

import numpy as np
import pandas as pd
import pytest

import diag_numpy
from gpras_amd._lib import GPRX_EINVAL, GPRX_OK, DeviceBuffer, ptr
from gpras_amd.diagnostics import CATEGORY_NAMES, DG_RT, DG_TILE, FieldDiagnostics, cdf_ranks

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_diag_ref import DETECT_EVENTS, DETECT_THRESHOLDS, detect_index, diag_ref_cases  # noqa: E402

FIX = np.load(os.path.join(GOLDEN, "diag_ref_golden.npz"))
FIELDS, DETECT = diag_ref_cases()
RANGES = [(lo, hi) for _, lo, hi in DETECT_EVENTS]
SIZES = (1, 2, 63, 64, 65, DG_TILE - 1, DG_TILE, DG_TILE + 1, 2 * DG_TILE + 37, 1_000_003)
# the live bytes of the "exactly k live bytes" families: passes skipped at the bottom, in the middle and at the top, even and odd counts
LIVE = {1: (3,), 2: (0, 7), 3: (1, 2, 5), 4: (0, 2, 4, 6), 5: (3, 4, 5, 6, 7), 6: (0, 1, 2, 3, 4, 5), 7: (0, 1, 2, 3, 5, 6, 7), 8: tuple(range(8))}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64)[~np.isnan(b)], b.view(np.int64)[~np.isnan(b)]) and np.array_equal(np.isnan(a), np.isnan(b))


@pytest.fixture(scope="module")
def fd(lib):
    d = FieldDiagnostics()
    yield d
    d.close()


def keys_with_live_bytes(rng, n, live):
    """Every byte outside `live` holds one value for all keys; every byte in `live` is random, with two different values forced (n >= 2)."""
    keys = np.zeros(n, dtype=np.uint64)
    for byte in range(8):
        if byte in live:
            digit = rng.integers(0, 256, n, dtype=np.uint64)
            if n >= 2:
                digit[0], digit[n - 1] = 17, 200
        else:
            digit = np.full(n, 0x5A + byte, dtype=np.uint64)
        keys |= digit << np.uint64(8 * byte)
    return keys


def key_families(n):
    rng = np.random.default_rng(n)
    fam = {"equal": np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)}
    for k, live in LIVE.items():
        fam[f"live{k}"] = keys_with_live_bytes(rng, n, live)
    fam["lowest"] = keys_with_live_bytes(rng, n, (0,))
    fam["highest"] = keys_with_live_bytes(rng, n, (7,))
    full = keys_with_live_bytes(rng, n, tuple(range(8)))
    fam["sorted"] = np.sort(full)
    fam["reverse"] = np.sort(full)[::-1].copy()
    two = np.full(n, 0x00FF00FF00FF00FF, dtype=np.uint64)
    two[n // 3] = 0x00FF00FF00FE00FF
    fam["two_values"] = two
    return fam


def live_bytes_of(keys):
    digits = [(keys >> np.uint64(8 * p)) & np.uint64(255) for p in range(8)]
    return [p for p in range(8) if digits[p].min() != digits[p].max()]


# ---- the raw sort ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_raw_sort_equals_numpy_for_every_key_family(fd, n):
    for name, keys in key_families(n).items():
        before = keys.copy()
        got = fd.sort_u64(keys)
        assert np.array_equal(keys, before)
        assert np.array_equal(got, np.sort(keys)), (n, name)
        info = fd.last_sort_info()
        assert info["executed_passes"] == live_bytes_of(keys), (n, name)  # a pass runs exactly when its byte takes more than one value
        assert info["skipped_passes"] == 8 - len(info["executed_passes"])
        if n >= 2 and name.startswith("live"):
            assert info["executed_passes"] == list(LIVE[int(name[4:])])
    assert fd.sort_u64(key_families(n)["equal"]).size == n and fd.last_sort_info()["executed_passes"] == []


# ---- the fused route ---------------------------------------------------------------------------------------------------------------------
def special_pair():
    rng = np.random.default_rng(5)
    a, b = rng.normal(size=(7, 300)), rng.normal(size=(7, 300))
    a[0, :6] = [0.0, -0.0, 0.0, -0.0, 5e-324, 1e-310]
    b[0, :6] = [0.0, 0.0, -0.0, -0.0, 0.0, 3e-310]  # 0, -0 -> +0, 0, 0, the smallest denormal, a denormal difference
    a[1, :4] = [np.inf, 1.0, -np.inf, 2.5e-308]
    b[1, :4] = [1.0, np.inf, 3.0, 2.4e-308]  # inf three times, a denormal from two normals
    a[2, 0], b[2, 1] = np.nan, np.nan  # NaN in a, NaN in b
    a[2, 2] = b[2, 2] = np.nan  # in both
    a[2, 3], b[2, 3] = np.inf, np.inf  # inf - inf: a NaN that is not in the inputs
    return a, b


def test_fused_route_special_values_non_flattened_and_inputs_unchanged(fd):
    a, b = special_pair()
    want = np.sort(np.abs(a - b).flatten())
    assert np.isnan(want).sum() == 4 and want[0] == 0.0 and not np.signbit(want[:4]).any() and 5e-324 in want and np.isinf(want).sum() == 3
    got = fd.sorted_abs_residual(a, b)
    assert got.shape == (a.size,) and same_bits(got, want) and not np.signbit(got[~np.isnan(got)]).any()
    # device buffers in: left as they were
    da, db = DeviceBuffer.from_array(a), DeviceBuffer.from_array(b)
    try:
        got = fd.sorted_abs_residual(da, db)
        assert same_bits(got, want)
        for buf, host in ((da, a), (db, b)):
            back = buf.to_array(host.shape)
            assert np.array_equal(back.view(np.int64), host.view(np.int64))
    finally:
        da.free()
        db.free()


@pytest.mark.parametrize("n", [1, 65, DG_TILE + 1])
def test_fused_route_with_constant_and_tiny_residuals(fd, n):
    rng = np.random.default_rng(n)
    a = rng.normal(size=n)
    assert same_bits(fd.sorted_abs_residual(a, a), np.zeros(n)) and fd.last_sort_info()["executed_passes"] == []  # no pass at all: the keys are built into the output
    b = a + 1.5  # the residuals share their top bytes (all in [1.5 - ulp, 1.5 + ulp])
    got = fd.sorted_abs_residual(a, b)
    assert same_bits(got, np.sort(np.abs(a - b)))


def test_workspace_is_reused_larger_then_smaller(fd):
    rng = np.random.default_rng(11)
    for n in (3 * DG_TILE + 5, DG_TILE - 7, 2 * DG_TILE, 300):
        a, b = 10.0 + rng.normal(size=n), 10.0 + rng.normal(size=n)
        assert same_bits(fd.sorted_abs_residual(a, b), np.sort(np.abs(a - b))), n


def test_fused_route_over_many_workgroups(fd):
    rng = np.random.default_rng(3)
    a = 100.0 + rng.normal(size=(1000, 1003))
    b = a + 0.1 * rng.normal(size=a.shape)
    got = fd.sorted_abs_residual(a, b)
    assert same_bits(got, np.sort(np.abs(a - b).flatten()))
    assert fd.last_sort_info()["executed_passes"] == live_bytes_of(np.abs(a - b).flatten().view(np.uint64))


# ---- CDF and scatter against the reference's recorded outputs ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_cdf_values_at_the_ranks_equal_the_reference_curves(fd, name):
    c = FIELDS[name]
    n = c["hf"].size
    for n_points in (1, 257, n, n + 3):
        lf_v, up_v, pcts = fd.residual_cdf(c["lf"], c["hf"], c["upskill"], n_points)
        ranks = cdf_ranks(n, n_points)
        assert lf_v.shape == up_v.shape == pcts.shape == (min(n, n_points),)
        assert same_bits(lf_v, FIX[f"fields/{name}/cdf_lf"][ranks]) and same_bits(up_v, FIX[f"fields/{name}/cdf_upskill"][ranks])
        assert np.array_equal(pcts, FIX[f"fields/{name}/pcts"][ranks])
    lf_v, up_v, _ = fd.residual_cdf(None, c["hf"], c["upskill"], 64)
    assert lf_v is None and same_bits(up_v, FIX[f"fields/{name}/cdf_upskill"][cdf_ranks(n, 64)])


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_scatter_summary_equals_the_reference_and_the_restatement(fd, name):
    c = FIELDS[name]
    for key, side in (("lf", c["lf"]), ("upskill", c["upskill"])):
        got = fd.scatter_summary(side, c["hf"])
        want = diag_numpy.scatter_summary(side, c["hf"])
        ends, label = FIX[f"fields/{name}/scatter_{key}/ends"], str(FIX[f"fields/{name}/scatter_{key}/label"])
        print(f"{name}/{key}: ll {got['ll']!r} ur {got['ur']!r} sum_sq {got['sum_sq']!r} (restated {want['sum_sq']!r}) rmse {got['rmse']!r}, reference {label!r}")
        assert np.array_equal([got["ll"], got["ur"]], ends, equal_nan=True)
        assert label == f"rmse: {round(got['rmse'], 2)}"
        assert same_bits([got["sum_sq"], got["rmse"]], [want["sum_sq"], want["rmse"]]) and got["n"] == side.size


@pytest.mark.parametrize("n", [1, 255, 8192, 8193, 8192 * 256 + 5])
def test_sum_of_squares_equals_the_restatement_bit_for_bit(fd, n):
    rng = np.random.default_rng(n)
    p, hf = 100.0 + rng.normal(size=n), 100.0 + rng.normal(size=n)
    got, want = fd.scatter_summary(p, hf), diag_numpy.scatter_summary(p, hf)
    assert same_bits([got["sum_sq"], got["rmse"], got["ll"], got["ur"]], [want["sum_sq"], want["rmse"], want["ll"], want["ur"]])


# ---- detection -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sorted(DETECT) if n != "negative"])
def test_detection_codes_equal_the_reference(fd, name):
    c = DETECT[name]
    assert len({hi - lo for lo, hi in RANGES}) == 3 and sorted(hi - lo for lo, hi in RANGES) == [1, 2, DG_RT + 1]
    for cn in (0, 1):
        for k, thr in enumerate(DETECT_THRESHOLDS):
            codes, names = fd.detection_categories(c["y_true"], c["y_pred"], RANGES, wet_threshold_depth=thr, include_correct_negative=bool(cn))
            assert codes.dtype == np.uint8 and names == CATEGORY_NAMES
            assert np.array_equal(codes, FIX[f"detect/{name}/cn{cn}/thr{k}/codes"]), (name, cn, thr)
    codes, _ = fd.detection_categories(c["y_true"], c["y_pred"], pd.MultiIndex.from_tuples(detect_index()), 0.25, True)
    assert np.array_equal(codes, FIX[f"detect/{name}/cn1/thr1/codes"])


def test_negative_maximum_raises_and_names_the_event(fd):
    c = DETECT["negative"]
    message = str(FIX["detect/negative/raises"])
    with pytest.raises(ValueError, match=message + r" \(event 'e2'\)"):
        fd.detection_categories(c["y_true"], c["y_pred"], pd.MultiIndex.from_tuples(detect_index()), 0.0, True)
    with pytest.raises(ValueError, match=message + r" \(event 1\)"):
        fd.detection_categories(c["y_true"], c["y_pred"], RANGES, 0.25, False)  # the check comes before the threshold
    ok = np.abs(c["y_pred"])
    codes, _ = fd.detection_categories(c["y_true"], ok, RANGES)  # the handle is still usable
    assert np.array_equal(codes, diag_numpy.detection_codes(c["y_true"], ok, RANGES))


# ---- DevicePipeline.diagnostics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hp", ["wse", "depth", "velocity"])
def test_pipeline_diagnostics_equal_the_host_chain(lib, hp):
    from gpras_amd.gpr import GPRAS
    from gpras_amd.pipeline import DevicePipeline
    from gpras_amd.preprocess import EOFProjector

    rng = np.random.default_rng(19 + len(hp))
    n, d, m, k, cells, t_star = 64, 3, 8, 3, 40, 29
    x = rng.normal(size=(n, d))
    y = np.stack([np.sin(x @ rng.normal(size=d)) + 0.05 * rng.normal(size=n) for _ in range(k)], axis=1)
    gpr = GPRAS("Matern32")
    gpr.fit(x, y, m, "grid", "adam", max_iter=4)
    dry = np.zeros(cells, dtype=bool)
    dry[[3, 17]] = True
    elev = rng.uniform(0.0, 2.0, size=cells)
    # (velocity: the fields go into the detection as they are, so the mean keeps the predicted field positive)
    proj = EOFProjector(dry, elev, rng.normal(size=cells - 2) + {"depth": 0.0, "wse": 1.5, "velocity": 40.0}[hp], rng.uniform(0.5, 1.5, size=cells - 2),
                        rng.normal(size=(k, cells - 2)) / np.sqrt(k), rng.normal(size=k), rng.uniform(0.5, 2, size=k), hydraulic_parameter=hp)
    x_test = rng.normal(size=(t_star, d))
    truth = rng.uniform(-0.5, 2.0, size=(t_star, cells)) + (0.5 if hp == "velocity" else elev)
    lf = truth + 0.3 * rng.normal(size=truth.shape)
    index = pd.MultiIndex.from_tuples([("e1", t) for t in range(12)] + [("e2", t) for t in range(t_star - 12)], names=["event", "timestep"])
    truth_df = pd.DataFrame(truth, index=index, columns=[f"c{j}" for j in range(cells)])
    pipe = DevicePipeline(gpr, proj)
    out = pipe.diagnostics(x_test, truth_df, lf, n_points=101, wet_threshold_depth=0.3, include_correct_negative=True)

    # the host chain from existing entries: the mean field brought down, then numpy (pipeline.py:265-277 and plotting.py)
    buf, ns = pipe.predict_mean_field_dev(x_test)
    pred = buf.to_array((ns, cells))
    buf.free()
    size = ns * cells
    ranks = cdf_ranks(size, 101)
    assert hp != "velocity" or pred.min() >= 0.0, "the test's own velocity field must be non-negative"
    assert out["n"] == size and np.array_equal(out["ranks"], ranks) and np.array_equal(out["pcts"], np.linspace(0, 100, size)[ranks])
    assert same_bits(out["cdf_upskill"], np.sort(np.abs(pred - truth).flatten())[ranks])
    assert same_bits(out["cdf_lf"], np.sort(np.abs(lf - truth).flatten())[ranks])
    for key, side in (("lf", lf), ("upskill", pred)):
        want = diag_numpy.scatter_summary(side, truth)
        assert same_bits([out["scatter"][key][f] for f in ("ll", "ur", "sum_sq", "rmse")], [want[f] for f in ("ll", "ur", "sum_sq", "rmse")])
    if hp != "velocity":
        def depth(a):
            a = a - elev
            a[a < 0] = 0
            return a

        pred_d, truth_d, lf_d = depth(pred + elev if hp == "depth" else pred), depth(truth), depth(lf)
    else:
        pred_d, truth_d, lf_d = pred, truth, lf
    for key, side in (("lf", lf_d), ("upskill", pred_d)):
        want = diag_numpy.scatter_summary(side, truth_d)
        assert same_bits([out["scatter_depth"][key][f] for f in ("ll", "ur", "sum_sq", "rmse")], [want[f] for f in ("ll", "ur", "sum_sq", "rmse")])
    assert out["events"] == ["e1", "e2"] and out["category_names"] == CATEGORY_NAMES
    assert np.array_equal(out["detection_codes"], diag_numpy.detection_codes(truth_d, pred_d, [(0, 12), (12, t_star)], 0.3, True))
    # without the low-fidelity field
    out = pipe.diagnostics(x_test, truth_df, None, n_points=size + 1, include_correct_negative=False)
    assert out["cdf_lf"] is None and "lf" not in out["scatter"] and same_bits(out["cdf_upskill"], np.sort(np.abs(pred - truth).flatten()))
    assert np.array_equal(out["detection_codes"], diag_numpy.detection_codes(truth_d, pred_d, [(0, 12), (12, t_star)], 0.0, False))


# ---- errors --------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_einval_with_a_message_and_the_handle_stays_usable(lib):
    h = C.c_void_p()
    assert lib.gprx_dg_create(0, C.byref(h)) == GPRX_OK
    try:
        a = DeviceBuffer.from_array(np.array([3.0, 1.0, 2.0]))
        out = DeviceBuffer(24)
        res = np.zeros(4)
        codes = DeviceBuffer(8)
        first = C.c_int64(0)
        one = np.array([0], dtype=np.int64)
        two = np.array([3], dtype=np.int64)
        hi1, hi2 = one + 1, one + 2
        calls = [
            lambda: lib.gprx_dg_sort_u64_dev(h, a.ptr, 0, out.ptr),
            lambda: lib.gprx_dg_sort_u64_dev(h, None, 3, out.ptr),
            lambda: lib.gprx_dg_sort_abs_residual_dev(h, a.ptr, a.ptr, 0, out.ptr),
            lambda: lib.gprx_dg_sort_abs_residual_dev(h, a.ptr, None, 3, out.ptr),
            lambda: lib.gprx_dg_sort_abs_residual_dev(h, a.ptr, a.ptr, 3, None),
            lambda: lib.gprx_dg_gather_dev(h, a.ptr, 3, ptr(two), 1, ptr(res)),  # rank 3 of 3 values
            lambda: lib.gprx_dg_gather_dev(h, a.ptr, 3, None, 1, ptr(res)),
            lambda: lib.gprx_dg_scatter_summary_dev(h, a.ptr, a.ptr, 0, ptr(res)),
            lambda: lib.gprx_dg_scatter_summary_dev(h, None, a.ptr, 3, ptr(res)),
            lambda: lib.gprx_dg_detect_dev(h, a.ptr, a.ptr, 1, 3, ptr(one), ptr(hi1), 0, 0.0, 1, codes.ptr, C.byref(first)),  # E = 0
            lambda: lib.gprx_dg_detect_dev(h, a.ptr, None, 1, 3, ptr(one), ptr(hi1), 1, 0.0, 1, codes.ptr, C.byref(first)),
            lambda: lib.gprx_dg_detect_dev(h, a.ptr, a.ptr, 1, 3, ptr(one), ptr(hi2), 1, 0.0, 1, codes.ptr, C.byref(first)),  # hi past the rows
        ]
        for i, call in enumerate(calls):
            assert call() == GPRX_EINVAL, i
            assert lib.gprx_dg_last_error(h).decode(), i
        assert lib.gprx_dg_sort_u64_dev(None, a.ptr, 3, out.ptr) == GPRX_EINVAL and lib.gprx_dg_last_error(None).decode() == "null handle"
        # after the errors: the same handle sorts
        assert lib.gprx_dg_sort_abs_residual_dev(h, a.ptr, a.ptr, 3, out.ptr) == GPRX_OK
        assert np.array_equal(out.to_array((3,)), np.zeros(3))
        zero = DeviceBuffer.from_array(np.zeros(3))
        assert lib.gprx_dg_sort_abs_residual_dev(h, a.ptr, zero.ptr, 3, out.ptr) == GPRX_OK
        assert np.array_equal(out.to_array((3,)), [1.0, 2.0, 3.0])
        assert lib.gprx_dg_synchronize(h) == GPRX_OK
        for b in (a, out, codes, zero):
            b.free()
    finally:
        assert lib.gprx_dg_destroy(h) == GPRX_OK
