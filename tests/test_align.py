"""Per-event temporal clipping without a device: the numpy restatement in the device's summation order (tests/align_numpy.py) against
the reference's own outputs (tests/golden/align_ref_golden.npz), the bookkeeping of _align_datasets, and the host side of
gpras_amd/align.py (argument checks, storage, the slices of ``clip``).

Bounds.  The cutoffs are integers and must be equal.  The curve: every value is a sum of non-negative terms of magnitude at most 1,
formed by the reference with numpy's pairwise sums and by the restatement with trees of depth 6 + 3 + ceil(C / 256) for a row sum and
sequential sums over the T - 1 rows for the total and the running sum; each sum of n terms is off by at most n units of 2^-53 relative,
so two curves differ by at most 2 (2 T + C / 256 + 16) 2^-53 -- 4.9e-13 with the largest T and C of the fixture.  The fixture's
eps_curve must respect that, and the restatement is held to the fixture's own eps_curve.
"""

import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import align_numpy
from gpras_amd import _lib
from gpras_amd.align import FILE_FORMAT, EventAligner

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_align_ref import ALIGN_HF, ALIGN_LF, ALIGN_PRESET, ALIGN_ROWS, COLS, ROWS, align_plans, align_ref_cases, input_checksums  # noqa: E402

FIX = np.load(os.path.join(GOLDEN, "align_ref_golden.npz"))
CASES = align_ref_cases()
PLANS = align_plans()
EPS, MARGIN = float(FIX["eps_curve"]), float(FIX["min_margin"])
RAISING = [n for n in CASES if f"{n}/raises" in FIX.files]
COMPUTING = [n for n in CASES if n not in RAISING]


def test_the_fixture_belongs_to_these_inputs():
    meta = json.loads(str(FIX["meta_json"]))
    assert meta["input_checksums"] == input_checksums(CASES, PLANS)
    assert EPS == meta["eps_curve"] and MARGIN == meta["min_margin"] >= 1e-9
    assert EPS <= 2.0 * (2 * max(ROWS) + max(COLS) / 256 + 16) * 2.0**-53
    assert sorted(RAISING) == ["nan/row0", "nan/row1"] and len(COMPUTING) == len(COLS) * (len(ROWS) - 1) + 1 + 8
    assert (align_numpy.W, align_numpy.S, align_numpy.ROW_TILE, align_numpy.FINISH_CHUNK) == (64, 256, 32, 1024)
    assert set(COLS) == {1, 63, 64, 65, 255, 256, 257, 2 * 256 + 37} and {2, 3, 33 + 1, 65, 130, 1024 + 76} <= set(ROWS)


@pytest.mark.parametrize("name", COMPUTING)
def test_restatement_against_the_reference(name):
    c = CASES[name]
    cum, used = align_numpy.curve(c["combo"])
    want = FIX[f"{name}/curve"]
    assert cum.shape == want.shape == (used - 1,)
    assert align_numpy.cutoff_of_curve(cum, c["threshold"]) == tuple(FIX[f"{name}/cutoff"])
    assert align_numpy.get_cutoff(c["combo"], c["threshold"]) == tuple(FIX[f"{name}/cutoff"])
    if name == "const/all":
        assert np.all(np.isnan(cum)) and np.all(np.isnan(want)) and tuple(FIX[f"{name}/cutoff"]) == (0, 0)
    else:
        diff = float(np.max(np.abs(cum - want)))
        print(f"{name}: max |curve difference| {diff:.3e}, eps_curve {EPS:.3e}")
        assert diff <= EPS


def test_the_quirks_the_fixture_records():
    assert tuple(FIX["nan/row2/cutoff"]) == (0, 0) and FIX["nan/row2/curve"].shape == (1,)  # two rows left: one difference row
    assert FIX["nan/last_row/curve"].shape == (38,) and FIX["nan/second_block/curve"].shape == (28,) and FIX["nan/tail/curve"].shape == (24,)
    assert FIX["thr/0.5/cutoff"][1] < FIX["thr/0.999/cutoff"][1]
    for T in ROWS[:2]:  # one and two difference rows: the indices are those of difference rows, unshifted
        assert tuple(FIX[f"grid/C64_T{T}/cutoff"]) == (0, T - 2)


@pytest.mark.parametrize("name", RAISING)
def test_fewer_than_two_rows_after_the_trim_raise(name):
    assert "empty sequence" in str(FIX[f"{name}/raises"])  # what the reference said
    with pytest.raises(ValueError):
        align_numpy.get_cutoff(CASES[name]["combo"])


def test_fewer_than_two_rows_raise_without_a_device():
    al = EventAligner()
    for bad in (np.zeros((1, 5)), np.zeros((0, 5))):
        with pytest.raises(ValueError, match="fewer than 2 rows"):
            al.get_cutoff(bad)
        with pytest.raises(ValueError, match="fewer than 2 rows"):
            al.cutoff_curve(bad)
        with pytest.raises(ValueError):
            align_numpy.get_cutoff(bad)
    with pytest.raises(ValueError, match="fewer than 2 rows"):
        al.align([("p", np.zeros((1, 3)), np.zeros((1, 2)))])
    assert al._h.value is None  # no handle was needed to say so


def test_align_datasets_bookkeeping():
    hf, lf, runs, t, cutoffs = align_numpy.align(PLANS, 0.95, ALIGN_PRESET)
    assert np.array_equal(hf, FIX["align/hf"], equal_nan=True) and np.array_equal(lf, FIX["align/lf"], equal_nan=True)
    assert hf.shape[1] == ALIGN_HF and lf.shape[1] == ALIGN_LF
    assert list(runs) == list(FIX["align/runs"]) and np.array_equal(t, FIX["align/t"])
    want = {p: tuple(int(v) for v in c) for (p, _, _), c in zip(PLANS, FIX["align/cutoffs"])}
    assert cutoffs == want and cutoffs["p2"] == ALIGN_PRESET["p2"]  # the preset entry is kept, the others are computed
    assert want["p3"][1] < ALIGN_ROWS["p3"] - 9  # p3's NaN rows were trimmed before its curve was formed
    at = 0
    for plan, a, _ in PLANS:  # the index: the plan's name and 0 .. stop - start - 1, plans in order
        start, stop = want[plan]
        n = stop - start
        assert list(runs[at : at + n]) == [plan] * n and np.array_equal(t[at : at + n], np.arange(n))
        assert np.array_equal(hf[at : at + n], a[start:stop], equal_nan=True)
        at += n
    assert at == len(runs) == len(hf) == len(lf)


def test_a_zero_length_event_contributes_no_rows():
    rng = np.random.default_rng(5)
    flat = np.broadcast_to(100.0 + rng.random(ALIGN_HF + ALIGN_LF), (12, ALIGN_HF + ALIGN_LF)).copy()
    plans = [PLANS[0], ("flat", flat[:, :ALIGN_HF], flat[:, ALIGN_HF:]), PLANS[2]]
    hf, lf, runs, t, cutoffs = align_numpy.align(plans)
    assert cutoffs["flat"] == (0, 0) and "flat" not in set(runs)
    n1 = cutoffs["p1"][1] - cutoffs["p1"][0]
    assert len(hf) == n1 + cutoffs["p3"][1] - cutoffs["p3"][0] and runs[n1 - 1] == "p1" and runs[n1] == "p3" and t[n1] == 0


def test_storage_round_trip():
    al = EventAligner(0.9, {"p2": (3, 17), "p10": (0, 0)})
    d = al.to_dict()
    assert str(d["format"]) == FILE_FORMAT and all(isinstance(v, np.ndarray) and v.dtype != object for v in d.values())
    back = EventAligner.from_dict(d)
    assert back.flow_convergence_threshold == 0.9 and back.cutoffs == {"p2": (3, 17), "p10": (0, 0)}
    import io

    f = io.BytesIO()
    np.savez(f, **d)
    f.seek(0)
    with np.load(f, allow_pickle=False) as z:
        again = EventAligner.from_dict({k: z[k] for k in z.files})
    assert again.cutoffs == back.cutoffs and again.flow_convergence_threshold == 0.9
    empty = EventAligner.from_dict(EventAligner().to_dict())
    assert empty.cutoffs == {} and empty.flow_convergence_threshold == 0.95
    with pytest.raises(ValueError):
        EventAligner.from_dict({k: v for k, v in d.items() if k != "format"})
    with pytest.raises(ValueError):
        EventAligner.from_dict(dict(d, cutoffs=d["cutoffs"][:1]))
    with pytest.raises(ValueError, match="string"):  # a plan that is not a string would come back under another key
        EventAligner(cutoffs={7: (1, 2)}).to_dict()


def test_clip_slices_another_table_by_the_plan_cutoff():
    import pandas as pd

    al = EventAligner(cutoffs={"p": (2, 5), "q": (4, 4)})
    table = np.arange(24.0).reshape(8, 3)
    assert np.array_equal(al.clip("p", table), table[2:5]) and al.clip("q", table).shape == (0, 3)
    frame = pd.DataFrame(table, columns=list("abc"))
    assert al.clip("p", frame).equals(frame.iloc[2:5])
    with pytest.raises(KeyError):
        al.clip("other", table)


def test_argument_checks_that_need_no_device():
    with pytest.raises(ValueError):
        EventAligner(float("nan"))
    with pytest.raises(ValueError):
        EventAligner(float("inf"))
    with pytest.raises(ValueError):
        EventAligner(cutoffs={"p": (1, 2, 3)})
    with pytest.raises(ValueError):
        EventAligner(cutoffs={"p": (-1, 2)})
    with pytest.raises(ValueError):
        EventAligner(cutoffs={"p": (0.5, 2)})
    al = EventAligner()
    with pytest.raises(ValueError):
        al.get_cutoff(np.zeros(7))
    with pytest.raises(ValueError):
        al.get_cutoff(np.zeros((7, 0)))
    with pytest.raises(ValueError, match="same T"):
        al.align([("p", np.zeros((5, 3)), np.zeros((4, 2)))])
    with pytest.raises(ValueError, match="no plans"):
        al.align([])
    assert al._h.value is None

    # the C ABI judges its arguments before it looks at the handle: every refusal says which argument it was
    lib = _lib.load()
    x = np.zeros((3, 4))
    start, stop = C.c_int64(), C.c_int64()

    def cutoff(n_blocks=1, cols=4, ld=4, rows=3, thr=0.95, block=x.ctypes.data):
        rc = lib.gprx_al_cutoff_dev(None, n_blocks, (C.c_void_p * 4)(block, block, block, block), (C.c_int64 * 4)(cols, cols, cols, cols),
                                    (C.c_int64 * 4)(ld, ld, ld, ld), rows, thr, C.byref(start), C.byref(stop), None, None)
        return rc, _lib.last_error()

    for kwargs, word in ((dict(n_blocks=0), "n_blocks"), (dict(n_blocks=5), "n_blocks"), (dict(cols=0), "cols"), (dict(ld=3), "ld"),
                         (dict(rows=0), "rows"), (dict(rows=1), "fewer than 2 rows"), (dict(thr=float("nan")), "threshold"),
                         (dict(thr=float("inf")), "threshold"), (dict(block=None), "null"), (dict(), "null handle")):
        rc, msg = cutoff(**kwargs)
        assert rc == _lib.GPRX_EINVAL and word in msg, (kwargs, msg)
    assert lib.gprx_al_cutoff(None, None, 3, 4, 0.95, C.byref(start), C.byref(stop), None, None) == _lib.GPRX_EINVAL
    assert lib.gprx_al_clip_dev(None, None, 3, 4, 0, 1, None, 4) == _lib.GPRX_EINVAL and "lds" in _lib.last_error()
    assert lib.gprx_al_clip_dev(None, None, 4, 4, 0, 1, None, 3) == _lib.GPRX_EINVAL and "ldd" in _lib.last_error()
    assert lib.gprx_al_clip_dev(None, None, 4, 4, -1, 1, None, 4) == _lib.GPRX_EINVAL and "start" in _lib.last_error()
    assert lib.gprx_al_create(0, None) == _lib.GPRX_EINVAL
    assert lib.gprx_al_timings(None, None) == _lib.GPRX_EINVAL and lib.gprx_al_synchronize(None) == _lib.GPRX_EINVAL
    assert lib.gprx_al_destroy(None) == _lib.GPRX_OK
