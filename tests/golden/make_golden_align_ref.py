"""Generate tests/golden/align_ref_golden.npz FROM THE REFERENCE ITSELF: ``DataBuilder.get_cutoff`` (gpras/preprocess.py:135-147) with
``_delta_cols_norm`` (:149-155), and ``DataBuilder._align_datasets`` (:89-116), borrowed by a small stub class that supplies what
they read: ``flow_convergence_threshold``, ``plans``, ``cutoffs`` and ``get_hf_plan_data`` / ``get_lf_plan_data`` returning pandas
frames.

Imports ``gpras.preprocess`` the way make_golden_resample_ref.py does (make_golden_pca_ref.import_reference_preprocess: inert modules
for the reference's imports that are not installed; nothing of them may be touched while the recorded calls run), with the REAL
pandas and numpy of this container (their versions are recorded).  Inputs are re-seeded by ``align_ref_cases()`` below (pure numpy;
the tests import it); the fixture holds outputs only, plus one checksum per input array.

    python tests/golden/make_golden_align_ref.py

Cases.  Hydrograph-like fields (every column a base level plus a skewed pulse with its own lag, width and height, and a slow
recession), not white noise: the curve is then a smooth S and stays away from the thresholds.
  grid/C{C}_T{T}   C in COLS x T in ROWS: the column counts around a wave (64) and a strip (256) of csrc/align.h and the row counts
                   around its row tile (32 difference rows) and its finish chunk (1024); every seventh column constant from C = 8 on.
  nan/*            NaN first at row 2, at the last row, only in the second block (from HF_COLS on), in a tail of whole rows; NaN first
                   at row 0 and at row 1, where the reference raises ValueError (recorded as such).
  const/*          constant columns among moving ones; an all-constant block, (0, 0).
  thr/*            thresholds 0.5 and 0.999 on one field.
  align/*          three plans through _align_datasets, "p2" with a preset cutoff, "p3" with NaN rows at its end.

Recorded per case: (start, stop) and the reference's cumulative curve: get_cutoff returns the integers only, so the module's
``np`` is replaced for the duration of the call by a pass-through that keeps what its ``np.cumsum`` (:143) returns.  ``eps_curve``:
the largest absolute difference between the curve of the restatement (tests/align_numpy.py, the device's summation order) and the
reference's.  ``min_margin``: the smallest
|cum - threshold| over all cases and both thresholds (the case's and 10e-4), on either curve.  The script asserts min_margin >= 1e-9
and that the restatement's cutoffs equal the reference's in every case: a condition on the inputs, not a tolerance.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

COLS = (1, 63, 64, 65, 255, 256, 257, 549)  # W - 1, W, W + 1, S - 1, S, S + 1, 2 S + 37 for W = 64, S = 256
ROWS = (2, 3, 33, 34, 65, 130, 1100)  # 34: one row past a row tile; 1100: past one finish chunk (grid: with C = 65 only)
HF_COLS, LF_COLS, SPECIAL_ROWS = 180, 120, 40
ALIGN_HF, ALIGN_LF = 101, 77
ALIGN_ROWS = {"p1": 48, "p2": 31, "p3": 70}
ALIGN_PRESET = {"p2": (3, 17)}


def hydrograph(rng, T, C):
    """(T, C): a base level and one skewed pulse per column, with a slow recession and a ripple far below the pulse."""
    t = np.arange(T, dtype=np.float64)[:, None]
    base = 100.0 + 5.0 * rng.random(C)
    amp = 0.5 + 2.0 * rng.random(C)
    peak = T * (0.25 + 0.3 * rng.random(C))
    rise = T * (0.05 + 0.05 * rng.random(C)) + 0.5
    fall = T * (0.15 + 0.15 * rng.random(C)) + 0.5
    width = np.where(t < peak, rise, fall)
    z = base + amp * np.exp(-0.5 * ((t - peak) / width) ** 2) + 1e-4 * rng.random((T, C))
    return np.ascontiguousarray(z)


def align_ref_cases():
    """Inputs of every recorded call: name -> dict(combo (T, C), threshold).  Pure numpy."""
    rng = np.random.default_rng(20261018)
    cases = {}
    for C in COLS:
        for T in ROWS:
            if T == 1100 and C != 65:
                continue
            z = hydrograph(rng, T, C)
            if C >= 8:
                z[:, ::7] = z[0, ::7]
            cases[f"grid/C{C}_T{T}"] = dict(combo=z, threshold=0.95)
    C, T = HF_COLS + LF_COLS, SPECIAL_ROWS

    def field():
        return hydrograph(rng, T, C)

    z = field()
    z[2, 17] = np.nan
    z[5:, 100] = np.nan
    cases["nan/row2"] = dict(combo=z, threshold=0.95)
    z = field()
    z[T - 1, C - 1] = np.nan
    cases["nan/last_row"] = dict(combo=z, threshold=0.95)
    z = field()
    z[29, HF_COLS + 63] = np.nan
    z[33:, HF_COLS + 5] = np.nan
    cases["nan/second_block"] = dict(combo=z, threshold=0.95)
    z = field()
    z[25:, :] = np.nan
    cases["nan/tail"] = dict(combo=z, threshold=0.95)
    for row in (0, 1):
        z = field()
        z[row, 200] = np.nan
        cases[f"nan/row{row}"] = dict(combo=z, threshold=0.95)
    z = field()
    z[:, 3:C:5] = 101.5
    z[:, 64:128] = z[7, 64:128]
    cases["const/some"] = dict(combo=z, threshold=0.95)
    cases["const/all"] = dict(combo=np.ascontiguousarray(np.broadcast_to(100.0 + rng.random(C), (T, C))), threshold=0.95)
    z = field()
    for thr in (0.5, 0.999):
        cases[f"thr/{thr}"] = dict(combo=z, threshold=thr)
    return cases


def align_plans():
    """The three plans of the _align_datasets run: [(plan, hf (T, ALIGN_HF), lf (T, ALIGN_LF))].  Pure numpy."""
    rng = np.random.default_rng(20261019)
    plans = []
    for plan, T in ALIGN_ROWS.items():
        both = hydrograph(rng, T, ALIGN_HF + ALIGN_LF)
        hf, lf = np.ascontiguousarray(both[:, :ALIGN_HF]), np.ascontiguousarray(both[:, ALIGN_HF:])
        if plan == "p3":
            lf[T - 9 :, 5] = np.nan
            hf[T - 4 :, :] = np.nan
        plans.append((plan, hf, lf))
    return plans


def input_checksums(cases, plans):
    out = {name: float(np.sum(np.where(np.isfinite(c["combo"]), c["combo"], 0.0))) for name, c in cases.items()}
    for plan, hf, lf in plans:
        out[f"align/{plan}/hf"] = float(np.sum(np.where(np.isfinite(hf), hf, 0.0)))
        out[f"align/{plan}/lf"] = float(np.sum(np.where(np.isfinite(lf), lf, 0.0)))
    return out


def main():
    import pandas as pd
    from make_golden_pca_ref import STUBBED, TOUCHED, import_reference_preprocess

    import align_numpy

    ref_pre = import_reference_preprocess()
    cases, plans = align_ref_cases(), align_plans()
    out = {}
    TOUCHED.clear()

    class Stub:  # what get_cutoff, _delta_cols_norm and _align_datasets read
        get_cutoff = ref_pre.DataBuilder.get_cutoff
        _delta_cols_norm = ref_pre.DataBuilder._delta_cols_norm
        _align_datasets = ref_pre.DataBuilder._align_datasets

        def __init__(self, threshold, plan_data=(), cutoffs=None):
            self.flow_convergence_threshold = threshold
            self.data = {p: (hf, lf) for p, hf, lf in plan_data}
            self.plans = [p for p, _, _ in plan_data]
            self.cutoffs = dict(cutoffs or {})
            self._hf_aligned = self._lf_aligned = None

        def get_hf_plan_data(self, plan):
            hf = self.data[plan][0]
            return pd.DataFrame(hf.copy(), index=pd.date_range("2026-01-01", periods=len(hf), freq="h"), columns=np.arange(hf.shape[1]))

        def get_lf_plan_data(self, plan):
            lf = self.data[plan][1]
            return pd.DataFrame(lf.copy(), index=pd.date_range("2026-01-01", periods=len(lf), freq="h"), columns=np.arange(lf.shape[1]))

    class RecordingNumpy:
        """numpy as gpras.preprocess sees it, with the results of cumsum kept: the curve is what passes through the reference's own
        ``np.cumsum`` call (:143) while its get_cutoff runs."""

        def __init__(self):
            self.curves = []

        def __getattr__(self, name):
            return getattr(np, name)

        def cumsum(self, *args, **kwargs):
            self.curves.append(np.cumsum(*args, **kwargs))
            return self.curves[-1]

    def reference_cutoff_and_curve(stub, combo):
        recorder = RecordingNumpy()
        ref_pre.np = recorder
        try:
            cutoff = stub.get_cutoff(combo)
        finally:
            ref_pre.np = np
        assert len(recorder.curves) == 1
        return cutoff, recorder.curves[0].copy()

    eps, margin, summary = 0.0, np.inf, {}
    for name, c in cases.items():
        stub = Stub(c["threshold"])
        with np.errstate(invalid="ignore", divide="ignore"):
            try:
                (start, stop), cum = reference_cutoff_and_curve(stub, c["combo"].copy())
            except ValueError as exc:
                out[f"{name}/raises"] = np.array(str(exc))
                try:
                    align_numpy.get_cutoff(c["combo"], c["threshold"])
                    raise AssertionError(f"{name}: the reference raises, the restatement does not")
                except ValueError:
                    pass
                summary[name] = "ValueError"
                continue
        assert (start, stop) == align_numpy.cutoff_of_curve(cum, c["threshold"]), name  # the curve recorded is the one get_cutoff judged
        mine, tp = align_numpy.curve(c["combo"])
        assert mine.shape == cum.shape and align_numpy.cutoff_of_curve(mine, c["threshold"]) == (start, stop), (name, start, stop)
        out[f"{name}/cutoff"] = np.array([start, stop], dtype=np.int64)
        out[f"{name}/curve"] = cum
        if np.all(np.isnan(cum)):
            assert np.all(np.isnan(mine)) and (start, stop) == (0, 0), name
        else:
            eps = max(eps, float(np.max(np.abs(mine - cum))))
            for curve in (cum, mine):
                for thr in (c["threshold"], align_numpy.START_THRESHOLD):
                    margin = min(margin, float(np.min(np.abs(curve - thr))))
        summary[name] = [int(start), int(stop), int(tp)]

    # ---- _align_datasets: three plans, one preset --------------------------------------------------------------------------------
    stub = Stub(0.95, plans, ALIGN_PRESET)
    with np.errstate(invalid="ignore", divide="ignore"):
        stub._align_datasets()
    hf_al, lf_al = stub._hf_aligned, stub._lf_aligned
    assert hf_al.index.names == ["run", "t"] and hf_al.index.equals(lf_al.index)
    out["align/hf"], out["align/lf"] = hf_al.values, lf_al.values
    out["align/runs"] = np.array([str(r) for r in hf_al.index.get_level_values("run")])
    out["align/t"] = np.asarray(hf_al.index.get_level_values("t"), dtype=np.int64)
    out["align/cutoffs"] = np.array([stub.cutoffs[p] for p, _, _ in plans], dtype=np.int64)
    assert tuple(stub.cutoffs["p2"]) == ALIGN_PRESET["p2"]
    mine = align_numpy.align(plans, 0.95, ALIGN_PRESET)
    assert all(tuple(mine[4][p]) == tuple(stub.cutoffs[p]) for p in stub.cutoffs)
    assert np.array_equal(mine[0], hf_al.values, equal_nan=True) and np.array_equal(mine[1], lf_al.values, equal_nan=True)
    for plan, hf, lf in plans:
        if plan in ALIGN_PRESET:
            continue
        for curve in (align_numpy.curve(np.concatenate([hf, lf], axis=1))[0],):
            for thr in (0.95, align_numpy.START_THRESHOLD):
                margin = min(margin, float(np.min(np.abs(curve - thr))))
    summary["align"] = {p: [int(v) for v in stub.cutoffs[p]] for p in stub.cutoffs}

    assert not TOUCHED, f"inert modules were used during the recorded calls: {TOUCHED[:10]}"
    assert margin >= 1e-9, margin
    out["eps_curve"], out["min_margin"] = np.array(eps), np.array(margin)
    meta = {
        "reference_file": "gpras/preprocess.py",
        "functions": ["DataBuilder._align_datasets :89-116", "DataBuilder.get_cutoff :135-147", "DataBuilder._delta_cols_norm :149-155"],
        "inert_modules": sorted(set(STUBBED)),
        "cases": summary,
        "eps_curve": eps,
        "min_margin": margin,
        "input_checksums": input_checksums(cases, plans),
        "python": sys.version.split()[0],
        "numpy": np.__version__,
        "pandas": pd.__version__,
    }
    out["meta_json"] = np.array(json.dumps(meta, sort_keys=True))
    path = os.path.join(HERE, "align_ref_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes): eps_curve = {eps:.3e}, min_margin = {margin:.3e}; " + json.dumps(summary))


if __name__ == "__main__":
    main()
