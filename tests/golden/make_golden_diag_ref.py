"""Generate tests/golden/diag_ref_golden.npz FROM THE REFERENCE ITSELF: ``performance_cdf`` (gpras/utils/plotting.py:201-233),
``performance_scatterplot`` (:155-198) and ``map_detection_categories`` (:716-859), run as they are with the drawing replaced by
recorders.

Imports ``gpras.utils.plotting`` the way make_golden_align_ref.py imports ``gpras.preprocess`` (make_golden_pca_ref: inert modules for
the reference's imports that are not installed -- geopandas, seaborn; nothing of them may be touched while the recorded calls run),
with the REAL numpy, pandas and matplotlib of this container (their versions are recorded).  The module's ``plt``,
``PatchCollection`` and ``apply_formatting`` are replaced for the duration of a call: ``plt.subplots`` hands out axes that keep every
call made on them, so that

  performance_cdf          the two curves are the first arguments of its two ``ax.plot`` calls (:226-227), the percentages the second;
  performance_scatterplot  ``(ll, ur)`` is the first argument of ``ax.plot`` (:184, :192), the label the ``rmse: ...`` string of ``ax.text``;
  map_detection_categories the per-cell face colours are the ``facecolor`` of its ``PatchCollection`` (:839), mapped back to categories
                           through the inverse of its ``color_map`` (:808-814; restated here as COLOR_TO_CODE, the only thing taken
                           from the function's text), the event is read from ``ax.set_title`` (:845).  The mesh frame is a pandas
                           frame with ``cell_id`` and stub polygon objects (``geom_type``, ``exterior.coords``).

All three functions could be driven this way; none is restated for the fixture.  Inputs are re-seeded by ``diag_ref_cases()`` below
(pure numpy; the tests import it); the fixture holds outputs only, plus one checksum per input array.

    python tests/golden/make_golden_diag_ref.py

Cases.
  fields/*   (lf, hf, upskill) triples: (7, 300); (17, 241) = DG_TILE + 1 values; (50, 601); a (5, 130) triple with NaN in lf, in hf
             and in both at one place, an inf, a -0.0 against 0.0 and denormal differences.
  detect/C{cells}/cn{0,1}/thr{0,1}   cells in 1, 63, 64, 65, 255, 256, 257; three events of 1, 2 and DG_RT + 1 = 17 rows; column 1 all
             NaN in the truth and column 2 NaN in some rows (where the field has them); thresholds 0 and 0.25; shuffled cell ids.
  detect/negative   a negative maximum in the second event: the reference's ValueError, recorded as such.

The script asserts that 100 * rmse is at least 1e-6 away from a half-integer in every scatter case (``round(rmse, 2)`` is then
stable), that no per-event maximum lies within 1e-9 of the wet threshold, and that the restatement (tests/diag_numpy.py) agrees
with everything recorded: conditions on the inputs, not tolerances.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

DG_TILE, DG_RT = 4096, 16  # gpras_amd/diagnostics.py
DETECT_CELLS = (1, 63, 64, 65, 255, 256, 257)
DETECT_EVENTS = (("e1", 0, 1), ("e2", 1, 3), ("e3", 3, 3 + DG_RT + 1))
DETECT_THRESHOLDS = (0.0, 0.25)
FIELD_SHAPES = {"small": (7, 300), "tile": (17, 241), "big": (50, 601)}
COLOR_TO_CODE = {"#FFFFFF": 0, "#009E73": 1, "#D55E00": 2, "#E69F00": 3, "#999999": 4}


def diag_ref_cases():
    """Inputs of every recorded call.  Pure numpy.  -> (fields, detect): fields[name] = dict(lf, hf, upskill); detect[name] =
    dict(y_true, y_pred, columns) with the rows of DETECT_EVENTS."""
    rng = np.random.default_rng(20261025)
    fields = {}
    for name, (T, C) in FIELD_SHAPES.items():
        t = np.arange(T, dtype=np.float64)[:, None]
        hf = 100.0 + 5.0 * rng.random(C) + 2.0 * np.exp(-0.5 * ((t - 0.4 * T) / (0.2 * T + 1.0)) ** 2) * rng.random(C)
        fields[name] = dict(lf=hf + 0.3 * rng.normal(size=(T, C)), hf=hf, upskill=hf + 0.04 * rng.normal(size=(T, C)))
    T, C = 5, 130
    hf = 3.0 + rng.random((T, C))
    lf, up = hf + 0.3 * rng.normal(size=(T, C)), hf + 0.04 * rng.normal(size=(T, C))
    lf[0, 3] = up[0, 5] = np.nan
    hf[1, 7] = np.nan
    lf[2, 9] = hf[2, 9] = up[2, 9] = np.nan
    lf[3, 11] = np.inf
    hf[4, 0], lf[4, 0], up[4, 0] = 0.0, -0.0, 5e-324
    hf[4, 1], lf[4, 1], up[4, 1] = 1e-310, 3e-310, 0.0
    fields["special"] = dict(lf=lf, hf=hf, upskill=up)
    detect = {}
    rows = DETECT_EVENTS[-1][2]
    for C in DETECT_CELLS:
        y_true = np.maximum(rng.normal(0.1, 0.5, size=(rows, C)), 0.0)
        y_pred = np.maximum(y_true + rng.normal(0.0, 0.3, size=(rows, C)), 0.0) * (rng.random((rows, C)) < 0.8)
        if C > 1:
            y_true[:, 1] = np.nan
        if C > 2:
            y_true[4:9, 2] = np.nan
            y_pred[0, 2] = y_pred[5, 2] = np.nan
        detect[f"C{C}"] = dict(y_true=y_true, y_pred=y_pred, columns=rng.permutation(C) + 1000)
    y_true = np.maximum(rng.normal(0.1, 0.5, size=(rows, 40)), 0.0)
    y_pred = y_true.copy()
    y_pred[2, 17] = -0.5
    y_pred[1, 17] = -1.0
    detect["negative"] = dict(y_true=y_true, y_pred=y_pred, columns=np.arange(40) + 1000)
    return fields, detect


def detect_index():
    return [(name, t) for name, lo, hi in DETECT_EVENTS for t in range(hi - lo)]


def input_checksums(fields, detect):
    out = {}
    for group, cases in (("fields", fields), ("detect", detect)):
        for name, c in cases.items():
            for key, a in c.items():
                a = np.asarray(a, dtype=np.float64)
                out[f"{group}/{name}/{key}"] = float(np.sum(np.where(np.isfinite(a), a, 0.0)))
    return out


# ---- the recorders -------------------------------------------------------------------------------------------------------------------
class RecordingAxes:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def record(*args, **kwargs):
            self.calls.append((name, args, kwargs))

        return record

    def of(self, name):
        return [c for c in self.calls if c[0] == name]


class RecordingFigure:
    def savefig(self, *a, **k):
        pass


class RecordingPyplot:
    def __init__(self):
        self.axes = []
        self.rcParams = {}

    def subplots(self, nrows=1, ncols=1, **kwargs):
        axs = [RecordingAxes() for _ in range(nrows * ncols)]
        self.axes.append(axs)
        return RecordingFigure(), (axs[0] if len(axs) == 1 else axs)

    def close(self, *a, **k):
        pass


class StubRing:
    coords = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)]


class StubPolygon:
    geom_type = "Polygon"
    exterior = StubRing()


def main():
    import matplotlib
    import pandas as pd
    from make_golden_pca_ref import REFERENCE, STUBBED, TOUCHED, _LastResortFinder, absent_reference_imports

    import diag_numpy

    sys.meta_path.append(_LastResortFinder(absent_reference_imports()))
    sys.path.insert(0, REFERENCE)
    import gpras.utils.plotting as ref

    assert os.path.abspath(ref.__file__).startswith(REFERENCE), ref.__file__
    fields, detect = diag_ref_cases()
    out, summary = {}, {}
    collections = []

    def recording_collection(patches, **kwargs):
        collections.append(kwargs)
        return object()

    real = (ref.plt, ref.PatchCollection, ref.apply_formatting)

    def run(fn, *args, **kwargs):
        plt = RecordingPyplot()
        ref.plt, ref.PatchCollection, ref.apply_formatting = plt, recording_collection, (lambda fig, ax: None)
        del collections[:]
        try:
            with np.errstate(invalid="ignore"):
                fn(*args, **kwargs)
        finally:
            ref.plt, ref.PatchCollection, ref.apply_formatting = real
        return plt.axes

    TOUCHED.clear()
    # ---- performance_cdf, performance_scatterplot ------------------------------------------------------------------------------------
    for name, c in fields.items():
        lf, hf, up = c["lf"], c["hf"], c["upskill"]
        ((ax,),) = run(ref.performance_cdf, lf.copy(), hf.copy(), up.copy(), "unused.png")
        (_, (curve_lf, pcts), _), (_, (curve_up, pcts2), _) = ax.of("plot")
        assert pcts is pcts2 and curve_lf.shape == (lf.size,)
        for key, curve, side in (("cdf_lf", curve_lf, lf), ("cdf_upskill", curve_up, up)):
            mine = diag_numpy.sorted_abs_residual(side, hf)
            assert np.array_equal(mine.view(np.int64)[~np.isnan(curve)], curve.view(np.int64)[~np.isnan(curve)]) and np.array_equal(np.isnan(mine), np.isnan(curve))
            out[f"fields/{name}/{key}"] = curve
        out[f"fields/{name}/pcts"] = pcts
        (axs,) = run(ref.performance_scatterplot, lf.copy(), hf.copy(), up.copy(), "unused.png")
        for key, ax, side in (("lf", axs[0], lf), ("upskill", axs[1], up)):
            ((_, (ends, ends2), _),) = ax.of("plot")
            ((_, targs, _),) = ax.of("text")
            label = targs[2]
            assert ends == ends2 and label.startswith("rmse: ")
            mine = diag_numpy.scatter_summary(side, hf)
            if np.isnan(ends[0]):
                assert np.isnan(mine["ll"]) and np.isnan(mine["ur"]) and label == "rmse: nan"
            else:
                assert (mine["ll"], mine["ur"]) == tuple(ends), (name, key)
                exact = float(np.mean((side.flatten() - hf.flatten()) ** 2) ** 0.5)
                for v in (exact, mine["rmse"]):
                    frac = (100.0 * v) % 1.0
                    assert abs(frac - 0.5) >= 1e-6, (name, key, v)
                assert label == f"rmse: {round(mine['rmse'], 2)}", (name, key, label, mine["rmse"])
            out[f"fields/{name}/scatter_{key}/ends"] = np.array(ends, dtype=np.float64)
            out[f"fields/{name}/scatter_{key}/label"] = np.array(label)
            summary[f"fields/{name}/{key}"] = label

    # ---- map_detection_categories ----------------------------------------------------------------------------------------------------
    index = np.empty(len(detect_index()), dtype=object)
    index[:] = detect_index()
    ranges = [(lo, hi) for _, lo, hi in DETECT_EVENTS]
    margin = np.inf
    for name, c in detect.items():
        y_true, y_pred, columns = c["y_true"], c["y_pred"], c["columns"]
        mesh = pd.DataFrame({"cell_id": np.sort(columns)[::-1].copy(), "geometry": [StubPolygon() for _ in columns]})
        if name == "negative":
            try:
                run(ref.map_detection_categories, mesh, y_true.copy(), y_pred.copy(), index, columns, ".", include_correct_negative=True, wet_threshold_depth=0.0)
                raise AssertionError("the reference does not raise on a negative maximum")
            except ValueError as exc:
                out["detect/negative/raises"] = np.array(str(exc))
            try:
                diag_numpy.detection_codes(y_true, y_pred, ranges, 0.0, True)
                raise AssertionError("the restatement does not raise")
            except ValueError:
                pass
            continue
        order = np.argsort(columns)  # the reference draws the cells sorted by id (:768-770)
        for cn in (0, 1):
            for k, thr in enumerate(DETECT_THRESHOLDS):
                axes = run(ref.map_detection_categories, mesh, y_true.copy(), y_pred.copy(), index, columns, ".", include_correct_negative=bool(cn),
                           wet_threshold_depth=thr)
                assert len(axes) == len(DETECT_EVENTS) == len(collections)
                codes = np.zeros((len(DETECT_EVENTS), len(columns)), dtype=np.uint8)
                seen = set()
                for (ax,), coll in zip(axes, list(collections)):
                    ((_, (title,), _),) = ax.of("set_title")
                    event = title.removeprefix("Detection Outcomes - ")
                    e = [n for n, _, _ in DETECT_EVENTS].index(event)
                    seen.add(e)
                    by_id = np.array([COLOR_TO_CODE[col] for col in coll["facecolor"]], dtype=np.uint8)
                    codes[e, order] = by_id
                assert len(seen) == len(DETECT_EVENTS)
                mine = diag_numpy.detection_codes(y_true, y_pred, ranges, thr, bool(cn))
                assert np.array_equal(mine, codes), (name, cn, thr)
                out[f"detect/{name}/cn{cn}/thr{k}/codes"] = codes
                summary[f"detect/{name}/cn{cn}/thr{k}"] = np.bincount(codes.ravel(), minlength=5).tolist()
                for lo, hi in ranges:
                    for f in (y_true, y_pred):
                        m = diag_numpy.event_max(f, lo, hi)
                        m = m[~np.isnan(m)]
                        if thr > 0.0:
                            margin = min(margin, float(np.min(np.abs(m - thr), initial=np.inf)))
                        margin = min(margin, float(np.min(m[m != 0.0], initial=np.inf)))  # thr = 0: a maximum is 0 exactly or well above it
    assert margin >= 1e-9, margin
    assert not TOUCHED, f"inert modules were used during the recorded calls: {TOUCHED[:10]}"
    meta = {
        "reference_file": "gpras/utils/plotting.py",
        "functions": ["performance_scatterplot :155-198", "performance_cdf :201-233", "map_detection_categories :716-859"],
        "restated_functions": [],
        "inert_modules": sorted(set(STUBBED)),
        "cases": summary,
        "min_threshold_margin": margin,
        "input_checksums": input_checksums(fields, detect),
        "python": sys.version.split()[0],
        "numpy": np.__version__,
        "pandas": pd.__version__,
        "matplotlib": matplotlib.__version__,
    }
    out["meta_json"] = np.array(json.dumps(meta, sort_keys=True))
    path = os.path.join(HERE, "diag_ref_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes): min_threshold_margin = {margin:.3e}; " + json.dumps(summary))


if __name__ == "__main__":
    main()
