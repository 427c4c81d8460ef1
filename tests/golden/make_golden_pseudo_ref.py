"""Generate tests/golden/pseudo_ref_golden.npz FROM THE REFERENCE ITSELF: ``RatingCurve`` (gpras/preprocess.py:454-513) directly, and
``PseudoSurfaceDataBuilder._set_centerline_interpolater`` (:643-667), ``.interpolate_centerline`` (:634-637),
``.interpolate_surface`` (:639-641) and ``.get_lf_plan_data`` (:581-599) borrowed by a small stub class that supplies what they read
(``plans``, the boundary ids, ``centerline_cell_ids``, ``get_ref_line_df``, ``get_hf_plan_data``, ``get_hms_inflow_ts``,
``cell_elevations``, ``hf_geometry_aoi``, ``get_lf_fluvial_est`` and the two curves).

Imports ``gpras.preprocess`` the way make_golden_pca_ref.py does (its last-resort finder hands out inert modules for the
reference's imports that are not installed; nothing of them may be touched while the recorded calls run), with the REAL pandas,
scipy and numpy of this container (their versions are recorded).  Inputs are re-seeded by ``pseudo_ref_cases()`` below (pure
numpy; the tests import it); the fixture holds outputs only, plus one checksum per input array.

    python tests/golden/make_golden_pseudo_ref.py

Cases.  Rating curves: non-finite, non-positive and out-of-band flows to be dropped; a curve with too few points (ValueError);
queries below, inside and above the fitted range, the knots themselves, a (T, 1) input.  Centerline fits over two plans: odd and
even counts of kept rows, masked rows, a row with us_wse == ds_wse (infinite ratios), a column that becomes NaN, tied middle
values, C = 37.  Surfaces: each of the three operands wins somewhere, n_cells odd, a NaN in the fluvial field.

``eps_spline`` is the largest relative difference between the numpy restatement (tests/pseudo_numpy.py) and the reference's
``RatingCurve.predict`` over all recorded queries; the GPU tests hold the device to 4 x eps_spline.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

US, DS = "us_line", "ds_line"
N_CENTERLINE, N_CELLS = 37, 101


def _curve_data(rng, n, base, gain):
    """A rating curve's raw record: flows over four decades with a concave stage, and entries the constructor must drop."""
    q = 10.0 ** rng.uniform(0.5, 4.5, n)
    wse = base + gain * np.log1p(q / 40.0) + 0.05 * rng.standard_normal(n)
    q[rng.choice(n, 6, replace=False)] = [np.nan, np.inf, -5.0, 0.0, 3.0, 5e11]  # not finite, not positive, below qmin, above qmax
    wse[rng.choice(n, 2, replace=False)] = [np.nan, -np.inf]
    return q, wse


def _fit_case(rng, rows, n_masked, nan_column=None, duplicate=False):
    """Boundary and centerline records of two plans (rows[0] + rows[1] timesteps)."""
    R = sum(rows)
    if duplicate:  # every row twice: the two middle values of an even count are often equal
        half = _fit_case(rng, (R // 2, 0), n_masked // 2)
        out = {k: (np.concatenate([v, v]) if isinstance(v, np.ndarray) else v) for k, v in half.items()}
        out["rows"] = rows
        return out
    us_wse = 120.0 + 6.0 * rng.random(R)
    ds_wse = us_wse - (1.0 + 4.0 * rng.random(R))
    frac = np.sort(rng.random(N_CENTERLINE))
    wse = us_wse[:, None] - (us_wse - ds_wse)[:, None] * (frac[None, :] + 0.08 * rng.standard_normal((R, N_CENTERLINE)))
    us_q = 50.0 + 900.0 * rng.random(R)
    ds_q = 60.0 + 900.0 * rng.random(R)
    masked = rng.choice(R, n_masked, replace=False)
    us_q[masked] = 0.0
    ds_q[masked] = np.where(rng.random(n_masked) < 0.5, 0.0, -3.0)
    us_q[np.setdiff1d(np.arange(R), masked)[0]] = 0.0  # one flow zero alone keeps its row
    kept = np.flatnonzero((us_q > 0) | (ds_q > 0))
    flat = kept[len(kept) // 3]
    ds_wse[flat] = us_wse[flat]  # a flat water surface: every ratio of the row is +-inf ...
    if nan_column is not None:
        wse[flat, nan_column] = us_wse[flat]  # ... or 0 / 0
    return dict(us_wse=us_wse, ds_wse=ds_wse, us_q=us_q, ds_q=ds_q, wse=wse, rows=rows)


def pseudo_ref_cases():
    """Inputs of every recorded call.  Pure numpy."""
    rng = np.random.default_rng(20261016)
    cases = {"curves": {}, "fits": {}, "surfaces": {}}
    for name, (n, base, gain) in {"us": (400, 118.0, 2.1), "ds": (353, 111.0, 1.7)}.items():
        q, wse = _curve_data(rng, n, base, gain)
        lo, hi = 10.0 ** 0.5, 10.0 ** 4.5
        queries = dict(below=np.linspace(0.2 * lo, lo, 40), inside=10.0 ** rng.uniform(1.1, 4.4, 300), above=np.linspace(hi, 4.0 * hi, 40),
                       column=(10.0 ** rng.uniform(0.3, 4.8, 57))[:, None])
        cases["curves"][name] = dict(q=q, wse=wse, queries=queries)
    q, wse = _curve_data(rng, 17, 100.0, 1.0)  # 17 raw points, 11 kept: fewer than max(8, n_knots + 5) = 12
    cases["curves"]["few"] = dict(q=q, wse=wse, queries={})
    cases["fits"]["odd"] = _fit_case(rng, (97, 94), 20)
    cases["fits"]["even"] = _fit_case(rng, (80, 111), 21)
    cases["fits"]["nan_column"] = _fit_case(rng, (50, 33), 8, nan_column=11)
    cases["fits"]["ties"] = _fit_case(rng, (30, 30), 10, duplicate=True)
    for name, (T, with_nan) in {"a": (23, True), "b": (64, False)}.items():
        us_q = 10.0 ** rng.uniform(0.8, 4.6, T)
        ds_q = us_q * rng.uniform(0.8, 1.3, T)
        elev = 108.0 + 16.0 * rng.random(N_CELLS)
        idx = rng.integers(0, N_CENTERLINE, N_CELLS)
        idx[:3] = [0, N_CENTERLINE - 1, 5]
        fluvial = 104.0 + 24.0 * rng.random((T, N_CELLS))
        if with_nan:
            fluvial[3, 17] = np.nan
            fluvial[T - 1, N_CELLS - 1] = np.nan
        cases["surfaces"][name] = dict(us_q=us_q, ds_q=ds_q, elev=elev, idx=idx, fluvial=fluvial, fit="odd")
    return cases


def input_checksums(cases):
    out = {}
    for group, members in cases.items():
        for name, c in members.items():
            for key, v in c.items():
                if isinstance(v, np.ndarray):
                    out[f"{group}/{name}/{key}"] = float(np.nansum(np.where(np.isfinite(v), v, 0.0)))
                elif isinstance(v, dict):
                    for k2, v2 in v.items():
                        out[f"{group}/{name}/{key}/{k2}"] = float(np.sum(v2))
    return out


def main():
    import pandas as pd
    import scipy
    from make_golden_pca_ref import STUBBED, TOUCHED, import_reference_preprocess

    import pseudo_numpy

    ref_pre = import_reference_preprocess()
    Builder = ref_pre.PseudoSurfaceDataBuilder
    cases = pseudo_ref_cases()
    out = {}
    TOUCHED.clear()

    # ---- rating curves ------------------------------------------------------------------------------------------------------
    curves = {}
    eps = 0.0
    for name in ("us", "ds"):
        c = cases["curves"][name]
        rc = ref_pre.RatingCurve(c["q"].copy(), c["wse"].copy())
        curves[name] = rc
        t = rc.spline.get_knots()
        knots = np.concatenate([[t[0]] * 3, t, [t[-1]] * 3])
        coef = np.asarray(rc.spline.get_coeffs())
        assert np.array_equal(knots, rc.spline._eval_args[0]) and np.array_equal(coef, rc.spline._eval_args[1][: len(coef)])
        out[f"curve/{name}/q"], out[f"curve/{name}/wse"] = rc.q, rc.wse
        out[f"curve/{name}/knots"], out[f"curve/{name}/coefficients"] = knots, coef
        stats = rc.fit_stats
        out[f"curve/{name}/fit_stats"] = np.array([stats["rmse"], stats["mae"]])
        queries = dict(c["queries"], knots=knots.copy())
        for qn, qv in queries.items():
            want = rc.predict(qv.copy())
            assert want.shape == qv.shape and np.all(np.abs(want) >= 1.0), (name, qn)
            out[f"curve/{name}/predict/{qn}"] = want
            got = pseudo_numpy.spline_eval(knots, coef, qv)
            eps = max(eps, float(np.max(np.abs(got - want) / np.abs(want))))
    try:
        ref_pre.RatingCurve(cases["curves"]["few"]["q"].copy(), cases["curves"]["few"]["wse"].copy())
        raised = ""
    except ValueError as e:
        raised = type(e).__name__
    assert raised == "ValueError"
    out["eps_spline"] = np.array(eps)

    # ---- the stub that lends the reference's methods what they read ------------------------------------------------------------
    class Stub:
        _set_centerline_interpolater = Builder._set_centerline_interpolater
        interpolate_centerline = Builder.interpolate_centerline
        interpolate_surface = Builder.interpolate_surface
        get_lf_plan_data = Builder.get_lf_plan_data
        us_bc_id_ras, ds_bc_id_ras, us_bc_id_hms, ds_bc_id_hms = US, DS, "us_hms", "ds_hms"
        centerline_cell_ids = np.arange(1000, 1000 + N_CENTERLINE)

        def get_ref_line_df(self, p):
            return self.frames[p][0]

        def get_hf_plan_data(self, p):
            return self.frames[p][1]

        def get_hms_inflow_ts(self, plan, bc_id):
            return self.flows[bc_id]

        def get_lf_fluvial_est(self, plan):
            return self.fluvial

    fitted = {}
    summary = {}
    for name, c in cases["fits"].items():
        s = Stub()
        s.plans = ["p1", "p2"]
        s.frames = {}
        r0 = 0
        for p, n in zip(s.plans, c["rows"]):
            sl = slice(r0, r0 + n)
            r0 += n
            index = pd.RangeIndex(n)
            bc = pd.DataFrame({f"{US}_wse": c["us_wse"][sl], f"{DS}_wse": c["ds_wse"][sl], f"{US}_flows": c["us_q"][sl], f"{DS}_flows": c["ds_q"][sl],
                               "another_line_wse": 0.0}, index=index)
            # the plan's cell table holds other cells too; the centerline cells come out by id
            cols = np.concatenate([[7, 8], s.centerline_cell_ids, [5000]])
            block = np.column_stack([np.full(n, -1.0), np.full(n, -2.0), c["wse"][sl], np.full(n, -3.0)])
            s.frames[p] = (bc, pd.DataFrame(block, index=index, columns=cols))
        with np.errstate(invalid="ignore", divide="ignore"):
            s._set_centerline_interpolater()
        w = np.asarray(s.cl_interpolater)
        assert w.shape == (N_CENTERLINE,)
        out[f"fit/{name}/cl_interpolater"] = w
        n_keep = int(((c["us_q"] > 0) | (c["ds_q"] > 0)).sum())
        summary[name] = dict(rows=int(sum(c["rows"])), kept=n_keep, nan_columns=int(np.isnan(w).sum()))
        assert np.array_equal(pseudo_numpy.fit_centerline(c["us_wse"], c["ds_wse"], c["us_q"], c["ds_q"], c["wse"]), w, equal_nan=True), name
        fitted[name] = w
    assert summary["odd"]["kept"] % 2 == 1 and summary["even"]["kept"] % 2 == 0 and summary["ties"]["kept"] % 2 == 0
    assert summary["nan_column"]["nan_columns"] == 1 and summary["odd"]["nan_columns"] == 0 and summary["odd"]["kept"] < summary["odd"]["rows"]

    # ---- surfaces -------------------------------------------------------------------------------------------------------------
    for name, c in cases["surfaces"].items():
        s = Stub()
        s.cl_interpolater = fitted[c["fit"]]
        s.cell_interpolater = c["idx"]
        s.cell_elevations = c["elev"]
        s.hf_geometry_aoi = pd.DataFrame({"cell_id": np.arange(N_CELLS)})
        s.us_rating_curve, s.ds_rating_curve = curves["us"], curves["ds"]
        T = len(c["us_q"])
        index = pd.RangeIndex(T)
        s.flows = {"us_hms": pd.DataFrame(c["us_q"], index=index, columns=["us_hms_FLOW"]),
                   "ds_hms": pd.DataFrame(c["ds_q"], index=index, columns=["ds_hms_FLOW"])}
        s.fluvial = c["fluvial"].copy()
        us_wse = curves["us"].predict(s.flows["us_hms"].values)
        ds_wse = curves["ds"].predict(s.flows["ds_hms"].values)
        assert us_wse.shape == (T, 1)
        cl = np.asarray(s.interpolate_centerline(us_wse, ds_wse))
        gathered = np.asarray(s.interpolate_surface(cl))
        full = s.get_lf_plan_data("p1").values
        assert cl.shape == (T, N_CENTERLINE) and gathered.shape == full.shape == (T, N_CELLS)
        out[f"surface/{name}/us_wse"], out[f"surface/{name}/ds_wse"] = us_wse, ds_wse
        out[f"surface/{name}/centerline"], out[f"surface/{name}/gathered"], out[f"surface/{name}/lf_plan_data"] = cl, gathered, full
        wins = [int(np.sum(full == gathered)), int(np.sum(full == c["elev"][None, :])), int(np.sum(full == c["fluvial"]))]
        assert min(wins) > 0.05 * full.size, wins  # each operand wins somewhere
        assert int(np.isnan(full).sum()) == int(np.isnan(c["fluvial"]).sum())
        assert np.array_equal(pseudo_numpy.surface(us_wse, ds_wse, s.cl_interpolater, c["idx"], c["elev"], c["fluvial"]), full, equal_nan=True)
        summary[f"surface_{name}"] = dict(T=T, wins=wins, nan=int(np.isnan(full).sum()))
    assert not TOUCHED, f"inert modules were used during the recorded calls: {TOUCHED[:10]}"
    meta = {
        "reference_file": "gpras/preprocess.py",
        "functions": ["RatingCurve :454-513", "PseudoSurfaceDataBuilder.get_lf_plan_data :581-599", "interpolate_centerline :634-637",
                      "interpolate_surface :639-641", "_set_centerline_interpolater :643-667"],
        "few_points_raises": raised,
        "inert_modules": sorted(set(STUBBED)),
        "cases": summary,
        "eps_spline": eps,
        "input_checksums": input_checksums(cases),
        "python": sys.version.split()[0],
        "numpy": np.__version__,
        "scipy": scipy.__version__,
        "pandas": pd.__version__,
    }
    out["meta_json"] = np.array(json.dumps(meta, sort_keys=True))
    path = os.path.join(HERE, "pseudo_ref_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes): eps_spline = {eps:.3e}; " + json.dumps(summary))


if __name__ == "__main__":
    main()
