"""Generate tests/golden/resample_ref_golden.npz FROM THE REFERENCE ITSELF: ``DataBuilder.get_hf_plan_data`` (gpras/preprocess.py:163-174),
``RasUpskillDataBuilder.get_lf_plan_data`` (:363-377) and ``RasInterpolaterBuilder.get_lf_plan_data`` (:433-451), borrowed by a small
stub class that supplies what they read: the plans' output blocks (``hf_ras`` / ``lf_ras`` with ``plan_hdfs[plan].mesh_timeseries_output``),
``lf_resampler`` / ``hf_resampler``, ``lf_geometry_aoi`` / ``hf_geometry_aoi`` (``cell_id`` and the centroid coordinates as pandas
frames), ``cell_elevations``, ``hydraulic_parameter``, ``mesh_id`` and the time index.

Imports ``gpras.preprocess`` the way make_golden_pseudo_ref.py does (make_golden_pca_ref.import_reference_preprocess: inert modules
for the reference's imports that are not installed; nothing of them may be touched while the recorded calls run), with the REAL
pandas, scipy and numpy of this container (their versions are recorded).  Inputs are re-seeded by ``resample_ref_cases()`` below
(pure numpy; the tests import it); the fixture holds outputs only, plus one checksum per input array.

    python tests/golden/make_golden_resample_ref.py

Cases.  n_hf = 101 HF cells; the LF plan's block has 53 cells of which 37, in no order, lie in the area of interest; T = 23, 64, 1.
Resamplers with repeated and unordered indices.  HF points inside the LF triangulation, ON its vertices, ON its edges (the LF
coordinates are multiples of 1/64, so the midpoint of two of them is exact) and outside the hull.  Each of value, elevation and NaN
wins somewhere; a NaN in the block; a NaN elevation (under a value, and under a point outside the hull); the velocity magnitude.

``eps_interp`` is the largest relative difference between the numpy restatement (tests/resample_numpy.py) and the reference over
all recorded fields; the GPU tests hold the device to the reference bit for bit when it is 0.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

N_HF, N_HF_FULL, N_LF, N_AOI = 101, 140, 53, 37
ROWS = {"a": 23, "b": 64, "c": 1}
# HF points by kind: [0, 70) random, [70, 78) on LF vertices, [78, 88) on LF edges, [88, 101) outside the hull
ON_VERTEX, ON_EDGE, OUTSIDE = slice(70, 78), slice(78, 88), slice(88, 101)


def resample_ref_cases():
    """Inputs of every recorded call.  Pure numpy."""
    rng = np.random.default_rng(20261017)
    geo = {}
    geo["lf_cell_ids"] = rng.permutation(N_LF)[:N_AOI]  # columns of the plan's block, in no order
    lf_xy = rng.integers(0, 641, (N_AOI, 2)) / 64.0  # in [0, 10], multiples of 1/64
    assert len(np.unique(lf_xy, axis=0)) == N_AOI
    geo["lf_xy"] = lf_xy
    hf_xy = np.empty((N_HF, 2))
    hf_xy[:70] = rng.uniform(0.5, 9.5, (70, 2))
    hf_xy[ON_VERTEX] = lf_xy[rng.choice(N_AOI, 8, replace=False)]
    # a point and its nearest neighbour are joined by an edge of every Delaunay triangulation
    start = rng.choice(N_AOI, 10, replace=False)
    d2 = ((lf_xy[start, None, :] - lf_xy[None, :, :]) ** 2).sum(axis=2)
    d2[np.arange(10), start] = np.inf
    hf_xy[ON_EDGE] = 0.5 * (lf_xy[start] + lf_xy[np.argmin(d2, axis=1)])
    angle = rng.uniform(0.0, 2.0 * np.pi, 13)
    hf_xy[OUTSIDE] = 5.0 + 9.0 * np.column_stack([np.cos(angle), np.sin(angle)])  # radius 9 around the centre of a 10 x 10 square
    geo["hf_xy"] = hf_xy
    geo["lf_resampler"] = rng.integers(0, N_LF, N_HF)  # repeated, unordered
    geo["lf_resampler"][:3] = [0, N_LF - 1, 0]
    geo["hf_resampler"] = rng.permutation(N_HF_FULL)[:N_HF]
    elev = 100.0 + 5.0 * rng.random(N_HF)
    elev[11] = np.nan  # under an interpolated value
    elev[95] = np.nan  # under a point outside the hull
    geo["cell_elevations"] = elev
    cases = {"geometry": {"g": geo}, "blocks": {}}
    for name, T in ROWS.items():
        wse = 100.0 + 5.0 * rng.random((T, N_LF))
        vx, vy = rng.standard_normal((T, N_LF)), rng.standard_normal((T, N_LF))
        hf_wse = 100.0 + 5.0 * rng.random((T, N_HF_FULL))
        if T > 3:
            wse[3, geo["lf_cell_ids"][5]] = np.nan  # a vertex of some triangles
            wse[T - 1, geo["lf_resampler"][17]] = np.nan
            vx[2, geo["lf_resampler"][40]] = np.nan
            vy[5, geo["lf_resampler"][41]] = np.inf
            hf_wse[1, geo["hf_resampler"][7]] = np.nan
        cases["blocks"][name] = dict(wse=wse, vx=vx, vy=vy, hf_wse=hf_wse)
    return cases


def input_checksums(cases):
    out = {}
    for group, members in cases.items():
        for name, c in members.items():
            for key, v in c.items():
                out[f"{group}/{name}/{key}"] = float(np.sum(np.where(np.isfinite(v), v, 0.0)))
    return out


def main():
    import pandas as pd
    import scipy
    from make_golden_pca_ref import STUBBED, TOUCHED, import_reference_preprocess

    import resample_numpy

    ref_pre = import_reference_preprocess()
    cases = resample_ref_cases()
    geo = cases["geometry"]["g"]
    out = {}
    TOUCHED.clear()

    # ---- the stubs that lend the reference's methods what they read ------------------------------------------------------------
    class Values:  # what mesh_timeseries_output returns: anything with .values
        def __init__(self, a):
            self.values = a.copy()

    class Asset:
        def __init__(self, blocks):
            self.blocks = blocks

        def mesh_timeseries_output(self, mesh_id, name):
            assert mesh_id == "mesh"
            return Values(self.blocks[name])

    class Model:
        def __init__(self, blocks):
            self.plan_hdfs = {"p1": Asset(blocks)}

    class Centroid:
        def __init__(self, xy):
            self.xy = xy

        def get_coordinates(self):
            return pd.DataFrame({"x": self.xy[:, 0], "y": self.xy[:, 1]})

    class Geometry:  # the part of a geo frame the methods read: ["cell_id"], .geometry.centroid and .centroid
        def __init__(self, cell_id, xy):
            self.frame = pd.DataFrame({"cell_id": cell_id})
            self.centroid = Centroid(xy)
            self.geometry = self

        def __getitem__(self, key):
            return self.frame[key]

    class Stub:
        get_hf_plan_data = ref_pre.DataBuilder.get_hf_plan_data
        mesh_id = "mesh"
        hf_resampler = geo["hf_resampler"]
        lf_resampler = geo["lf_resampler"]
        cell_elevations = geo["cell_elevations"]
        lf_geometry_aoi = Geometry(geo["lf_cell_ids"], geo["lf_xy"])
        hf_geometry_aoi = Geometry(geo["hf_resampler"], geo["hf_xy"])

        def __init__(self, hydraulic_parameter, hf_blocks, lf_blocks, T):
            self.hydraulic_parameter = hydraulic_parameter
            self.hf_ras, self.lf_ras = Model(hf_blocks), Model(lf_blocks)
            self.index = pd.date_range("2026-01-01", periods=T, freq="h")

        def get_unsteady_timeseries_index(self, plan):
            return self.index

        def get_lf_unsteady_timeseries_index(self, plan):
            return self.index

    class Upskill(Stub):
        get_lf_plan_data = ref_pre.RasUpskillDataBuilder.get_lf_plan_data

    class Interpolater(Stub):
        get_lf_plan_data = ref_pre.RasInterpolaterBuilder.get_lf_plan_data

    # ---- recorded calls ---------------------------------------------------------------------------------------------------------
    simplex, vert, c = resample_numpy.locate(geo["lf_xy"], geo["hf_xy"])
    folded = np.where(vert >= 0, geo["lf_cell_ids"][np.where(vert >= 0, vert, 0)], -1)
    assert np.all(simplex[OUTSIDE] == -1) and np.all(simplex[ON_VERTEX] >= 0) and np.all(simplex[ON_EDGE] >= 0)
    assert np.all(np.sort(np.abs(c[ON_VERTEX]), axis=1)[:, :2] < 1e-12)  # on a vertex: one weight of 1
    assert np.all(np.min(np.abs(c[ON_EDGE]), axis=1) < 1e-12)  # on an edge: one weight of 0
    elev = geo["cell_elevations"]
    eps = 0.0
    summary = {"outside": int((simplex < 0).sum())}

    def relative(got, want):
        ok = np.isfinite(want)
        assert np.array_equal(got[~ok], want[~ok], equal_nan=True)  # NaN and infinities in the same places
        return float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]))) if ok.any() else 0.0

    for name, b in cases["blocks"].items():
        T = ROWS[name]
        lf_wse = {"Water Surface": b["wse"]}
        lf_vel = {"Cell Velocity - Velocity X": b["vx"], "Cell Velocity - Velocity Y": b["vy"]}
        hf_vel = {"Cell Velocity - Velocity X": b["hf_wse"] - 102.0, "Cell Velocity - Velocity Y": 103.0 - b["hf_wse"]}
        with np.errstate(invalid="ignore"):
            near = Upskill("wse", {"Water Surface": b["hf_wse"]}, lf_wse, T)
            hf = near.get_hf_plan_data("p1")
            assert list(hf.columns) == list(geo["hf_resampler"])
            out[f"hf/{name}/wse"] = hf.values
            out[f"nearest/{name}/lf_plan_data"] = near.get_lf_plan_data("p1").values
            vel = Upskill("velocity", hf_vel, lf_vel, T)
            out[f"hf/{name}/velocity"] = vel.get_hf_plan_data("p1").values
            out[f"velocity/{name}/lf_plan_data"] = vel.get_lf_plan_data("p1").values
            lin = Interpolater("wse", {"Water Surface": b["hf_wse"]}, lf_wse, T).get_lf_plan_data("p1").values
            out[f"linear/{name}/lf_plan_data"] = lin
        for key in (f"hf/{name}/wse", f"nearest/{name}/lf_plan_data", f"velocity/{name}/lf_plan_data", f"linear/{name}/lf_plan_data"):
            assert out[key].shape == (T, N_HF), key
        eps = max(eps, relative(resample_numpy.nearest(b["hf_wse"], geo["hf_resampler"]), out[f"hf/{name}/wse"]))
        eps = max(eps, relative(resample_numpy.nearest(b["wse"], geo["lf_resampler"], elev), out[f"nearest/{name}/lf_plan_data"]))
        eps = max(eps, relative(resample_numpy.velocity(b["vx"], b["vy"], geo["lf_resampler"]), out[f"velocity/{name}/lf_plan_data"]))
        eps = max(eps, relative(resample_numpy.velocity(hf_vel["Cell Velocity - Velocity X"], hf_vel["Cell Velocity - Velocity Y"], geo["hf_resampler"]),
                                out[f"hf/{name}/velocity"]))
        eps = max(eps, relative(resample_numpy.linear(b["wse"], folded, c, elev), lin))
        # who wins where (linear): the interpolated value, the elevation over a smaller value, the elevation over NaN
        raw = resample_numpy.linear(b["wse"], folded, c)
        e = np.broadcast_to(elev, raw.shape)
        with np.errstate(invalid="ignore"):
            wins = [int(np.sum(lin == raw)), int(np.sum((raw < e) & (lin == e))), int(np.sum(np.isnan(raw) & (lin == e)))]
            near_out = out[f"nearest/{name}/lf_plan_data"]
            near_wins = [int(np.sum(near_out == b["wse"][:, geo["lf_resampler"]])), int(np.sum(near_out == e))]
        assert min(wins) > 0 and min(near_wins) > 0.05 * raw.size, (wins, near_wins)
        summary[name] = dict(T=T, linear_wins=wins, nearest_wins=near_wins, nan=[int(np.isnan(lin).sum()), int(np.isnan(near_out).sum())])
    assert summary["a"]["nan"][0] > 0 and summary["a"]["nan"][1] > 0  # a NaN elevation under NaN; a NaN value that stays
    assert not TOUCHED, f"inert modules were used during the recorded calls: {TOUCHED[:10]}"
    out["eps_interp"] = np.array(eps)
    meta = {
        "reference_file": "gpras/preprocess.py",
        "functions": ["DataBuilder.get_hf_plan_data :163-174", "RasUpskillDataBuilder.get_lf_plan_data :363-377",
                      "RasInterpolaterBuilder.get_lf_plan_data :433-451"],
        "inert_modules": sorted(set(STUBBED)),
        "cases": summary,
        "eps_interp": eps,
        "input_checksums": input_checksums(cases),
        "python": sys.version.split()[0],
        "numpy": np.__version__,
        "scipy": scipy.__version__,
        "pandas": pd.__version__,
    }
    out["meta_json"] = np.array(json.dumps(meta, sort_keys=True))
    path = os.path.join(HERE, "resample_ref_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes): eps_interp = {eps:.3e}; " + json.dumps(summary))


if __name__ == "__main__":
    main()
