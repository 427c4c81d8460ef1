"""LF-to-HF mesh resampling without a device: the numpy restatement (tests/resample_numpy.py) against the reference's own outputs
(tests/golden/resample_ref_golden.npz), and the host side of gpras_amd/resample.py (point location, weights, index folding, the
outside marker, storage, the domain)."""

import json
import os
import sys

import numpy as np
import pytest

import resample_numpy
from gpras_amd.resample import FILE_FORMAT, MeshResampler

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_resample_ref import N_AOI, N_HF, N_HF_FULL, N_LF, ON_EDGE, ON_VERTEX, OUTSIDE, ROWS, input_checksums, resample_ref_cases  # noqa: E402

FIX = np.load(os.path.join(GOLDEN, "resample_ref_golden.npz"))
CASES = resample_ref_cases()
GEO = CASES["geometry"]["g"]
EPS = float(FIX["eps_interp"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64)[~np.isnan(b)], b.view(np.int64)[~np.isnan(b)]) and np.array_equal(np.isnan(a), np.isnan(b))


def linear_resampler(elev=True):
    return MeshResampler.linear(GEO["lf_xy"], GEO["hf_xy"], GEO["cell_elevations"] if elev else None, GEO["lf_cell_ids"], n_lf=N_LF)


def test_the_fixture_belongs_to_these_inputs():
    meta = json.loads(str(FIX["meta_json"]))
    assert meta["input_checksums"] == input_checksums(CASES)
    assert EPS == meta["eps_interp"] == 0.0  # the restatement reproduces the reference's bits: the device is held to them
    assert (N_HF, N_LF, N_AOI) == (101, 53, 37) and sorted(ROWS.values()) == [1, 23, 64]


@pytest.mark.parametrize("name", list(ROWS))
def test_restatement_equals_the_reference_bit_for_bit(name):
    b = CASES["blocks"][name]
    elev = GEO["cell_elevations"]
    assert same_bits(resample_numpy.nearest(b["hf_wse"], GEO["hf_resampler"]), FIX[f"hf/{name}/wse"])
    assert same_bits(resample_numpy.nearest(b["wse"], GEO["lf_resampler"], elev), FIX[f"nearest/{name}/lf_plan_data"])
    assert same_bits(resample_numpy.velocity(b["vx"], b["vy"], GEO["lf_resampler"]), FIX[f"velocity/{name}/lf_plan_data"])
    assert same_bits(resample_numpy.velocity(b["hf_wse"] - 102.0, 103.0 - b["hf_wse"], GEO["hf_resampler"]), FIX[f"hf/{name}/velocity"])
    rs = linear_resampler()
    assert same_bits(resample_numpy.linear(b["wse"], rs.idx, rs.weights, elev), FIX[f"linear/{name}/lf_plan_data"])
    rs.close()


def test_linear_host_preparation_weights_folding_and_outside_marker():
    rs = linear_resampler()
    simplex, vert, c = resample_numpy.locate(GEO["lf_xy"], GEO["hf_xy"])
    outside = simplex < 0
    assert rs.n_vert == 3 and rs.n_src == N_LF and rs.n_out == N_HF and rs.idx.dtype == np.int32
    assert same_bits(rs.weights, c)  # the vectorised weights equal the scalar restatement, NaN rows included
    assert np.array_equal(rs.idx[~outside], GEO["lf_cell_ids"][vert[~outside]])  # columns of the plan's block, not of the AOI
    assert np.all(rs.idx[outside] == -1) and np.all(np.isnan(rs.weights[outside])) and np.all(outside[OUTSIDE])
    assert not outside[ON_VERTEX].any() and not outside[ON_EDGE].any()
    assert np.all(np.sort(np.abs(rs.weights[ON_VERTEX]), axis=1)[:, :2] < 1e-12)
    assert np.all(np.min(np.abs(rs.weights[ON_EDGE]), axis=1) < 1e-12)
    # without ids the block holds exactly the AOI cells, in order
    plain = MeshResampler.linear(GEO["lf_xy"], GEO["hf_xy"], None)
    assert plain.n_src == N_AOI and np.array_equal(plain.idx[~outside], vert[~outside]) and plain.cell_elevations is None
    assert MeshResampler.linear(GEO["lf_xy"], GEO["hf_xy"], None, GEO["lf_cell_ids"]).n_src == int(GEO["lf_cell_ids"].max()) + 1


def test_a_located_degenerate_simplex_is_refused(monkeypatch):
    import scipy.spatial

    class Fake:  # two triangles of a square, the second one without a barycentric transform, three of four points in it
        def __init__(self, points):
            self.simplices = np.array([[0, 1, 2], [0, 2, 3]])
            self.transform = np.zeros((2, 3, 2))
            self.transform[1] = np.nan

        def find_simplex(self, p):
            return np.array([0, 1, 1, 1, -1])[: len(p)]

    monkeypatch.setattr(scipy.spatial, "Delaunay", Fake)
    square = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    with pytest.raises(ValueError, match="3 HF points lie in degenerate simplices"):
        MeshResampler.linear(square, np.full((5, 2), 0.5), None)
    assert MeshResampler.linear(square, np.full((1, 2), 0.5), None).n_out == 1  # a degenerate simplex that holds no point does no harm


@pytest.mark.parametrize("kind", ["nearest", "velocity", "linear", "gather"])
def test_file_round_trip(tmp_path, kind):
    if kind == "linear":
        rs = linear_resampler()
    elif kind == "gather":
        rs = MeshResampler.nearest(GEO["hf_resampler"], N_HF_FULL)
    else:
        rs = MeshResampler.nearest(GEO["lf_resampler"], N_LF, GEO["cell_elevations"], "velocity" if kind == "velocity" else "wse")
    assert (rs.cell_elevations is None) == (kind in ("velocity", "gather"))  # the velocity magnitude has no floor
    path = tmp_path / "resampler.npz"
    rs.to_file(path)
    with np.load(path, allow_pickle=False) as z:
        assert str(z["format"]) == FILE_FORMAT == "gpras_amd-resample-1"
    back = MeshResampler.from_file(path)
    a, b = rs.to_dict(), back.to_dict()
    assert a.keys() == b.keys()
    for key in a:
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f"), key
    assert (back.n_src, back.n_out, back.n_vert, back.hydraulic_parameter) == (rs.n_src, rs.n_out, rs.n_vert, rs.hydraulic_parameter)
    np.savez(path, format=np.array("gpras_amd-pseudo-1"), **a)
    with pytest.raises(ValueError, match="not a mesh-resampler file"):
        MeshResampler.from_file(path)


def test_domain_errors():
    idx, elev = GEO["lf_resampler"], GEO["cell_elevations"]
    bad = idx.copy()
    bad[4] = N_LF
    for args in ((bad, N_LF), (-idx - 1, N_LF), (idx.astype(float), N_LF), (idx.reshape(1, -1), N_LF), (idx[:0], N_LF), (idx, 0), (idx, 2**28 + 1)):
        with pytest.raises(ValueError):
            MeshResampler.nearest(*args)
    with pytest.raises(ValueError):
        MeshResampler.nearest(idx, N_LF, elev[:-1])
    with pytest.raises(ValueError):
        MeshResampler.nearest(idx, N_LF, elev, "stage")
    lf, hf = GEO["lf_xy"], GEO["hf_xy"]
    for args in ((lf[:2], hf, None), (lf[:, :1], hf, None), (np.column_stack([lf, lf[:, 0]]), hf, None), (lf, hf[:, 0], None), (lf, hf, elev[:5]),
                 (lf, hf, None, GEO["lf_cell_ids"][:-1]), (lf, hf, None, -GEO["lf_cell_ids"] - 1), (lf, np.where(hf > 9, np.nan, hf), None)):
        with pytest.raises(ValueError):
            MeshResampler.linear(*args)
    with pytest.raises(ValueError):
        MeshResampler.linear(lf, hf, None, GEO["lf_cell_ids"], n_lf=N_AOI)  # ids beyond the block
    mixed = linear_resampler().idx.copy()
    mixed[int(np.flatnonzero(mixed[:, 0] >= 0)[0]), 1] = -1  # neither three vertices nor the marker
    with pytest.raises(ValueError):
        MeshResampler(N_LF, mixed, np.zeros((N_HF, 3)))
    with pytest.raises(ValueError):
        MeshResampler(N_LF, linear_resampler().idx, None)  # weights missing
    with pytest.raises(ValueError):
        MeshResampler(N_LF, idx, np.zeros((N_HF, 3)))  # weights without vertices
    # shapes and operands of the calls are checked before the device is touched
    rs = MeshResampler.nearest(idx, N_LF, elev)
    z = np.zeros((3, N_LF))
    for call in (lambda: rs.lf_plan_data(z[:, :-1]), lambda: rs.lf_plan_data(z[0]), lambda: rs.lf_plan_data(z, z), lambda: rs.hf_plan_data(z)):
        with pytest.raises(ValueError):
            call()
    vel = MeshResampler.nearest(idx, N_LF, hydraulic_parameter="velocity")
    for call in (lambda: vel.lf_plan_data(z), lambda: vel.lf_plan_data(z, z[:2]), lambda: linear_resampler().hf_plan_data(z)):
        with pytest.raises(ValueError):
            call()
    assert rs._h.value is None and vel._h.value is None  # no device state was created
