"""Numpy restatement of the LF-to-HF resampling of gpras/preprocess.py (:163-174, :363-377, :433-451), operation by operation: what
gpras_amd/csrc/resample.h computes on the device and gpras_amd/resample.py prepares on the host.  Used by the tests as the
reference for shapes the fixture (tests/golden/resample_ref_golden.npz, the reference's own outputs) does not hold."""

import numpy as np


def nearest(z, idx, elev=None):
    """vals[:, lf_resampler] floored by the cell elevations (:373-376): a NaN value stays, a NaN elevation never wins."""
    vals = np.asarray(z, dtype=np.float64)[:, idx]
    if elev is not None:
        e = np.broadcast_to(np.asarray(elev, dtype=np.float64), vals.shape)
        with np.errstate(invalid="ignore"):
            mask = vals < e
        vals[mask] = e[mask]
    return vals


def velocity(vx, vy, idx):
    """sqrt(vx**2 + vy**2)[:, lf_resampler], no floor (:367-373)."""
    vx, vy = np.asarray(vx, dtype=np.float64)[:, idx], np.asarray(vy, dtype=np.float64)[:, idx]
    return np.sqrt(vx * vx + vy * vy)


def locate(lf_points, hf_points):
    """(simplex (n_hf,), vertices (n_hf, 3), weights (n_hf, 3)) of scipy's Delaunay / find_simplex, the barycentric coordinates in
    the operations of LinearNDInterpolator: d = p - r, c_i = (0 + T_i0 d_0) + T_i1 d_1, c_2 = (1 - c_0) - c_1.  Outside the hull:
    simplex -1, vertices -1, NaN weights."""
    from scipy.spatial import Delaunay

    tri = Delaunay(np.asarray(lf_points, dtype=np.float64))
    p = np.asarray(hf_points, dtype=np.float64)
    s = tri.find_simplex(p)
    n = len(p)
    vert = np.full((n, 3), -1, dtype=np.int64)
    c = np.full((n, 3), np.nan)
    for j in range(n):
        if s[j] < 0:
            continue
        T = tri.transform[s[j]]
        d0, d1 = p[j, 0] - T[2, 0], p[j, 1] - T[2, 1]
        c0 = (0.0 + T[0, 0] * d0) + T[0, 1] * d1
        c1 = (0.0 + T[1, 0] * d0) + T[1, 1] * d1
        c[j] = c0, c1, (1.0 - c0) - c1
        vert[j] = tri.simplices[s[j]]
    return s, vert, c


def linear(z, vert, c, elev=None):
    """acc = ((0 + c0 z[v0]) + c1 z[v1]) + c2 z[v2]; with elevations, values below them and NaN become the elevation (:449-450).
    vert: columns of z; a row of -1 (outside the hull) gives NaN."""
    z = np.asarray(z, dtype=np.float64)
    outside = vert[:, 0] < 0
    v = np.where(outside[:, None], 0, vert)
    with np.errstate(invalid="ignore"):
        acc = ((0.0 + c[:, 0] * z[:, v[:, 0]]) + c[:, 1] * z[:, v[:, 1]]) + c[:, 2] * z[:, v[:, 2]]
        acc[:, outside] = np.nan
        if elev is not None:
            e = np.broadcast_to(np.asarray(elev, dtype=np.float64), acc.shape)
            mask = (acc < e) | np.isnan(acc)
            acc[mask] = e[mask]
    return acc
