"""A numpy restatement of the covariance route of ``PreProcessor.fit``: the reference's fit
(gpras/preprocess.py:947-1007) for more samples than wet cells, where its ``IncrementalPCA`` keeps all n_wet components in
every batch, so the fit is the PCA of the whole centred matrix: eigh of Xc2^T Xc2, svd_flip(u_based_decision=False),
explained_variance_ = lambda / (n - 1).  Also the pure-Python replay of the order in which numpy sums a long contiguous column.
Shared by the CPU pins and the GPU parity tests."""

import numpy as np

from gpras_amd.preprocess import PCAFit, compute_norths_rule
from pca_fit_numpy import classify, svd_flip_rows

PIECE = 8192  # np.getbufsize(): a buffered reduction hands the inner loop pieces of this many elements


def _pairwise(a, lo, n):
    """numpy's pairwise_sum over a[lo : lo + n] with Python floats (IEEE doubles, one rounding per addition)."""
    if n < 8:
        res = 0.0
        for i in range(lo, lo + n):
            res += a[i]
        return res
    if n <= 128:
        r = [a[lo + i] for i in range(8)]
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] += a[lo + i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res += a[lo + i]
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(a, lo, n2) + _pairwise(a, lo + n2, n - n2)


def chunked_pairwise_sum(col):
    """The sum of one contiguous column as ``np.add.reduce`` forms it: pieces of 8192 elements, each in its pairwise tree, the piece
    sums added left to right."""
    a = [float(v) for v in col]
    total = None
    for lo in range(0, len(a), PIECE):
        s = _pairwise(a, lo, min(PIECE, len(a) - lo))
        total = s if total is None else total + s
    return total


def single_tree_sum(col):
    """One pairwise tree over the whole column: what numpy does NOT do beyond 8192 rows."""
    a = [float(v) for v in col]
    return _pairwise(a, 0, len(a))


def fit_reference_tall(x, elevations, weights, k, mode, thr=0.03):
    """Every attribute PreProcessor.fit sets, as a dict, by the covariance route (weights: the compacted weights, np.empty(0) when
    unweighted); ``transform``: the standardised training projection."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if mode == "depth":
        x = np.maximum(x - elevations, 0.0)
        classes = classify(x.max(axis=0), x.min(axis=0), thr)
    elif mode == "wse":
        classes = classify(x.max(axis=0) - elevations, x.min(axis=0) - elevations, thr)
    else:
        classes = np.repeat("TF", x.shape[1])
    dry = classes == "AD"
    n = x.shape[0]
    xw = np.asfortranarray(x[:, ~dry])
    input_mean = xw.mean(axis=0)  # contiguous columns: numpy's chunked pairwise order
    xw = xw - input_mean
    w = np.empty(0)
    if weights is not None:
        w = weights[~dry]
        xw *= w
    xc2 = xw - (0.0 + np.asfortranarray(xw).sum(axis=0)) / n
    lam, v = np.linalg.eigh(xc2.T @ xc2)
    lam, comps = np.maximum(lam[::-1], 0.0), np.ascontiguousarray(v[:, ::-1].T)
    _, comps = svd_flip_rows(np.empty((1, comps.shape[0])), comps)
    ev = lam / (n - 1)
    pca = PCAFit(explained_variance_=ev, n_samples_seen_=n, components_=comps)
    k = compute_norths_rule(pca) if k is None else k
    eofs = comps[:k]
    z = xw @ eofs.T
    x_mean, x_std = z.mean(axis=0), z.std(axis=0)
    return dict(wetness_classes=classes, input_mean=input_mean, weights=w, eofs=eofs, eigenvalues=ev, spatial_mode_count=k, n_samples_fit=n,
                x_mean=x_mean, x_std=x_std, transform=(z - x_mean) / x_std)


def assert_tall_fit_close(got, want, report=None):
    """The bounds of the covariance route (DESIGN.md sections 3.12 / 3.13 / 3.12b): classes, weights, mode count, n_samples_fit and
    input_mean exact; eigenvalues <= 1e-12 lambda_max absolute; EOF row i <= 1e-12 lambda_max / gap_i with the sign of the largest entry
    equal; x_mean <= 1e-12 x_std[0]; x_std <= 1e-11 relative; transform (when both sides carry it) <= 1e-9.  ``report``: a dict that
    receives every measured figure before its assertion."""
    fig = {} if report is None else report
    assert np.array_equal(np.asarray(got["wetness_classes"]), np.asarray(want["wetness_classes"]))
    assert int(got["spatial_mode_count"]) == int(want["spatial_mode_count"])
    assert int(got["n_samples_fit"]) == int(want["n_samples_fit"])
    assert np.array_equal(np.asarray(got["weights"]), np.asarray(want["weights"]))
    assert np.array_equal(got["input_mean"], want["input_mean"])
    ev, ev_w = np.asarray(got["eigenvalues"]), np.asarray(want["eigenvalues"])
    lam_max = ev_w[0]
    assert ev.shape == ev_w.shape == (np.asarray(want["input_mean"]).shape[0],)
    fig["eigenvalues"] = float(np.max(np.abs(ev - ev_w)) / lam_max)
    assert fig["eigenvalues"] <= 1e-12, fig
    k = int(want["spatial_mode_count"])
    e, e_w = np.asarray(got["eofs"]), np.asarray(want["eofs"])
    assert e.shape == e_w.shape == (k, ev_w.shape[0])
    fig["eofs"] = 0.0
    for i in range(k):
        gap = min(abs(ev_w[i] - ev_w[j]) for j in (i - 1, i + 1) if 0 <= j < len(ev_w))
        bound = 1e-12 * lam_max / gap
        err = float(np.max(np.abs(e[i] - e_w[i])))
        fig["eofs"] = max(fig["eofs"], err / bound)
        assert err <= bound, (i, err, bound)
        j = np.argmax(np.abs(e_w[i]))
        assert np.sign(e[i, j]) == np.sign(e_w[i, j])
    if k:
        xs_w = np.asarray(want["x_std"])
        fig["x_mean"] = float(np.max(np.abs(np.asarray(got["x_mean"]) - want["x_mean"])) / xs_w[0])
        fig["x_std"] = float(np.max(np.abs(np.asarray(got["x_std"]) - xs_w) / xs_w))
        assert fig["x_mean"] <= 1e-12, fig
        assert fig["x_std"] <= 1e-11, fig
        if got.get("transform") is not None and want.get("transform") is not None:
            fig["transform"] = float(np.max(np.abs(np.asarray(got["transform"]) - np.asarray(want["transform"]))))
            assert fig["transform"] <= 1e-9, fig
    else:
        assert np.asarray(got["x_mean"]).shape == (0,) and np.asarray(got["x_std"]).shape == (0,)
