"""A numpy restatement of the reference's PreProcessor.fit (gpras/preprocess.py:947-1007) with the single-batch
IncrementalPCA it calls (sklearn partial_fit, first batch: X -= col_mean, SVD, svd_flip(u_based_decision=False),
explained_variance_ = S^2 / (n - 1)).  Shared by the CPU pins and the GPU parity tests."""

import numpy as np

from gpras_amd.preprocess import PCAFit, compute_norths_rule


def classify(max_depth, min_depth, thr):
    """_classify_depths (:1128-1133)."""
    classes = np.empty(max_depth.shape, dtype="<U2")
    classes[max_depth < thr] = "AD"
    classes[max_depth > thr] = "TF"
    classes[min_depth > thr] = "AF"
    return classes


def svd_flip_rows(u, vt):
    """sklearn's svd_flip(u, v, u_based_decision=False): the largest |entry| of each row of vt becomes positive."""
    idx = np.argmax(np.abs(vt), axis=1)
    signs = np.sign(vt[np.arange(vt.shape[0]), idx])
    return u * signs[np.newaxis, :], vt * signs[:, np.newaxis]


def single_batch_pca(x):
    """(components_, explained_variance_) of IncrementalPCA().fit(x) for samples <= 5 * features (one batch)."""
    n = x.shape[0]
    xc = x - x.sum(axis=0) / n
    u, s, vt = np.linalg.svd(xc, full_matrices=False)
    u, vt = svd_flip_rows(u, vt)
    return vt, s**2 / (n - 1)


def fit_reference(x, elevations, weights, k, mode, thr=0.03):
    """Every attribute PreProcessor.fit sets, as a dict (weights: the compacted weights, np.empty(0) when unweighted)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if mode == "depth":
        x = np.maximum(x - elevations, 0.0)
        classes = classify(x.max(axis=0), x.min(axis=0), thr)
    elif mode == "wse":
        classes = classify(x.max(axis=0) - elevations, x.min(axis=0) - elevations, thr)
    else:
        classes = np.repeat("TF", x.shape[1])
    dry = classes == "AD"
    xw = np.asfortranarray(x[:, ~dry])  # what boolean indexing of the second axis returns: Fortran order
    input_mean = xw.mean(axis=0)  # so every column is one contiguous run, reduced in numpy's pairwise order
    xw = xw - input_mean
    w = np.empty(0)
    if weights is not None:
        w = weights[~dry]
        xw *= w
    comps, ev = single_batch_pca(xw)
    pca = PCAFit(explained_variance_=ev, n_samples_seen_=x.shape[0], components_=comps)
    k = compute_norths_rule(pca) if k is None else k
    eofs = comps[:k]
    z = xw @ eofs.T
    return dict(wetness_classes=classes, input_mean=input_mean, weights=w, eofs=eofs, eigenvalues=ev, spatial_mode_count=k,
                n_samples_fit=x.shape[0], x_mean=z.mean(axis=0), x_std=z.std(axis=0))


def assert_fit_close(got, want, exact_mean=True):
    """The bounds of the fit's parity table."""
    assert np.array_equal(np.asarray(got["wetness_classes"]), np.asarray(want["wetness_classes"]))
    assert int(got["spatial_mode_count"]) == int(want["spatial_mode_count"])
    assert int(got["n_samples_fit"]) == int(want["n_samples_fit"])
    assert np.array_equal(np.asarray(got["weights"]), np.asarray(want["weights"]))
    if exact_mean:
        assert np.array_equal(got["input_mean"], want["input_mean"])
    else:
        assert np.allclose(got["input_mean"], want["input_mean"], rtol=1e-15, atol=0)
    ev, ev_w = np.asarray(got["eigenvalues"]), np.asarray(want["eigenvalues"])
    lam_max = ev_w[0]
    assert ev.shape == ev_w.shape
    assert np.max(np.abs(ev - ev_w)) <= 1e-12 * lam_max, np.max(np.abs(ev - ev_w)) / lam_max
    k = int(want["spatial_mode_count"])
    e, e_w = np.asarray(got["eofs"]), np.asarray(want["eofs"])
    assert e.shape == e_w.shape == (k, want["input_mean"].shape[0])
    for i in range(k):
        bound = 1e-13 * lam_max / ev_w[i]
        err = np.max(np.abs(e[i] - e_w[i]))
        assert err <= bound, (i, err, bound)
        j = np.argmax(np.abs(e_w[i]))
        assert np.sign(e[i, j]) == np.sign(e_w[i, j])
    if k:
        xs_w = np.asarray(want["x_std"])
        assert np.max(np.abs(np.asarray(got["x_mean"]) - want["x_mean"])) <= 1e-12 * xs_w[0]
        assert np.max(np.abs(np.asarray(got["x_std"]) - xs_w) / xs_w) <= 1e-11
    else:
        assert np.asarray(got["x_mean"]).shape == (0,) and np.asarray(got["x_std"]).shape == (0,)
