"""A numpy restatement of the reference's HmsPreProcessor (gpras/preprocess.py:1165-1320) with the IncrementalPCA it calls,
written the way the device computes it: the covariance route (T >= p: eigh of X2^T X2, eigenvectors as components) or the
Gram route (T < p: one batch, SVD), explained_variance_ = S^2 / (T - 1), svd_flip(u_based_decision=False).  Shared by the CPU
pins and the GPU parity tests."""

import numpy as np

from gpras_amd.preprocess import PCAFit, compute_norths_rule


def flip_rows(vt):
    """svd_flip(u_based_decision=False): the first largest |entry| of each row becomes positive."""
    idx = np.argmax(np.abs(vt), axis=1)
    return vt * np.sign(vt[np.arange(vt.shape[0]), idx])[:, None]


def incremental_pca(xp):
    """(components_, explained_variance_) of IncrementalPCA().fit(xp), all min(T, p) of them."""
    T, p = xp.shape
    x2 = xp - np.asfortranarray(xp).mean(axis=0)
    if T >= p:
        lam, v = np.linalg.eigh(x2.T @ x2)
        lam, v = np.maximum(lam[::-1], 0.0), v[:, ::-1]
        comps = flip_rows(np.ascontiguousarray(v.T))
    else:
        _, s, vt = np.linalg.svd(x2, full_matrices=False)
        lam, comps = s**2, flip_rows(vt)
    return comps, lam / (T - 1)


def api(a, k=0.85, window=None):
    """calc_antecedent_precipitation_index (:1284-1294)."""
    if window is None:
        window = len(a)
    w = np.array([k**i for i in range(window)])
    return np.convolve(a, w, mode="full")[: len(a), np.newaxis]


def api_fast(a, k):
    """The same sums for window = len(a) without the O(T^2) convolution: the zero tail of 0.85**i cut, k = 1 as a cumulative
    sum in extended precision (for large T only; its rounding differs from np.convolve's, within the parity bounds)."""
    if k == 1:
        return np.cumsum(a.astype(np.longdouble)).astype(np.float64)[:, None]
    w = []
    for i in range(len(a)):
        v = k**i
        if v == 0:
            break
        w.append(v)
    return np.convolve(a, np.array(w), mode="full")[: len(a), np.newaxis]


def columns(mask, n):
    return np.arange(n)[np.asarray(mask)]


def features(x, input_mean, bc_mask, precip_mask, eofs, fast_api=False):
    xc = x - input_mean
    n = x.shape[1]
    xb, xp = xc[:, columns(bc_mask, n)], xc[:, columns(precip_mask, n)]
    avg = xp.mean(axis=1)
    a1, a2 = (api_fast(avg, 0.85), api_fast(avg, 1)) if fast_api else (api(avg), api(avg, k=1))
    return np.concatenate([xb, xp @ eofs.T, avg[:, None], a1, a2], axis=1)


def fit_reference(x, bc_mask, precip_mask, k=None, fast_api=False):
    """Every attribute HmsPreProcessor.fit sets, as a dict."""
    x = np.asarray(x, dtype=np.float64)
    input_mean = np.asfortranarray(x).mean(axis=0)
    xp = (x - input_mean)[:, columns(precip_mask, x.shape[1])]
    comps, ev = incremental_pca(xp)
    pca = PCAFit(explained_variance_=ev, n_samples_seen_=x.shape[0], components_=comps)
    k = compute_norths_rule(pca) if k is None else k
    eofs = comps[:k]
    f = features(x, input_mean, bc_mask, precip_mask, eofs, fast_api)
    x_std = np.array([np.std(f[f[:, i] != 0, i]) if np.any(f[:, i] != 0) else np.nan for i in range(f.shape[1])])
    return dict(input_mean=input_mean, eofs=eofs, eigenvalues=ev, precip_spatial_mode_count=k, n_samples_fit=x.shape[0],
                x_mean=f.mean(axis=0), x_std=x_std)


def transform_reference(state, x, fast_api=False):
    f = features(np.asarray(x, dtype=np.float64), state["input_mean"], state["bc_mask"], state["precip_mask"], state["eofs"], fast_api)
    return (f - state["x_mean"]) / state["x_std"]


def assert_close(a, b, rel, what):
    """|a - b| <= rel * max(1, |b|) elementwise, NaN exactly where b is NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN positions differ"
    ok = ~np.isnan(b)
    err = np.abs(a[ok] - b[ok]) / np.maximum(1.0, np.abs(b[ok]))
    assert err.size == 0 or err.max() <= rel, (what, float(err.max()))


def assert_fit_close(got, want, x):
    """The bounds of DESIGN.md section 3.13."""
    assert int(got["precip_spatial_mode_count"]) == int(want["precip_spatial_mode_count"])
    assert int(got["n_samples_fit"]) == int(want["n_samples_fit"])
    xmax = np.max(np.abs(x), axis=0)
    assert np.all(np.abs(got["input_mean"] - want["input_mean"]) <= 1e-14 * xmax), "input_mean"
    ev, ev_w = np.asarray(got["eigenvalues"]), np.asarray(want["eigenvalues"])
    assert ev.shape == ev_w.shape
    lam_max = ev_w[0]
    assert np.max(np.abs(ev - ev_w)) <= 1e-12 * lam_max, np.max(np.abs(ev - ev_w)) / lam_max
    e, e_w = np.asarray(got["eofs"]), np.asarray(want["eofs"])
    assert e.shape == e_w.shape
    for i in range(e_w.shape[0]):
        gaps = [abs(ev_w[i] - ev_w[j]) for j in (i - 1, i + 1) if 0 <= j < len(ev_w)]
        bound = 1e-12 * lam_max / min(gaps)
        err = np.max(np.abs(e[i] - e_w[i]))
        assert err <= bound, (i, err, bound)
    # x_mean of a centred column is rounding noise: its bound scales with the column's spread
    xs_w = np.asarray(want["x_std"])
    assert_close(got["x_std"], xs_w, 1e-10, "x_std")
    scale = np.maximum(np.abs(want["x_mean"]), np.nan_to_num(xs_w, nan=0.0))
    assert np.all(np.abs(np.asarray(got["x_mean"]) - want["x_mean"]) <= 1e-10 * scale), "x_mean"
