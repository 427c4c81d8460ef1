"""Generate tests/golden/hms_ref_golden.npz FROM THE REFERENCE ITSELF: ``HmsPreProcessor.fit`` / ``transform`` /
``calc_antecedent_precipitation_index`` / ``to_dict`` (gpras/preprocess.py:1165-1320) with the scikit-learn ``IncrementalPCA``
they call, and ``compute_norths_rule`` (:1323-1353).

Imports ``gpras.preprocess`` the way make_golden_pca_ref.py does (its last-resort finder hands out inert modules for the
reference's imports that are not installed here; nothing of them may be touched while the recorded calls run), with the
REAL scikit-learn and numpy of this container (their versions are recorded).  Inputs are re-seeded by ``hms_ref_cases()``
below (pure numpy; the tests import it); the fixture holds outputs only.

    python tests/golden/make_golden_hms_ref.py

Cases: T < p (one IncrementalPCA batch), p < T <= 5p, T > 5p with a final batch of one row; k given and North's rule;
precip columns interleaved with the bc columns; integer index masks (unsorted); always-dry precip cells; an all-zero bc
column (x_std NaN); one API call with window < len(x).  The generator asserts the margins that make the comparison well
posed: retained eigenvalues differ by >= 1e-3 relatively, and no comparison North's rule makes is within 2 % of a tie.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

# name -> (T, p, n_bc, latent scales, k given (None: North's rule), layout)
_SHAPES = {
    "t_lt_p": (40, 61, 3, (3.0, 1.6, 0.8), 3, "blocks"),
    "t_lt_p_north": (35, 50, 2, (2.5, 1.2, 0.5), None, "blocks"),
    "t_mid": (150, 47, 2, (2.0, 1.1, 0.45), 3, "blocks"),
    "t_mid_north": (173, 52, 3, (2.2, 1.0, 0.4), None, "blocks"),
    "t_gt_5p": (5 * 22 * 3 + 1, 22, 2, (1.8, 0.9, 0.5), 2, "blocks"),
    "t_gt_5p_north": (5 * 19 * 2 + 1, 19, 3, (2.0, 1.0, 0.45), None, "blocks"),
    "interleaved": (120, 30, 4, (2.4, 1.1), None, "interleaved"),
    "int_index": (90, 26, 3, (2.0, 0.9), 2, "index"),
    "dry_cells": (110, 36, 2, (2.3, 1.0, 0.5), None, "dry"),
    "zero_bc": (80, 24, 3, (2.0, 0.8), 2, "zero_bc"),
}
_SEED_SHIFT: dict = {}
API_CASE = dict(n=300, k=0.9, window=45)


def _outer_sum(amp, pat):
    """amp @ pat with elementwise numpy only: a BLAS product rounds differently on different CPUs, these inputs may not."""
    out = amp[:, :1] * pat[0]
    for i in range(1, amp.shape[1]):
        out = out + amp[:, i : i + 1] * pat[i]
    return out


def hms_ref_cases():
    """name -> dict(x (T, n_features), bc_mask, precip_mask, k (None: North's rule)).  Pure numpy."""
    cases = {}
    for ci, (name, (T, p, n_bc, scales, k, layout)) in enumerate(_SHAPES.items()):
        rng = np.random.default_rng(20261017 + 31 * ci + _SEED_SHIFT.get(name, 0))
        r = len(scales)
        amp = rng.standard_normal((T, r)) * np.asarray(scales)
        pat = rng.standard_normal((r, p))
        precip = 3.0 + 0.4 * _outer_sum(amp, pat) + 0.02 * rng.random((T, p))
        if layout == "dry":
            precip[:, rng.choice(p, 5, replace=False)] = 0.0  # cells where it never rains
        bc = 50.0 + 10.0 * rng.standard_normal((T, n_bc)) + 0.5 * np.arange(T)[:, None] / T
        if layout == "zero_bc":
            bc[:, 1] = 0.0
        nf = n_bc + p
        if layout == "interleaved":
            pcols = np.sort(rng.choice(nf, p, replace=False))
        else:
            pcols = np.arange(n_bc, nf)
        bcols = np.setdiff1d(np.arange(nf), pcols)
        x = np.empty((T, nf))
        x[:, pcols] = precip
        x[:, bcols] = bc
        if layout == "index":
            pm = rng.permutation(pcols)  # integer index arrays, not sorted
            bm = bcols[::-1].copy()
        else:
            pm = np.zeros(nf, dtype=bool)
            pm[pcols] = True
            bm = ~pm
        cases[name] = dict(x=x, bc_mask=bm, precip_mask=pm, k=k)
    return cases


def api_case():
    rng = np.random.default_rng(99)
    return rng.random(API_CASE["n"]) * (rng.random(API_CASE["n"]) < 0.3), API_CASE["k"], API_CASE["window"]


def check_margins(ev, n, k):
    """The comparison is well posed: distinct retained eigenvalues, no near tie in North's rule."""
    ev = np.asarray(ev)
    if k > 1:
        top = ev[: k + 1] if len(ev) > k else ev[:k]
        assert np.all((top[:-1] - top[1:]) / top[:-1] >= 1e-3), "retained eigenvalues are not separated"
    assert np.all(np.abs(ev - 1.0) > 1e-6), "an eigenvalue lies within 1e-6 of 1"
    big = ev[ev > 1]
    if len(big) > 1:
        d_eigen = np.abs(np.diff(big))
        d_error = np.sqrt(2 / n) * big[:-1]
        upto = int(np.argmax(d_eigen <= d_error)) if np.any(d_eigen <= d_error) else len(d_eigen) - 1
        assert np.all(np.abs(d_eigen - d_error)[: upto + 1] >= 0.02 * d_error[: upto + 1]), "North's rule compares a near tie"


def main():
    from make_golden_pca_ref import STUBBED, TOUCHED, import_reference_preprocess

    import sklearn

    ref_pre = import_reference_preprocess()
    out = {}
    summary = {}
    keys = None
    TOUCHED.clear()
    for name, c in hms_ref_cases().items():
        pp = ref_pre.HmsPreProcessor()
        pp.fit(c["x"].copy(), c["bc_mask"], c["precip_mask"], c["k"])
        k = int(pp.precip_spatial_mode_count)
        check_margins(pp.eigenvalues, c["x"].shape[0], k)
        for a in ("input_mean", "eigenvalues", "x_mean", "x_std"):
            out[f"{name}/{a}"] = np.asarray(pp.__dict__[a])
        out[f"{name}/eofs"] = np.ascontiguousarray(pp.eofs)
        out[f"{name}/precip_spatial_mode_count"] = np.array(k)
        out[f"{name}/n_samples_fit"] = np.array(int(pp.n_samples_fit))
        out[f"{name}/transform"] = pp.transform(c["x"].copy())
        keys = sorted(pp.to_dict().keys())
        summary[name] = dict(shape=list(c["x"].shape), p=int(pp.eofs.shape[1]), k=k, n_eofs=int(pp.eofs.shape[0]),
                             n_samples_fit_type=type(pp.n_samples_fit).__name__, nan_std=int(np.isnan(pp.x_std).sum()))
    a, k, window = api_case()
    out["api/window"] = ref_pre.HmsPreProcessor().calc_antecedent_precipitation_index(a.copy(), k=k, window=window)
    out["api/default"] = ref_pre.HmsPreProcessor().calc_antecedent_precipitation_index(a.copy())
    assert not TOUCHED, f"inert modules were used during the recorded calls: {TOUCHED[:10]}"
    meta = {
        "reference_file": "gpras/preprocess.py",
        "functions": ["HmsPreProcessor.fit :1208-1261", "transform :1263-1282", "calc_antecedent_precipitation_index :1284-1294",
                      "to_dict :1296-1307", "compute_norths_rule :1323-1353"],
        "to_dict_keys": keys,
        "inert_modules": sorted(set(STUBBED)),
        "cases": summary,
        "python": sys.version.split()[0],
        "numpy": np.__version__,
        "sklearn": sklearn.__version__,
    }
    out["meta_json"] = np.array(json.dumps(meta, sort_keys=True))
    path = os.path.join(HERE, "hms_ref_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes): " + ", ".join(f"{n} k={s['k']}" for n, s in summary.items()))


if __name__ == "__main__":
    main()
