"""Generate tests/golden/pca_fit_ref_golden.npz FROM THE REFERENCE ITSELF: ``PreProcessor.fit`` (gpras/preprocess.py:947-1007)
with the scikit-learn ``IncrementalPCA`` it calls, ``compute_norths_rule`` (:1323-1353) and ``to_dict`` (:1135-1151).

Imports ``gpras.preprocess`` the way make_golden_pca_ref.py does (its last-resort finder hands out inert modules for the
reference's imports that are not installed here; nothing of them may be touched while the recorded calls run), with the
REAL scikit-learn and numpy of this container (their versions are recorded).  Inputs are re-seeded by ``pca_fit_ref_cases()``
below (pure numpy; the tests import it); the fixture holds outputs only.

    python tests/golden/make_golden_pca_fit_ref.py

Cases: wse / depth / velocity x weighted / unweighted x k given / North's rule, with always-dry cells, one cell whose
maximum depth equals the threshold exactly (class ""), n_wet not a multiple of 16 or 64, 7 to 60 samples, and one case
where no eigenvalue exceeds 1 (North's rule keeps 0 modes).  The generator asserts the margins that make the comparison
well posed: consecutive retained eigenvalues differ by >= 1e-3 relatively, no eigenvalue lies within 1e-6 of 1, and every
comparison North's rule makes is >= 2 % away from a tie.

Unweighted fits keep ``weights == np.empty(0)`` (:917), so the reference's transform cannot broadcast (:1031); the recorded
transform of those cases sets the attribute to None first (the branch its ``is not None`` guards describe).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
MODES = ("wse", "depth", "velocity")
THRESHOLD = 0.03

# (n_samples, n_cells, mode scales, k given) per (mode, weighted); the North's-rule cases reuse the shape with another seed
_SHAPES = {
    ("wse", True): (7, 97, (3.0, 1.2, 0.45), 2),
    ("wse", False): (23, 150, (2.5, 1.4, 1.3, 0.5), 3),
    ("depth", True): (31, 211, (2.0, 0.9, 0.35), 3),
    ("depth", False): (12, 131, (2.2, 1.0, 0.6, 0.25), 2),
    ("velocity", True): (47, 263, (1.5, 1.1, 0.5), 4),
    ("velocity", False): (60, 300, (1.8, 0.7, 0.3, 0.2), 3),
}
_SEED_SHIFT = {"depth_u_k": 1000}  # the first seed of this case put two retained eigenvalues too close (check_margins)


def _outer_sum(amp, pat):
    """amp @ pat with elementwise numpy only: a BLAS product rounds differently on different CPUs, these inputs may not."""
    out = amp[:, :1] * pat[0]
    for i in range(1, amp.shape[1]):
        out = out + amp[:, i : i + 1] * pat[i]
    return out


def pca_fit_ref_cases():
    """name -> dict(mode, weighted, k (None: North's rule), x, elevations, weights (None: unweighted)).  Pure numpy."""
    cases = {}
    for ci, ((mode, weighted), (n_s, cells, scales, k_given)) in enumerate(_SHAPES.items()):
        for kmode in ("k", "north"):
            name = f"{mode}_{'w' if weighted else 'u'}_{kmode}"
            rng = np.random.default_rng(20261016 + 17 * ci + (kmode == "north") + _SEED_SHIFT.get(name, 0))
            elev = 10.0 + 2.0 * rng.random(cells)
            dry = rng.random(cells) < 0.15
            dry[:3] = False
            elev[dry] += 50.0  # the water never reaches these cells
            r = len(scales)
            amp = rng.standard_normal((n_s, r)) * np.asarray(scales)
            pat = rng.standard_normal((r, cells))
            x = 11.0 + 0.5 * _outer_sum(amp, pat) + 0.01 * rng.standard_normal((n_s, cells))
            if mode == "velocity":
                x = x - 10.0
            else:
                # cell 1: always flooded and barely moving; cell 3: maximum depth exactly the threshold
                x[:, 1] = elev[1] + 1.0 + 0.01 * rng.standard_normal(n_s)
                elev[3] = 0.0
                x[:, 3] = THRESHOLD * (1.0 - 0.5 * rng.random(n_s))
                x[rng.integers(n_s), 3] = THRESHOLD
            weights = 0.5 + rng.random(cells) if weighted else None
            cases[name] = dict(
                mode=mode, weighted=weighted, k=None if kmode == "north" else k_given, x=np.ascontiguousarray(x), elevations=elev,
                weights=weights)
    # North's rule keeps nothing: every eigenvalue <= 1
    rng = np.random.default_rng(7)
    cells, n_s = 89, 9
    elev = 10.0 + rng.random(cells)
    x = elev + 0.5 + 0.004 * rng.standard_normal((n_s, cells))
    cases["wse_u_zero"] = dict(mode="wse", weighted=False, k=None, x=np.ascontiguousarray(x), elevations=elev, weights=None)
    return cases


def norths_rule_cases():
    """Eigenvalue lists for compute_norths_rule: separated (ind == 0), a near tie (ind > 0), nothing above 1 (empty)."""
    return {
        "separated": (np.array([50.0, 20.0, 6.0, 2.5, 0.4, 0.1]), 40),
        "tie": (np.array([50.0, 20.0, 19.0, 6.0, 0.5]), 30),
        "tie_first": (np.array([9.0, 8.9, 3.0, 0.2]), 25),
        "single": (np.array([4.0, 0.9, 0.3]), 10),  # the reference raises ValueError here (argmax of an empty array)
        "empty": (np.array([0.9, 0.5, 0.1]), 12),
    }


def check_margins(ev, n, k):
    """The comparison is well posed: distinct retained eigenvalues, none near 1, no near tie in North's rule."""
    ev = np.asarray(ev)
    assert np.all(np.abs(ev - 1.0) > 1e-6), "an eigenvalue lies within 1e-6 of 1"
    if k > 1:
        top = ev[:k]
        assert np.all((top[:-1] - top[1:]) / top[:-1] >= 1e-3), "retained eigenvalues are not separated"
    big = ev[ev > 1]
    if len(big) > 1:
        d_eigen = np.abs(np.diff(big))
        d_error = np.sqrt(2 / n) * big[:-1]
        upto = int(np.argmax(d_eigen <= d_error)) if np.any(d_eigen <= d_error) else len(d_eigen) - 1
        # the comparisons that decide the rule: every one up to its first "tie"
        assert np.all(np.abs(d_eigen - d_error)[: upto + 1] >= 0.02 * d_error[: upto + 1]), "North's rule compares a near tie"


def main():
    from make_golden_pca_ref import STUBBED, TOUCHED, import_reference_preprocess

    import sklearn
    from sklearn.decomposition import IncrementalPCA

    ref_pre = import_reference_preprocess()
    out = {}
    summary = {}
    keys = None
    TOUCHED.clear()
    for name, c in pca_fit_ref_cases().items():
        pp = ref_pre.PreProcessor(wet_threshold=THRESHOLD, hydraulic_parameter=c["mode"])
        pp.fit(c["x"].copy(), c["elevations"].copy(), None if c["weights"] is None else c["weights"].copy(), c["k"])
        k = int(pp.spatial_mode_count)
        check_margins(pp.eigenvalues, c["x"].shape[0], k)
        out[f"{name}/wetness_classes"] = np.asarray(pp.wetness_classes)
        out[f"{name}/input_mean"] = pp.input_mean
        out[f"{name}/weights"] = np.asarray(pp.weights)
        out[f"{name}/eofs"] = np.ascontiguousarray(pp.eofs)
        out[f"{name}/eigenvalues"] = pp.eigenvalues
        out[f"{name}/x_mean"] = pp.x_mean
        out[f"{name}/x_std"] = pp.x_std
        out[f"{name}/spatial_mode_count"] = np.array(k)
        out[f"{name}/n_samples_fit"] = np.array(int(pp.n_samples_fit))
        if c["weights"] is None:
            pp.weights = None
        out[f"{name}/transform"] = pp.transform(c["x"].copy())
        keys = sorted(pp.to_dict().keys())
        summary[name] = dict(shape=list(c["x"].shape), n_wet=int((~pp.dry_indices).sum()), k=k,
                             classes={s: int(np.sum(pp.wetness_classes == s)) for s in ("", "AD", "TF", "AF")})
    for name, (ev, n) in norths_rule_cases().items():
        pca = IncrementalPCA()
        pca.explained_variance_, pca.n_samples_seen_ = ev.copy(), n
        try:
            out[f"norths/{name}"] = np.array(ref_pre.compute_norths_rule(pca))
        except ValueError:  # exactly one eigenvalue above 1: np.argmax of an empty comparison raises (-1 records that)
            out[f"norths/{name}"] = np.array(-1)
    out["norths/not_a_pca"] = np.array(ref_pre.compute_norths_rule(object()))
    assert not TOUCHED, f"inert modules were used during the recorded calls: {TOUCHED[:10]}"
    meta = {
        "reference_file": "gpras/preprocess.py",
        "functions": ["PreProcessor.fit :947-1007", "transform :1009-1038", "to_dict :1135-1151", "compute_norths_rule :1323-1353"],
        "to_dict_keys": keys,
        "inert_modules": sorted(set(STUBBED)),
        "cases": summary,
        "python": sys.version.split()[0],
        "numpy": np.__version__,
        "sklearn": sklearn.__version__,
    }
    out["meta_json"] = np.array(json.dumps(meta, sort_keys=True))
    path = os.path.join(HERE, "pca_fit_ref_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes): " + ", ".join(f"{n} k={s['k']} n_wet={s['n_wet']}" for n, s in summary.items()))


if __name__ == "__main__":
    main()
