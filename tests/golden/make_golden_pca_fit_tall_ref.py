"""Generate tests/golden/pca_fit_tall_ref_golden.npz FROM THE REFERENCE ITSELF: ``PreProcessor.fit`` (gpras/preprocess.py:947-1007)
with the scikit-learn ``IncrementalPCA`` it calls, on inputs with MORE SAMPLES THAN WET CELLS -- one batch of more rows than columns
(n_wet < n_samples <= 5 n_wet) and several batches (beyond 5 n_wet) -- which the covariance route of the device fit serves
(``PreProcessor.sample_route = "auto"``).

Imports ``gpras.preprocess`` through ``make_golden_pca_ref.import_reference_preprocess`` as make_golden_pca_fit_ref.py does, with the
real scikit-learn and numpy of this container (versions recorded).  Inputs are re-seeded by ``pca_fit_tall_ref_cases()`` below (pure
numpy; the tests import it); the fixture holds outputs only.

    python tests/golden/make_golden_pca_fit_tall_ref.py

Cases: wse / depth / velocity x weighted / unweighted x k given / North's rule, every one with always-dry cells (wse, depth), one
cell whose maximum depth equals the threshold exactly (class "") and n_wet not a multiple of 16, over four sample counts:
n_samples = n_wet + 1; one batch of about 3 n_wet; n_samples = 5 n_wet + 1 (two batches, the last of one row); three or more
batches.  One deep case, (8201, 29), crosses the 8192-row piece of numpy's column sums; its ``transform`` is omitted to keep the file
small.  The generator asserts the margins of make_golden_pca_fit_ref.py (``check_margins``).

The reference alone stays inside the bounds the tests apply (tests/pca_fit_tall_numpy.py ``assert_tall_fit_close``): the generator
asserts that the numpy restatement of the covariance route meets them against every recorded fit, and prints the largest figure of
each kind as a fraction of its bound.  On this container (numpy 2.2.6, scikit-learn 1.7.2) the margin is more than 100.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_pca_fit_ref import THRESHOLD, _outer_sum, check_margins  # noqa: E402

# (n_wet, n_dry for wse / depth, mode scales, k given) per (mode, weighted)
_SHAPES = {
    ("wse", True): (37, 6, (3.0, 1.2, 0.45), 2),
    ("wse", False): (45, 5, (2.5, 1.4, 0.8, 0.3), 3),
    ("depth", True): (29, 7, (2.0, 0.9, 0.35), 3),
    ("depth", False): (21, 4, (2.2, 1.0, 0.6, 0.25), 2),
    ("velocity", True): (33, 0, (1.5, 1.1, 0.5), 4),
    ("velocity", False): (26, 0, (1.8, 0.7, 0.3, 0.2), 3),
}
# sample count from n_wet: the four kinds are dealt over the twelve cases in turn
_KINDS = (("plus1", lambda n: n + 1), ("onebatch", lambda n: 3 * n - 2), ("twobatch", lambda n: 5 * n + 1), ("manybatch", lambda n: 15 * n + 11))
_SEED_SHIFT = {}


def _case(rng, mode, weighted, n_s, n_wet, n_dry, scales):
    cells = n_wet + n_dry
    elev = 9.5 + 1.5 * rng.random(cells)  # below the top of every cell's range: only the cells chosen next are always dry
    dry = np.zeros(cells, dtype=bool)
    if n_dry:
        dry[4 + rng.choice(cells - 4, size=n_dry, replace=False)] = True
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
    return dict(mode=mode, weighted=weighted, x=np.ascontiguousarray(x), elevations=elev, weights=weights, n_wet=n_wet)


def pca_fit_tall_ref_cases():
    """name -> dict(mode, weighted, k (None: North's rule), x, elevations, weights (None: unweighted), n_wet, kind).  Pure numpy."""
    cases = {}
    turn = 0
    for ci, ((mode, weighted), (n_wet, n_dry, scales, k_given)) in enumerate(_SHAPES.items()):
        for kmode in ("k", "north"):
            kind, rows_of = _KINDS[(turn + ci) % len(_KINDS)]  # (+ ci: weighted and unweighted cases both meet every kind)
            turn += 1
            name = f"{mode}_{'w' if weighted else 'u'}_{kmode}_{kind}"
            rng = np.random.default_rng(20261020 + 17 * ci + (kmode == "north") + _SEED_SHIFT.get(name, 0))
            c = _case(rng, mode, weighted, rows_of(n_wet), n_wet, n_dry, scales)
            c.update(k=None if kmode == "north" else k_given, kind=kind)
            cases[name] = c
    # the deep case: more rows than one piece of numpy's buffered column sum
    rng = np.random.default_rng(8201)
    c = _case(rng, "wse", False, 8201, 26, 3, (2.0, 1.0, 0.4))
    c.update(k=2, kind="deep")
    cases["wse_u_k_deep"] = c
    return cases


def main():
    from make_golden_pca_ref import STUBBED, TOUCHED, import_reference_preprocess

    import sklearn

    for path in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):  # tests/ (pca_fit_tall_numpy), the repository (gpras_amd)
        if path not in sys.path:
            sys.path.insert(0, path)
    from pca_fit_tall_numpy import assert_tall_fit_close, fit_reference_tall

    ref_pre = import_reference_preprocess()
    out = {}
    summary = {}
    worst = {}
    TOUCHED.clear()
    for name, c in pca_fit_tall_ref_cases().items():
        pp = ref_pre.PreProcessor(wet_threshold=THRESHOLD, hydraulic_parameter=c["mode"])
        pp.fit(c["x"].copy(), c["elevations"].copy(), None if c["weights"] is None else c["weights"].copy(), c["k"])
        k = int(pp.spatial_mode_count)
        n_s = c["x"].shape[0]
        n_wet = int((~pp.dry_indices).sum())
        assert n_wet == c["n_wet"] and n_wet % 16 != 0 and n_s > n_wet, (name, n_wet)
        assert np.sum(pp.wetness_classes == "") == (c["mode"] != "velocity"), name
        assert len(pp.eigenvalues) == n_wet and int(pp.n_samples_fit) == n_s, name
        check_margins(pp.eigenvalues, n_s, k)
        rec = dict(wetness_classes=np.asarray(pp.wetness_classes), input_mean=pp.input_mean, weights=np.asarray(pp.weights),
                   eofs=np.ascontiguousarray(pp.eofs), eigenvalues=pp.eigenvalues, x_mean=pp.x_mean, x_std=pp.x_std,
                   spatial_mode_count=np.array(k), n_samples_fit=np.array(int(pp.n_samples_fit)))
        if c["weights"] is None:
            pp.weights = None
        if c["kind"] != "deep":
            rec["transform"] = pp.transform(c["x"].copy())
        # the reference against the restatement of the covariance route, under the bounds of the tests
        fig = {}
        assert_tall_fit_close(fit_reference_tall(c["x"], c["elevations"], c["weights"], c["k"], c["mode"], THRESHOLD), rec, report=fig)
        bounds = dict(eigenvalues=1e-12, eofs=1.0, x_mean=1e-12, x_std=1e-11, transform=1e-9)
        for key, v in fig.items():
            worst[key] = max(worst.get(key, 0.0), v / bounds[key])
        for key, v in rec.items():
            out[f"{name}/{key}"] = v
        summary[name] = dict(shape=list(c["x"].shape), n_wet=n_wet, k=k, kind=c["kind"],
                             classes={s: int(np.sum(pp.wetness_classes == s)) for s in ("", "AD", "TF", "AF")})
    assert not TOUCHED, f"inert modules were used during the recorded calls: {TOUCHED[:10]}"
    assert max(worst.values()) <= 1e-2, worst  # the reference itself uses less than a hundredth of every bound
    meta = {
        "reference_file": "gpras/preprocess.py",
        "functions": ["PreProcessor.fit :947-1007", "transform :1009-1038"],
        "inert_modules": sorted(set(STUBBED)),
        "cases": summary,
        "worst_fraction_of_bound": worst,
        "python": sys.version.split()[0],
        "numpy": np.__version__,
        "sklearn": sklearn.__version__,
    }
    out["meta_json"] = np.array(json.dumps(meta, sort_keys=True))
    path = os.path.join(HERE, "pca_fit_tall_ref_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes): " + ", ".join(f"{n} k={s['k']} n_wet={s['n_wet']}" for n, s in summary.items()))
    print("largest figure as a fraction of its bound:", worst)


if __name__ == "__main__":
    main()
