"""Generate tests/golden/events_ref_golden.npz FROM THE REFERENCE ITSELF: ``EventSelection`` of
``production/pre_processing/event_selection.py`` (:13-257), constructed on a temporary parquet file per case and run unchanged with the
numpy, pandas, scipy, scikit-learn and pyarrow of this container (versions recorded).

    python tests/golden/make_golden_events_ref.py [path to the reference checkout]

Inputs come from ``events_ref_cases()`` below (pure numpy; the tests import it): gamma-shaped pulses with random amplitude, ragged event
lengths, shuffled rows and ids.  The fixture holds outputs only, plus one checksum per input array.

Cases (E events, H = longest event):
  A  257 x 24, arrival_rate 10   ragged; last block of 7 events; events below the lowest knot (negative return periods)
  B  1030 x 65, arrival_rate 10  H crosses a wave (64)
  C  64 x 70, arrival_rate 4     E < H; scikit-learn's "full" solver
  D  120 x 30, arrival_rate 10   equal lengths but for one single-row event; two blocks share a maximum of either variable (made so);
                                 every block's top event has a maximum equal to a knot

Recorded per case: ``event_max``; the ``_select_aep_storms`` frame (ids, Set, index); the ``_select_diverse_storms`` ids; the
``_select_test_storms`` ids; the ``run_selection`` result.  The standardised scores are what passes through the reference's own
``StandardScaler().fit_transform`` call (:165-167) while ``_select_diverse_storms`` runs (the module's ``PCA`` and ``StandardScaler`` are
replaced for the duration by subclasses that keep their inputs and outputs); the pick order comes from the reference alone as well:
``_select_diverse_storms(ids, m)`` for m = 1 .. num adds exactly one id per step.

Conditions on the inputs, asserted here (not tolerances of any test):
  1. every fitted PCA reports a solver other than "randomized";
  2. (lambda_i - lambda_{i+1}) / lambda_1 >= 1e-4 for i <= n_components, both pivots;
  3. every greedy pick beats the runner-up by at least 1e-6 relative (in distance);
  4. the numpy restatement (tests/events_numpy.py) agrees with everything recorded: maxima and return periods bit for bit, the ids and
     the pick order exactly, the scores within 16 x ``score_dev_two_routes``.
``score_dev_two_routes``: the largest difference, per case, between the standardised scores as the reference computed them and the
same matrix from an SVD of each centred pivot (signs aligned, standardised with numpy).  Where scikit-learn's solver is "full" -- which
is that SVD, the same LAPACK call, so the two routes are one -- the second route is the eigenvectors of Xc^T Xc instead.
Case B keeps the scores of every fourth row only (``B/scores_rows``), to keep the fixture small.
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

N_COMPONENTS = 5
# name -> (E, H, arrival_rate, n_train, n_test, target_rps, test_rp_range)
CASES = {
    "A": (257, 24, 10, 14, 4, [2, 5, 10, 25], [1.05, 2000]),
    "B": (1030, 65, 10, 30, 8, [2, 5, 10, 25, 50, 100], [1.5, 2000]),
    "C": (64, 70, 4, 10, 2, [2, 5, 10], [1.05, 2000]),
    "D": (120, 30, 10, 10, 2, [2, 5, 10], [1.05, 2000]),
}
SEEDS = {"A": 14, "B": 12, "C": 13, "D": 15}
COLLIDE = (2, 7)  # case D: these two blocks (in id order) share their maximum


def _pulse(t, peak, shape):
    """A gamma-shaped pulse with its maximum 1 at t = peak."""
    x = np.maximum(t, 0.0) / peak
    return x**shape * np.exp(shape * (1.0 - x))


def events_ref_cases():
    """name -> dict(event_id, datetime, precip_excess, precip_cum, inflow, arrival_rate, ...): the long-format columns, rows shuffled."""
    out = {}
    for name, (E, H, ar, n_train, n_test, target_rps, test_range) in CASES.items():
        rng = np.random.default_rng(20261018 + SEEDS[name])
        ids = np.sort(rng.choice(10 * E, size=E, replace=False)).astype(np.int64) + 100
        if name == "D":
            lengths = np.full(E, H)
            lengths[41] = 1
        else:
            lengths = rng.integers(max(2, H // 2), H + 1, size=E)
            lengths[rng.integers(0, E)] = H
        series = []
        for e in range(E):
            n = int(lengths[e])
            t = np.arange(n, dtype=np.float64)
            amp = np.exp(rng.normal(0.0, 0.9))
            pe = 0.4 * amp * _pulse(t + 1.0, 2.0 + 0.35 * H * rng.random(), 1.5 + 2.0 * rng.random())
            if rng.random() < 0.4:  # a second burst
                pe = pe + 0.3 * amp * rng.random() * _pulse(t + 1.0, 0.5 * H + 0.3 * H * rng.random(), 3.0 + 2.0 * rng.random())
            q = -3.0 + 40.0 * rng.random() + 900.0 * amp * np.exp(rng.normal(0.0, 0.35)) * _pulse(t + 1.0, 4.0 + 0.45 * H * rng.random(), 2.0 + 2.0 * rng.random())
            series.append([pe, np.cumsum(pe), q])
        if name == "D":
            # two blocks share their maximum, of precip-cum and of inflow: the top event of one block is scaled up to the other's top
            for col in (1, 2):
                mx = np.array([s[col].max() for s in series])
                tops = [int(np.argmax(mx[b * ar : (b + 1) * ar])) + b * ar for b in COLLIDE]
                a, b = (tops[0], tops[1]) if mx[tops[0]] > mx[tops[1]] else (tops[1], tops[0])
                s = series[b][col] * (mx[a] / mx[b])
                s[int(np.argmax(s))] = mx[a]
                series[b][col] = s
                assert s.max() == mx[a]
        start = np.datetime64("2026-01-01T00:00:00", "ns") + (rng.integers(0, 24 * 365, size=E) * 3600 * 10**9).astype("timedelta64[ns]")
        ev = np.concatenate([np.full(int(lengths[e]), ids[e]) for e in range(E)])
        dt = np.concatenate([start[e] + (np.arange(int(lengths[e])) * 3600 * 10**9).astype("timedelta64[ns]") for e in range(E)])
        cols = [np.concatenate([s[c] for s in series]) for c in range(3)]
        perm = rng.permutation(ev.size)
        out[name] = dict(event_id=ev[perm], datetime=dt[perm], precip_excess=cols[0][perm], precip_cum=cols[1][perm], inflow=cols[2][perm],
                         arrival_rate=ar, n_events=E, n_hours=H, n_train=n_train, n_test=n_test, target_rps=list(target_rps),
                         test_rp_range=list(test_range), n_components=N_COMPONENTS)
    return out


def input_checksums(cases):
    out = {}
    for name, c in cases.items():
        for col in ("precip_excess", "precip_cum", "inflow"):
            out[f"{name}/{col}"] = float(np.sum(c[col]))
        out[f"{name}/event_id"] = int(np.sum(c["event_id"] * (np.arange(c["event_id"].size) % 7 + 1)))
        out[f"{name}/datetime"] = int(np.sum(c["datetime"].astype(np.int64) // 10**9 % 1000003))
    return out


def align_signs(a, b):
    """b with every column turned to the side of a's."""
    s = np.sign(np.sum(a * b, axis=0))
    s[s == 0] = 1.0
    return b * s


def main():
    import pandas as pd
    import pyarrow
    import scipy
    import sklearn

    import events_numpy as en

    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GPRAS_REFERENCE", "/root/reference")
    sys.path.insert(0, os.path.join(ref_root, "production", "pre_processing"))
    import event_selection as ref_mod

    class RecordingPCA(ref_mod.PCA):
        fitted = []

        def fit_transform(self, X, y=None):
            x = np.array(X, dtype=np.float64)
            z = super().fit_transform(X, y)
            RecordingPCA.fitted.append((x, np.array(z), self._fit_svd_solver))
            return z

    class RecordingScaler(ref_mod.StandardScaler):
        outputs = []

        def fit_transform(self, X, y=None, **kw):
            z = super().fit_transform(X, y, **kw)
            RecordingScaler.outputs.append(np.array(z))
            return z

    cases = events_ref_cases()
    out, summary = {}, {}
    for name, c in cases.items():
        k = c["n_components"]
        df = pd.DataFrame({"event_id": c["event_id"], "datetime": c["datetime"], "precip-excess": c["precip_excess"], "precip-cum": c["precip_cum"],
                           "inflow": c["inflow"]})
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "storms.pq")
            df.to_parquet(path)
            with np.errstate(all="ignore"):
                ref = ref_mod.EventSelection(path, arrival_rate=c["arrival_rate"], test_rp_range=c["test_rp_range"])
        em = ref.event_max
        for col in ("event_id", "precip-cum", "inflow", "RP_precip-cum", "RP_inflow"):
            out[f"{name}/event_max/{col}"] = em[col].to_numpy()
        with np.errstate(all="ignore"):
            aep = ref._select_aep_storms(c["target_rps"])
        out[f"{name}/aep/event_id"] = aep["event_id"].to_numpy(dtype=np.float64)
        out[f"{name}/aep/index"] = aep.index.to_numpy(dtype=np.int64)
        out[f"{name}/aep/set"] = aep["Set"].to_numpy().astype(str)
        sel_ids = aep.event_id.tolist()
        num = c["n_train"] - len(aep)
        assert num >= 3, (name, len(aep))

        ref_mod.PCA, ref_mod.StandardScaler = RecordingPCA, RecordingScaler
        RecordingPCA.fitted, RecordingScaler.outputs = [], []
        try:
            diverse = ref._select_diverse_storms(sel_ids, num)
            pcas, scores = list(RecordingPCA.fitted), RecordingScaler.outputs[0]
            order, have = [], set()
            for m in range(1, num + 1):  # the pick order, from the reference alone: one more id per step
                step = set(ref._select_diverse_storms(sel_ids, m).event_id.tolist())
                new = step - have
                assert len(new) == 1 and have <= step, (name, m)
                order.append(new.pop())
                have = step
        finally:
            ref_mod.PCA, ref_mod.StandardScaler = RecordingPCA.__mro__[1], RecordingScaler.__mro__[1]
        assert set(order) == set(diverse.event_id.tolist())
        out[f"{name}/diverse/event_id"] = diverse["event_id"].to_numpy()
        out[f"{name}/diverse/order"] = np.array(order, dtype=np.int64)
        keep = np.arange(0, scores.shape[0], 4 if name == "B" else 1)
        out[f"{name}/scores"], out[f"{name}/scores_rows"] = scores[keep], keep

        excluded = sel_ids + diverse.event_id.tolist()
        test = ref._select_test_storms(c["test_rp_range"], c["n_test"], excluded)
        out[f"{name}/test/event_id"] = test["event_id"].to_numpy()
        with np.errstate(all="ignore"):
            selected, _ = ref.run_selection(c["n_train"], c["n_test"], c["target_rps"])
        out[f"{name}/run/event_id"] = selected["event_id"].to_numpy(dtype=np.float64)
        out[f"{name}/run/set"] = selected["Set"].to_numpy().astype(str)
        out[f"{name}/run/type"] = selected["Type"].to_numpy().astype(str)

        # ---- condition 1 and the two routes ---------------------------------------------------------------------------------------
        assert len(pcas) == 2 and all(p[2] != "randomized" for p in pcas), [p[2] for p in pcas]
        def standardised(blocks):
            z = np.concatenate(blocks, axis=1)
            return (z - z.mean(axis=0)) / z.std(axis=0)

        gaps, svd_blocks, eigh_blocks = [], [], []
        for x, z, _ in pcas:
            xc = x - x.mean(axis=0)
            u, s, vt = np.linalg.svd(xc, full_matrices=False)
            svd_blocks.append(u[:, :k] * s[:k])
            w, v = np.linalg.eigh(xc.T @ xc)
            eigh_blocks.append(xc @ v[:, ::-1][:, :k])
            lam = s**2 / (x.shape[0] - 1)
            gaps.append(float(np.min((lam[:k] - lam[1 : k + 1]) / lam[0])))
        assert np.allclose(standardised([z for _, z, _ in pcas]), scores, rtol=0, atol=1e-13)  # the recorded blocks are the scaler's input
        two_routes = float(np.max(np.abs(align_signs(scores, standardised(svd_blocks)) - scores)))
        if all(p[2] == "full" for p in pcas):
            # scikit-learn's "full" solver IS the SVD of the centred matrix (the same LAPACK call): the two routes are one, and their
            # difference shows the scaler's rounding only.  The second route is then the eigenvectors of Xc^T Xc.
            two_routes = float(np.max(np.abs(align_signs(scores, standardised(eigh_blocks)) - scores)))
        assert min(gaps) >= 1e-4, (name, gaps)  # condition 2

        # ---- the restatement (conditions 3 and 4) -----------------------------------------------------------------------------------
        ids, rank, hour = en.rank_and_hour(c["event_id"], c["datetime"])
        E, H = ids.size, int(hour.max()) + 1
        assert (E, H) == (c["n_events"], c["n_hours"]) and np.array_equal(ids, em["event_id"].to_numpy())
        for col, key in (("precip_cum", "precip-cum"), ("inflow", "inflow")):
            mx = en.event_maxima(rank, c[col], E)
            assert np.array_equal(mx, em[key].to_numpy()), (name, key)
            xk, yk = en.knots(mx, c["arrival_rate"])
            assert np.array_equal(en.rp_eval(xk, yk, mx), em["RP_" + key].to_numpy()), (name, key)
            if name == "D":
                nb = -(-E // c["arrival_rate"])
                assert xk.size == nb - 1, (name, key, xk.size, nb)  # two blocks collide
                assert np.count_nonzero(np.isin(mx, xk)) >= xk.size
        if name == "A":
            assert E % c["arrival_rate"] == 7 and min(em["RP_precip-cum"].min(), em["RP_inflow"].min()) < 0.0
        mine = en.diverse_scores(en.pivot(rank, hour, c["precip_excess"], E, H), en.pivot(rank, hour, c["inflow"], E, H), k)
        score_err = float(np.max(np.abs(align_signs(scores, mine) - scores)))
        assert score_err <= 16.0 * two_routes, (name, score_err, two_routes)
        sel_rows = np.unique(np.searchsorted(ids, np.array(sel_ids)))
        picks, _, margin2 = en.farthest(scores, sel_rows, num, margins=True)
        margin = 1.0 - np.sqrt(1.0 - margin2)  # of squared distances -> of distances
        assert np.array_equal(ids[picks], np.array(order)), (name, ids[picks], order)
        assert margin.min() >= 1e-6, (name, margin.min())  # condition 3
        picks_mine = en.farthest(align_signs(scores, mine), sel_rows, num)[0]
        assert np.array_equal(picks_mine, picks), name
        out[f"{name}/score_dev_two_routes"] = np.array(two_routes)
        summary[name] = dict(E=E, H=H, rows=int(c["event_id"].size), solvers=[p[2] for p in pcas], score_dev_two_routes=two_routes, restatement_score_err=score_err,
                             min_gap=min(gaps), min_pick_margin=float(margin.min()), n_aep=int(len(aep)), n_diverse=int(num), n_test=int(len(test)),
                             min_rp=float(min(em["RP_precip-cum"].min(), em["RP_inflow"].min())))

    meta = {
        "reference_file": "production/pre_processing/event_selection.py",
        "functions": ["EventSelection._calculate_return_periods :34-67", "EventSelection._select_aep_storms :73-146",
                      "EventSelection._select_diverse_storms :148-185", "EventSelection._select_test_storms :187-237", "EventSelection.run_selection :239-257"],
        "cases": summary,
        "input_checksums": input_checksums(cases),
        "python": sys.version.split()[0],
        "numpy": np.__version__,
        "pandas": pd.__version__,
        "scipy": scipy.__version__,
        "scikit-learn": sklearn.__version__,
        "pyarrow": pyarrow.__version__,
    }
    out["meta_json"] = np.array(json.dumps(meta, sort_keys=True))
    path = os.path.join(HERE, "events_ref_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
