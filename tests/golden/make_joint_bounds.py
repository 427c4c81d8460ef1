"""Regenerates tests/golden/joint_bounds.json on the CPU: python tests/golden/make_joint_bounds.py

For every case of tests/test_gpu_joint_routes.py (tests/joint_reference.py, per cell and include_noise) the float64 restatement of
csrc/gp_joint.h's predict_joint_batch runs on exactly the data the test uses, and its distance from the longdouble definition of the
joint prediction is recorded in the three measures of joint_reference.py:

  mean    max |m - ref| / max |ref|
  cov     max_ij |Lc Lc^T - C|_ij / S_ij, S the natural scale of the entry
  factor  max_{i >= j} |Lc_ij - Lref_ij| / sqrt(C_ii)

Each number is the maximum over the run on the longdouble kernel rounded to double and three seeded perturbations of it by what the
device's kernel build is allowed, never below u.  The GPU tests allow 8 x the recorded ratio (another summation grouping, FMA
contraction).  The numbers are measured, not chosen.  Deterministic: a second run writes the same bytes.

One cap is asserted and printed: no new bound is looser than the one it replaces, the absolute 1e-8 (variance + noise) on Lc Lc^T of
tests/test_gpu_ensemble.py -- 8 x recorded cov ratio x S_ij <= 1e-8 (variance + noise) for every element of every case.  A case that
breaks it gets other hyperparameters; the cap stays.
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import joint_reference as jr  # noqa: E402


def compute(verbose=False):
    """(bounds, the largest share of the cap any element uses and where)."""
    out, worst = {}, (0.0, None)
    for cid, c in jr.CASES.items():
        ratios = jr.case_ratios(cid)
        for cell in range(c.cells):
            for nz in (0, 1):
                k = jr.key(cid, cell, nz, "cov")
                used = jr.cap_used(cid, cell, nz, ratios[k])
                assert used <= 1.0, f"{k}: 8 x {ratios[k]:.3e} x max S is {used:.2f} x the bound it replaces, 1e-8 (variance + noise)"
                worst = max(worst, (used, k))
        out.update(ratios)
        jr._parts.cache_clear()
        jr.joint_ld.cache_clear()
        if verbose:
            print(f"{cid}: cov {max(v for k, v in ratios.items() if k.endswith('/cov')):.2e}, factor "
                  f"{max(v for k, v in ratios.items() if k.endswith('/factor')):.2e}, mean {max(v for k, v in ratios.items() if k.endswith('/mean')):.2e}",
                  flush=True)
    return out, worst


def render(bounds=None) -> str:
    return json.dumps(compute()[0] if bounds is None else bounds, indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    bounds, (used, where) = compute(verbose=True)
    with open(jr.BOUNDS_PATH, "w") as fh:
        fh.write(render(bounds))
    print(f"cap: the loosest new bound is {used:.3e} of 1e-8 (variance + noise), at {where}")
    print(jr.BOUNDS_PATH)
