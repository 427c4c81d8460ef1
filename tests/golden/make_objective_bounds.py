"""Regenerates tests/golden/objective_bounds.json on the CPU: python tests/golden/make_objective_bounds.py

For every case of tests/test_gpu_objective_routes.py (tests/objective_reference.py: the single models, the second hyperparameter vector
of the state test, the batch cases, per cell) the float64 restatement of the device's evaluation of the exact-model objective
(csrc/gp_exact.h, grad.h, solve.h) runs on exactly the data the test uses, once per way of forming alpha -- "substitution" (the
backward solve) and "from_inverse" (X^T beta from the explicit inverse) --, and its distance from the longdouble objective is recorded
under "<case>/c<cell>/<route>/m<mask>/<quantity>":

  loss  |loss - ref| / (1/2 y^T K^-1 y + sum |log L_ii| + n/2 log 2 pi + sum |log prior of the trained parameters|)
  g<k>  |g_k - ref_k| / S_k,  S_k = (1/2 sum_ij |W_ij| |dK_ij/du_k| + |d log prior/du_k|) |du_k/dw_k|   (trained components only)

Each number is the maximum over the run on the longdouble kernel rounded to double and three seeded perturbations of it by what the
device's kernel build is allowed, never below u = 2^-53.  The GPU tests allow 8 x the recorded ratio (another summation grouping, FMA
contraction).  The numbers are measured, not chosen: they follow the condition of K.  Deterministic: a second run writes the same bytes.
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import objective_reference as orf  # noqa: E402


def render() -> str:
    return json.dumps(orf.compute_bounds(), indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    with open(orf.BOUNDS_PATH, "w") as fh:
        fh.write(render())
    print(orf.BOUNDS_PATH)
