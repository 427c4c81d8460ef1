"""Regenerates tests/golden/sparse_objective_bounds.json on the CPU: python tests/golden/make_sparse_objective_bounds.py

For every case of tests/test_gpu_sparse_objective_routes.py (tests/sparse_objective_reference.py: per cell and per mask) the float64
restatement of the device's evaluation of the sparse objective (csrc/sgpr_fused.h, gp_sparse.h, sgpr_asm.h) runs on exactly the data the
test uses -- a cell that holds rows out: on the rows it keeps --, and its distance from the longdouble objective is recorded under
"<case>/c<cell>/m<mask>/<quantity>":

  loss  |loss - ref| / natural scale of the loss
  g<k>  |g_k - ref_k| / natural scale of hyperparameter component k   (trained components only)
  gz    the maximum over the m d entries of Z of |gz_ik - ref_ik| / natural scale of that entry   (when Z trains)

with the natural scales of the module's docstring.  Each number is the maximum over the run on the longdouble kernel rounded to double
and three seeded perturbations of it by what the device's kernel build is allowed, never below u = 2^-53.  The GPU tests allow 8 x the
recorded ratio (another summation grouping, FMA contraction).  The numbers are measured, not chosen: they follow the condition of
Kuu + jitter I.  Deterministic: a second run writes the same bytes.
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import sparse_objective_reference as sr  # noqa: E402


def render() -> str:
    return json.dumps(sr.compute_bounds(), indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    with open(sr.BOUNDS_PATH, "w") as fh:
        fh.write(render())
    print(sr.BOUNDS_PATH)
