"""Regenerates tests/golden/predict_bounds.json on the CPU: python tests/golden/make_predict_bounds.py

For every case of tests/test_gpu_predict_routes.py (tests/predict_reference.py: the single models S1-S7, the two extra hyperparameter
vectors of the state test, the batch cases B1-B6, per cell) the float64 restatements of the two prediction routes of csrc/gp_predict.h
run on exactly the data the test uses, and their distance from the longdouble prediction is recorded per route:

  mean  max |m - ref| / max |ref|
  var   max (|v - ref| / ref), the variance with the noise term

Each number is the maximum over the run on the longdouble kernel rounded to double and three seeded perturbations of it by what the
device's kernel build is allowed (r2 (1 + d1), |d1| <= 4u; g (1 + d2), |d2| <= 2u), never below u.  The GPU tests allow 8 x the
recorded ratio (another summation grouping, FMA contraction).  The numbers are measured, not chosen: they follow the condition of K.
Deterministic: a second run writes the same bytes.
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import predict_reference as pr  # noqa: E402


def render() -> str:
    return json.dumps(pr.compute_bounds(), indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    with open(pr.BOUNDS_PATH, "w") as fh:
        fh.write(render())
    print(pr.BOUNDS_PATH)
