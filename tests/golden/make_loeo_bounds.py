"""Regenerates tests/golden/loeo_bounds.json on the CPU: python tests/golden/make_loeo_bounds.py

For every case of tests/test_gpu_loeo.py (tests/loeo_reference.py, per cell) the float64 restatements of the two leave-one-event-out
routes -- the downdate of csrc/sf_loeo.h and the refactor route of gpras_amd/loeo.py -- run on exactly the data the test uses, and
their distance from the longdouble definition (the model refitted in longdouble on the data without each event) is recorded per route:

  mean  max |m - ref| / max |ref|            over the rows of the events
  var   max (|v - ref| / ref), the variance with the noise term

Each number is the maximum over the run on the longdouble kernel rounded to double and three seeded perturbations of it by what the
device's kernel build is allowed, never below u.  The GPU tests allow 8 x the recorded ratio (another summation grouping, FMA
contraction).  The numbers are measured, not chosen.  Deterministic: a second run writes the same bytes.
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import loeo_reference as lr  # noqa: E402


def render() -> str:
    return json.dumps(lr.compute_bounds(), indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    with open(lr.BOUNDS_PATH, "w") as fh:
        fh.write(render())
    print(lr.BOUNDS_PATH)
