"""Regenerates tests/golden/loeo_blocked_bounds.json on the CPU: python tests/golden/make_loeo_blocked_bounds.py

For every case of tests/test_gpu_loeo_blocked.py (tests/loeo_blocked_reference.py, per cell) the float64 restatements of the blocked
leave-one-event-out route (csrc/gp_loeo_blocked.h: the explicit inverse of chol(H)) and of the refactor route of gpras_amd/loeo.py --
for case B50 also of the one-workgroup downdate -- run on exactly the data the test uses, and their distance from the longdouble
definition (the model refitted in longdouble on the data without each event) is recorded per route:

  mean  max |m - ref| / max |ref|            over the rows of the events
  var   max (|v - ref| / ref), the variance with the noise term

Each number is the maximum over the run on the longdouble kernel rounded to double and three seeded perturbations of it by what the
device's kernel build is allowed, never below u: the rule of make_loeo_bounds.py.  The GPU tests allow 8 x the recorded ratio.  The
numbers are measured, not chosen.  Deterministic: a second run writes the same bytes.
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import loeo_blocked_reference as br  # noqa: E402


def render() -> str:
    return json.dumps(br.compute_bounds(), indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    with open(br.BOUNDS_PATH, "w") as fh:
        fh.write(render())
    print(br.BOUNDS_PATH)
