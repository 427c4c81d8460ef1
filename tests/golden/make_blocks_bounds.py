"""Regenerates tests/golden/blocks_bounds.json on the CPU: python tests/golden/make_blocks_bounds.py

For every solve, inverse and reduction case of tests/test_gpu_solve_blocks.py a float64 numpy restatement of the block algorithm of
csrc/solve.h (tests/blocks_reference.py, emu_*: explicit inverses of the 64 x 64 diagonal blocks plus products) runs on exactly the
matrices the test uses, and its worst componentwise ratio against the longdouble reference is recorded:

  factor      |A - L L^T|   / (u |L| |L|^T)      (tests/test_gpu_potrf_batched.py; emu_potrf restates csrc/potrf.h, and its solved
                                                   rows and inverse blocks are taken against its own factor)
  solves      |op(L) X - B| / (n u (|op(L)| |X| + |B|))
  inverse     |X L - I|     / (n u (|X| |L| + I))
  reductions  |got - ref|   / (sum of the magnitudes of the terms), not below u = 2^-53

The GPU tests allow 8 x the recorded ratio (another summation order, FMA contraction).  The constants are measured, not chosen: with
explicit block inverses they depend on the condition of the diagonal blocks.  Deterministic: a second run writes the same bytes.
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import blocks_reference as br  # noqa: E402


def render() -> str:
    return json.dumps(br.compute_bounds(), indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    with open(br.BOUNDS_PATH, "w") as fh:
        fh.write(render())
    print(br.BOUNDS_PATH)
