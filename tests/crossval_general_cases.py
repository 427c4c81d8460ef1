"""Cases of the held-out row ranges in the GENERAL sparse launch sequence ("held_general" = 1: M > 64, or M <= 64 with "sgpr_fused" = 0),
shared by tests/test_crossval_general.py (no GPU) and tests/test_gpu_crossval_general.py.

The inputs are crossval_cases.draw_inputs' (the recipe of test_gpu_sparse_variants) with seeds 200 + i.  Every case has eight cells, one
hold per cell; the holds sit where the masked Kuf build and the split-K products could go wrong: tiles are 64 columns, split-K chunks
256.  N = 600 pads to np = 640 (no split-K), N = 1100 to np = 1152 >= 1024 (split-K, the last chunk 128 columns).
"""

import numpy as np

import crossval_cases as cc

CELLS = 8
EMPTY_CELL = 7
SUFFIX_CELL = 5

# kernel, class, d, M, N, what it reaches
_TABLE = [
    ("RBF", "iso", 9, 50, 600, '"sgpr_fused" = 0: one block, sgpr_small_kernel'),
    ("Matern32", "iso", 10, 100, 600, "mp 128: sgpr_b_finish_kernel, no split-K"),
    ("Matern12", "expanded", 20, 65, 600, "expanded form, its own bound"),
    ("RBF", "ard", 14, 130, 1100, "mp 192: add-diag route; np 1152 >= 1024: split-K with a partial last chunk"),
    ("Matern52", "ard", 50, 300, 1100, "the top of the reference's sweep; d > KM_DC"),
    ("Exponential", "iso", 3, 129, 1100, "low d, mp 192"),
]


def holds_for(n):
    return [
        (70, 100),      # inside a tile
        (60, 70),       # across a tile edge
        (250, 262),     # across a split-K chunk edge
        (256, 512),     # whole tiles and a whole chunk: the early-return path of the build
        (0, 37),        # prefix
        (n - 37, n),    # suffix
        (3, n - 2),     # five rows kept
        (300, 300),     # empty
    ]


def _cases():
    out = []
    for i, (kernel, cls, d, m, n, _) in enumerate(_TABLE):
        ard, form = cc.class_flags(kernel, cls)
        out.append(dict(id=f"general-{kernel}-{cls}-d{d}-m{m}-n{n}", kernel=kernel, cls=cls, d=d, m=m, n=n, ard=ard, form=form, cells=CELLS,
                        seed=200 + i, unfused=m <= 64))
    return out


CASES = _cases()
RESIDENT_CASES = [CASES[1], CASES[3]]  # M = 100 (b-finish, no split-K) and M = 130 (add-diag, split-K)


def hold_arrays(case):
    holds = holds_for(case["n"])
    return (np.ascontiguousarray([h[0] for h in holds], dtype=np.int64), np.ascontiguousarray([h[1] for h in holds], dtype=np.int64))


def keep_rows(case, c):
    return cc.keep_rows(holds_for(case["n"])[c], case["n"])


def tolerances(case):
    """(loss, gradient block) bounds: the project's 1e-9 / 1e-7, the nonsmooth expanded class at its own."""
    return cc.NONSMOOTH_EXPANDED_TOL if case["form"] == 1 and case["kernel"] in cc.EXPANDED_ISO else (1e-9, 1e-7)


_REF = {}


def ref_cell(case, c, mask_bits=15):
    """The oracle's loss and gradient of cell c on its kept rows (mask 15: everything trainable; 8: Z only, no priors), computed once."""
    key = (case["id"], c, mask_bits)
    if key not in _REF:
        x, y, thetas, zs, units, *_ = cc.draw_inputs(case)
        keep = keep_rows(case, c)
        flags = tuple(bool(mask_bits & b) for b in (1, 2, 4, 8))
        _REF[key] = cc.ref_eval(case, x[keep], y[keep, units[c]], zs[c], thetas[c], flags)
    return _REF[key]
