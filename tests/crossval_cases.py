"""Cases of the held-out row ranges of the fused sparse evaluation (gprx_*_held) and of the event-fold cross-validation, shared by
tests/test_crossval.py (no GPU) and tests/test_gpu_crossval.py.

The inputs restate the recipe of test_gpu_sparse_variants.draw_inputs -- ``make_regression(..., config=31, unit=seed)``, Z on data rows plus
1e-3 noise, the same draws of variance, lengthscales and noise from ``default_rng(500 + seed)`` -- so that the preconditions of that
parity test (Kuf away from underflow, Kuu well conditioned) carry over; tests/test_crossval.py asserts them on every cell's kept rows.

N = 600 is three chunks of 256 columns, the last one partial (88 columns: one full tile and 24 columns of a second).  Every case has
eight cells, one hold per cell; the holds sit where the streamed passes could go wrong.
"""

import numpy as np

from gpras_amd.synth import make_regression
from oracle import kernels as okn
from oracle import sgpr as osg
from oracle import transforms as otr

N = 600
UNITS = 3
# (lo, hi) and where it lies: tiles are 64 columns, chunks 256
HOLDS = [
    (70, 100),   # inside a tile
    (60, 70),    # across a tile edge
    (250, 262),  # across a chunk edge
    (256, 512),  # a whole chunk
    (0, 37),     # prefix
    (563, 600),  # suffix
    (3, 598),    # five rows kept, fewer than M
    (300, 300),  # empty
]
SUFFIX_CELL = 5
EMPTY_CELL = 7
CELLS = len(HOLDS)
EXPANDED_ISO = ("Matern12", "Exponential")
NONSMOOTH_EXPANDED_TOL = (1e-7, 2e-6)  # test_gpu_sparse_variants.NONSMOOTH_EXPANDED_TOL: loss, gradient blocks

# kernel, class, d, M: NP = 6 (d = 8, 3), 8 (d = 14) and 0 (d = 20, 50); ISO = 1 (iso) and 0; both distance forms; d over more than one
# chunk of 16 dimensions
_TABLE = [("RBF", "iso", 8, 50), ("Matern32", "ard", 14, 64), ("Matern12", "expanded", 20, 17), ("Matern52", "ard", 50, 7),
          ("Exponential", "iso", 3, 1)]


def class_flags(kernel, cls):
    """(ard, form) of a class: iso-difference, ARD-difference, expanded (isotropic for Matern12 / Exponential, ARD otherwise)."""
    if cls == "iso":
        return False, 0
    if cls == "ard":
        return True, 0
    return kernel not in EXPANDED_ISO, 1


def _cases():
    out = []
    for i, (kernel, cls, d, m) in enumerate(_TABLE):
        ard, form = class_flags(kernel, cls)
        out.append(dict(id=f"{kernel}-{cls}-d{d}-m{m}", kernel=kernel, cls=cls, d=d, m=m, n=N, ard=ard, form=form, cells=CELLS, seed=100 + i))
    return out


CASES = _cases()
RESIDENT_CASES = CASES[:2]  # RBF iso and Matern32 ard: ISO = 1 and 0, NP = 6 and 8


def inducing_on_rows(x, m, rng):
    n, d = x.shape
    rows = rng.choice(n, size=min(m, n), replace=False)
    return x[rows] + 1e-3 * rng.standard_normal((rows.size, d))


_DRAWN = {}


def draw_inputs(case):
    """(x, y, thetas, zs, units, variance, ls, noise) of a case: drawn once, shared by every test, never written."""
    if case["id"] in _DRAWN:
        return _DRAWN[case["id"]]
    d, m, n, cells = case["d"], case["m"], case["n"], case["cells"]
    x, y, _ = make_regression(n, d, n_outputs=UNITS, n_test=0, config=31, unit=case["seed"])
    rng = np.random.default_rng(500 + case["seed"])
    nl = d if case["ard"] else 1
    variance = rng.uniform(0.5, 2.0, cells)
    ls = np.sqrt(d) * rng.uniform(0.6, 1.6, (cells, nl))
    noise = 10.0 ** rng.uniform(-2.0, -0.5, cells)
    thetas = np.ascontiguousarray([np.concatenate([np.atleast_1d(w) for w in otr.unconstrain(variance[c], ls[c], noise[c])]) for c in range(cells)])
    zs = np.ascontiguousarray(np.stack([inducing_on_rows(x, m, rng) for _ in range(cells)]))
    units = np.ascontiguousarray(rng.integers(0, UNITS, size=cells), dtype=np.int32)
    units[0], units[-1] = 0, UNITS - 1  # (mixed units in every batch)
    out = (np.ascontiguousarray(x), np.ascontiguousarray(y), thetas, zs, units, variance, ls, noise)
    for a in out:
        a.setflags(write=False)
    _DRAWN[case["id"]] = out
    return out


def keep_rows(hold, n=N):
    a, b = hold
    return np.r_[0:a, b:n]


def form_name(case):
    return "expanded" if case["form"] else "direct"


def ls_arg(case, ls):
    return ls if case["ard"] else float(ls[0])


def ref_eval(case, x, y, z, theta, mask=(True, True, True, True)):
    """The oracle's loss and gradient ``[d theta | d Z]`` of one cell on the rows it is given."""
    wl = theta[1:-1] if case["ard"] else float(theta[1])
    loss, g = osg.loss_and_grad(case["kernel"], x, y, z, float(theta[0]), wl, float(theta[-1]), mask, form=form_name(case))
    return loss, np.concatenate([[g["variance"]], np.atleast_1d(g["lengthscales"]), [g["noise"]], np.asarray(g["Z"]).ravel()])


_REF = {}


def ref_cell(case, c, mask_bits=15):
    """``ref_eval`` of cell c on its kept rows (mask 15: everything trainable; 8: Z only, no priors), computed once."""
    key = (case["id"], c, mask_bits)
    if key not in _REF:
        x, y, thetas, zs, units, *_ = draw_inputs(case)
        keep = keep_rows(HOLDS[c])
        flags = tuple(bool(mask_bits & b) for b in (1, 2, 4, 8))
        _REF[key] = ref_eval(case, x[keep], y[keep, units[c]], zs[c], thetas[c], flags)
    return _REF[key]


def preconditions(case, x, z, variance, ls):
    """The median of Kuf / variance and cond(Kuu + 1e-6 I) of one cell on the rows given."""
    kuf = okn.kmat(case["kernel"], z, x, variance, ls_arg(case, ls), form_name(case))
    kuu = okn.kmat(case["kernel"], z, z, variance, ls_arg(case, ls), form_name(case))
    return float(np.median(kuf / variance)), float(np.linalg.cond(kuu + 1e-6 * np.eye(z.shape[0])))


def blockwise_error(got, ref, nt):
    """Largest |got - ref| of the hyperparameter block and of the Z block, each relative to its block's largest |ref|."""
    return (float(np.max(np.abs(got[:nt] - ref[:nt])) / np.max(np.abs(ref[:nt]))),
            float(np.max(np.abs(got[nt:] - ref[nt:])) / np.max(np.abs(ref[nt:]))))
