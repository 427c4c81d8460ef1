"""numpy mirror of ``gpras_amd/csrc/normals.h``: Philox4x64-10 on split ``uint64`` arithmetic, the addressing of ``gprx_pca_normals_dev``
(include/gprx.h), the uniform ``((w >> 12) + 0.5) 2^-52`` and Wichura's AS 241 ``PPND16`` with numpy's rounded ``* + - /`` (numpy fuses
nothing) and ``np.log`` in the tails, where the header has ``px_log``: the central branch ``|q| <= 0.425`` is the header's bit for bit, the
tails agree with it to the few ulp the two logarithms differ by."""

import numpy as np

M0, M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
W0, W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B
MASK64 = (1 << 64) - 1
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)

# index 0 .. 7
A = (3.3871328727963666080e0, 1.3314166789178437745e2, 1.9715909503065514427e3, 1.3731693765509461125e4,
     4.5921953931549871457e4, 6.7265770927008700853e4, 3.3430575583588128105e4, 2.5090809287301226727e3)
B = (1.0, 4.2313330701600911252e1, 6.8718700749205790830e2, 5.3941960214247511077e3,
     2.1213794301586595867e4, 3.9307895800092710610e4, 2.8729085735721942674e4, 5.2264952788528545610e3)
C = (1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
     1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4)
D = (1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1,
     1.48103976427480074590e-1, 1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9)
E = (6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0, 2.96560571828504891230e-1,
     2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7)
F = (1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2,
     7.86869131145613259100e-4, 1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15)


def _u64(x):
    """``x`` (Python integers below 2^64, or an integer array) as a ``uint64`` array, never through float."""
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64)
    return np.array(x, dtype=object).astype(np.uint64)


def mulhilo(a: int, b):
    """``(hi, lo)`` of the 128-bit product of the constant ``a`` and the ``uint64`` array ``b``, from 32-bit halves."""
    a_lo, a_hi = np.uint64(a & 0xFFFFFFFF), np.uint64(a >> 32)
    b_lo, b_hi = b & _M32, b >> _S32
    ll, lh, hl, hh = a_lo * b_lo, a_lo * b_hi, a_hi * b_lo, a_hi * b_hi
    mid = (ll >> _S32) + (lh & _M32) + (hl & _M32)
    lo = (ll & _M32) | ((mid & _M32) << _S32)
    hi = hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32)
    return hi, lo


def philox4x64_10(c0, c1, c2, c3, k0: int, k1: int):
    """The four words ``(..., 4)`` of every counter ``(c0, c1, c2, c3)`` (broadcast against each other) under the key ``(k0, k1)``."""
    c0, c1, c2, c3 = (np.atleast_1d(a).copy() for a in np.broadcast_arrays(_u64(c0), _u64(c1), _u64(c2), _u64(c3)))
    k0, k1 = int(k0) & MASK64, int(k1) & MASK64
    for _ in range(10):
        hi0, lo0 = mulhilo(M0, c0)
        hi1, lo1 = mulhilo(M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK64, (k1 + W1) & MASK64
    return np.stack([c0, c1, c2, c3], axis=-1)


def philox4x64_10_int(c, k):
    """The same block on Python integers: ``c`` four counter words, ``k`` two key words."""
    c0, c1, c2, c3 = (int(v) for v in c)
    k0, k1 = (int(v) for v in k)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 64) ^ c1 ^ k0, p1 & MASK64, (p0 >> 64) ^ c3 ^ k1, p0 & MASK64
        k0, k1 = (k0 + W0) & MASK64, (k1 + W1) & MASK64
    return [c0, c1, c2, c3]


def uniform(w):
    return ((_u64(w) >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0**-52


def _horner(coef, x):
    p = np.full_like(x, coef[7])
    for c in coef[6::-1]:
        p = p * x + c
    return p


def ppnd16(u):
    """``(z, central)``: the normal quantile of ``u`` by AS 241 and the mask of the branch ``|q| <= 0.425``."""
    u = np.asarray(u, dtype=np.float64)
    q = u - 0.5
    central = np.abs(q) <= 0.425
    r = 0.180625 - q * q
    zc = q * _horner(A, r) / _horner(B, r)
    rt = np.sqrt(-np.log(np.where(q < 0.0, u, 1.0 - u)))
    x1, x2 = rt - 1.6, rt - 5.0
    zt = np.where(rt <= 5.0, _horner(C, x1) / _horner(D, x1), _horner(E, x2) / _horner(F, x2))
    zt = np.where(q < 0.0, -zt, zt)
    return np.where(central, zc, zt), central


def tail_radius(w):
    """``r = sqrt(-log min(u, 1 - u))`` of words (the branch beyond ``|q| = 0.425`` splits at ``r = 5``)."""
    u = uniform(w)
    return np.sqrt(-np.log(np.minimum(u, 1.0 - u)))


def normal(w):
    return ppnd16(uniform(w))[0]


def is_central(w):
    return ppnd16(uniform(w))[1]


def boundary_words():
    """``w = 0``, ``w = 2^64 - 1`` and the words either side of ``|q| = 0.425`` (both signs) and of ``r = 5`` (both tails)."""
    out = [0, MASK64, 1 << 12, MASK64 - (1 << 12), 1 << 63, (1 << 63) - 1]
    hi = int(0.925 * 2.0**52)  # u = 0.925: q = +0.425
    lo = int(0.075 * 2.0**52)  # u = 0.075: q = -0.425
    far = int(np.exp(-25.0) * 2.0**52)  # min(u, 1 - u) = e^-25: r = 5
    for m in (hi, lo, far):
        for d in range(-3, 4):
            out += [(m + d) << 12, ((m + d) << 12) | 0xFFF]
    for d in range(-3, 4):
        out.append(MASK64 - ((far + d) << 12))
    return _u64(out)


def assert_normals_match(got, w, label=""):
    """What any build of normals.h owes the mirror on the words ``w``: the central branch bit for bit, the tails within 16 eps relative
    (``px_log`` against ``np.log``: test_normals.py has the argument), the signs equal.  Returns the masks ``(central, far tail)``."""
    eps = np.finfo(np.float64).eps
    got, w = np.asarray(got).ravel(), np.asarray(w).ravel()
    want, central = ppnd16(uniform(w))
    assert np.array_equal(got[central], want[central]), f"{label}: the central branch differs"
    rel = np.abs(got[~central] - want[~central]) / np.abs(want[~central])
    if rel.size:
        print(f"{label}: {central.sum()} central words bit for bit; {rel.size} tail words, max {rel.max() / eps:.2f} eps")
        assert rel.max() <= 16 * eps, (label, rel.max() / eps)
    assert np.array_equal(np.signbit(got), np.signbit(want)), label
    return central, ~central & (tail_radius(w) > 5.0)


def words(seed, stream, event, K, member0, members, rows, tp, pair_offset=0):
    """``(K, members, tp) uint64``: the word of ``(seed, stream, event, mode, member0 + slot, t)`` for ``t < rows``, zero beyond.  With
    ``pair_offset = h > 0`` a member ``s >= h`` reads the counter of member ``s - h``."""
    s = np.arange(member0, member0 + members, dtype=np.int64)
    if pair_offset:
        s = np.where(s >= pair_offset, s - pair_offset, s)
    blocks = (tp + 3) // 4
    w = philox4x64_10(np.arange(blocks, dtype=np.uint64)[None, None, :], s.astype(np.uint64)[None, :, None],
                      np.arange(K, dtype=np.uint64)[:, None, None], _u64(int(event)), seed, stream)
    w = w.reshape(K, members, 4 * blocks)[:, :, :tp].copy()
    w[:, :, rows:] = 0
    return w


def normals(seed, stream, event, K, member0, members, rows, tp, pair_offset=0):
    """``(K, members, tp) float64``: the draws ``gprx_pca_normals_dev`` writes, exact zeros for ``t >= rows``; with ``pair_offset = h > 0``
    the members ``s >= h`` are the negation of the members ``s - h``."""
    z = normal(words(seed, stream, event, K, member0, members, rows, tp, pair_offset))
    z[:, :, rows:] = 0.0
    if pair_offset:
        s = np.arange(member0, member0 + members)
        z[:, s >= pair_offset, :rows] = -z[:, s >= pair_offset, :rows]
    return z


def central_mask(seed, stream, event, K, member0, members, rows, tp, pair_offset=0):
    """The branch of every draw of ``normals(...)`` (False in the padding)."""
    m = is_central(words(seed, stream, event, K, member0, members, rows, tp, pair_offset))
    m[:, :, rows:] = False
    return m
