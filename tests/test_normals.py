"""The device generator of ``PeakEnsemble`` without a device: the numpy mirror (normals_numpy.py) against ``numpy.random.Philox`` and against
``sqrt(2) erfinv(2u - 1)`` in 40-digit mpmath, its moments, ``gpras_amd/csrc/normals.h`` compiled for the host (tests/normals_host.cpp)
against the mirror, and the argument checks of ``PeakEnsemble.evaluate`` that come before any device work.

Bounds.  The mirror against mpmath: 8 eps relative -- the restatement with ``np.log`` measures 2.8 eps over bulk and tails, the rest is
room for another libm's ``log``.  The header against the mirror: bit for bit where ``|q| <= 0.425`` (only + - * / there, each rounded once on
both sides); 16 eps relative elsewhere: ``px_log`` and ``np.log`` are each below 1 ulp, so ``L = -log p`` differs by at most 2 ulp, ``r = sqrt(L)``
halves that, and ``dz/z`` per ``dL/L`` is below 1 over the tail (0.95 at ``p = 0.075``); 16 eps is 8 times that.  Moments of n draws: the mean
of n standard normals has standard deviation ``1 / sqrt(n)``, their variance ``sqrt(2 / n)``, a sample correlation ``1 / sqrt(n)``: five of
each."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import normals_numpy as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpras_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tests", "normals_host.cpp")
EPS = np.finfo(np.float64).eps
TOP = nn.MASK64


def _host_compiler():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for cand in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++"):
        if os.path.exists(cand):
            return cand
    raise RuntimeError("the clang++ that ships with hipcc was not found: normals.h cannot be compiled for the host")


def test_boundary_words_straddle_the_branches():
    w = nn.boundary_words()
    c = nn.is_central(w)
    r = nn.tail_radius(w)
    assert c.any() and (~c).any() and (r[~c] <= 5.0).any() and (r[~c] > 5.0).any()
    u = nn.uniform(w)
    assert u.min() == 2.0**-53 and u.max() == 1.0 - 2.0**-53
    for side in (u < 0.5, u > 0.5):  # either side of each boundary, in each half
        assert (c & side).any() and (~c & side & (r <= 5.0)).any() and (~c & side & (r > 5.0)).any()


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, stream, e, k, s", [(0, 0, 0, 0, 0), (1, 2, 3, 4, 5), (2**63 + 11, 2**64 - 1, 7, 2, 4095), (2**64 - 1, 2**63, 34, 63, 17),
                                                   (12345678901234567890, 9876543210987654321, 2**31, 49, 255)])
def test_mirror_words_against_numpy_philox(seed, stream, e, k, s):
    blocks = [1, 2, 3, 21, 255, 256]
    got = nn.philox4x64_10(np.array(blocks, dtype=np.uint64), s, k, e, seed, stream)
    for i, b in enumerate(blocks):
        # (numpy increments the counter before its first block; uint64 arrays: a list holding values >= 2^63 would be cast through float)
        bitgen = np.random.Philox(counter=np.array([b - 1, s, k, e], dtype=np.uint64), key=np.array([seed, stream], dtype=np.uint64))
        want = bitgen.random_raw(4)
        assert np.array_equal(got[i], want), (b, got[i], want)
        assert nn.philox4x64_10_int([b, s, k, e], [seed, stream]) == [int(v) for v in want]
    # the addressing: row t is word t & 3 of block t >> 2; mode, member and event are counter words 2, 1, 3
    w = nn.words(seed, stream, e, k + 1, s, 1, 23, 64)
    assert w.shape == (k + 1, 1, 64) and not w[:, :, 23:].any()
    for t in (0, 5, 22):
        assert int(w[k, 0, t]) == nn.philox4x64_10_int([t >> 2, s, k, e], [seed, stream])[t & 3]


def _reference_words():
    """>= 20 000 words: the bulk, both tails down to the last 50 values of ``w >> 12``, and words shifted down 20 and 40 bits."""
    bulk = nn.philox4x64_10(np.arange(1500, dtype=np.uint64), 3, 1, 4, 1, 5).ravel()  # 6000
    low = np.arange(50, dtype=np.uint64) << np.uint64(12)
    parts = [bulk, low, ~low, low | np.uint64(0xFFF), bulk[:2000] >> np.uint64(20), bulk[2000:4000] >> np.uint64(40), nn.boundary_words()]
    w = np.concatenate(parts)
    return np.concatenate([w, ~w])  # mirrored words: the other tail


@pytest.fixture(scope="module")
def mp_reference():
    import mpmath as mp

    w = _reference_words()
    assert w.size >= 20000
    u = nn.uniform(w)
    with mp.workdps(40):
        root2 = mp.sqrt(2)
        ref = [root2 * mp.erfinv(2 * mp.mpf(float(x)) - 1) for x in u]
        z = nn.normal(w)
        err = np.array([float(abs((mp.mpf(float(a)) - b) / b)) for a, b in zip(z, ref)])
    return w, z, err


def test_mirror_normals_against_mpmath(mp_reference):
    w, z, err = mp_reference
    c = nn.is_central(w)
    r = nn.tail_radius(w)
    assert c.sum() > 4000 and (~c & (r <= 5.0)).sum() > 1000 and (r > 5.0).sum() > 1000  # every branch is exercised
    for name, mask in (("central", c), ("tail", ~c & (r <= 5.0)), ("far tail", ~c & (r > 5.0))):
        print(f"{name}: {mask.sum()} words, max relative error {err[mask].max() / EPS:.2f} eps")
    assert err.max() <= 8 * EPS, err.max() / EPS
    assert np.all(np.isfinite(z)) and np.all(z != 0.0)


def test_antisymmetry_is_exact(mp_reference):
    w = mp_reference[0]
    assert np.array_equal(nn.uniform(~w), 1.0 - nn.uniform(w))
    assert np.array_equal(nn.normal(~w), -nn.normal(w))
    assert np.array_equal(nn.is_central(~w), nn.is_central(w))


def test_moments_and_independence_of_neighbouring_streams():
    n = 2**16
    seed, stream = 2024, 3
    bound = 5.0 / np.sqrt(n)
    # (K = 3 modes, members 6 and 7) of events 0 and 1: n rows each, taken as n / 4 blocks
    z = {e: nn.normal(nn.words(seed, stream, e, 3, 6, 2, n, n)) for e in (0, 1)}
    for e in z:
        assert z[e].shape == (3, 2, n)
        for kk in range(3):
            for s in range(2):
                x = z[e][kk, s]
                assert abs(x.mean()) <= bound, (e, kk, s, x.mean())
                assert abs(x.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n), (e, kk, s, x.var())

    def corr(a, b):
        return float(np.corrcoef(a, b)[0, 1])

    for kk in range(2):
        assert abs(corr(z[0][kk, 0], z[0][kk + 1, 0])) <= bound  # adjacent modes
    for kk in range(3):
        assert abs(corr(z[0][kk, 0], z[0][kk, 1])) <= bound  # adjacent members
        assert abs(corr(z[0][kk, 0], z[1][kk, 0])) <= bound  # adjacent events
    assert abs(corr(z[0][0, 0][:-1], z[0][0, 0][1:])) <= bound  # adjacent rows
    other = nn.normal(nn.words(seed, stream + 1, 0, 1, 6, 1, n, n))[0, 0]
    assert abs(corr(z[0][0, 0], other)) <= bound  # adjacent key streams


def test_mirror_blocks_and_antithetic_members():
    args = dict(seed=2**63 + 1, stream=2**64 - 2, event=7, K=3, rows=65, tp=128)
    full = nn.normals(member0=0, members=8, **args)
    assert not full[:, :, 65:].any() and np.all(full[:, :, :65] != 0.0)
    assert np.array_equal(nn.normals(member0=4, members=4, **args), full[:, 4:])
    assert np.array_equal(nn.normals(member0=0, members=8, **{**args, "rows": 5, "tp": 64})[:, :, :5], full[:, :, :5])
    anti = nn.normals(member0=0, members=8, pair_offset=4, **args)
    assert np.array_equal(anti[:, :4], full[:, :4]) and np.array_equal(anti[:, 4:], -full[:, :4])
    assert np.array_equal(nn.normals(member0=3, members=3, pair_offset=4, **args), anti[:, 3:6])


# ---- csrc/normals.h on the host -------------------------------------------------------------------------------------------------------------
def _build(directory, *flags):
    exe = directory / ("normals_host" + ("_san" if flags else ""))
    res = subprocess.run([_host_compiler(), "-std=c++17", "-O1", *flags, f"-I{CSRC}", PROGRAM, "-o", str(exe)], capture_output=True, text=True)
    return exe, res


def _run(exe, directory, addresses, words):
    addresses = np.ascontiguousarray(addresses, dtype=np.uint64).reshape(-1, 6)
    words = np.ascontiguousarray(words, dtype=np.uint64)
    with open(directory / "in.bin", "wb") as f:
        np.array([addresses.shape[0], words.size], dtype=np.uint64).tofile(f)
        addresses.tofile(f)
        words.tofile(f)
    out = subprocess.run([str(exe), str(directory / "in.bin"), str(directory / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    n = addresses.shape[0]
    raw = np.fromfile(directory / "out.bin", dtype=np.uint64)
    assert raw.size == 2 * n + words.size
    return raw[:n], raw[n : 2 * n].view(np.float64), raw[2 * n :].view(np.float64)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("normals_host")
    exe, res = _build(d)
    assert res.returncode == 0, res.stderr
    return exe, d


def _addresses():
    rng = np.random.default_rng(17)
    keys = [(0, 0), (1, 2), (2**63 + 11, 2**64 - 1), (2**64 - 1, 2**63)]
    rows = []
    for seed, stream in keys:
        for _ in range(600):
            rows.append([seed, stream, int(rng.integers(0, 40)), int(rng.integers(0, 64)), int(rng.integers(0, 4096)), int(rng.integers(0, 1024))])
    rows.append([5, 6, 2**62, 63, 4095, 1023])
    return np.array(rows, dtype=object).astype(np.uint64)


def test_header_on_the_host_against_the_mirror(host_program):
    exe, d = host_program
    addr = _addresses()
    bulk = nn.philox4x64_10(np.arange(1024, dtype=np.uint64), 9, 8, 7, 6, 5).ravel()
    chosen = np.concatenate([nn.boundary_words(), bulk, bulk >> np.uint64(40), ~(bulk >> np.uint64(40))])
    w_addr, z_addr, z_words = _run(exe, d, addr, chosen)
    want_w = np.array([nn.philox4x64_10_int([int(a[5]) >> 2, int(a[4]), int(a[3]), int(a[2])], [int(a[0]), int(a[1])])[int(a[5]) & 3] for a in addr],
                      dtype=object).astype(np.uint64)
    assert np.array_equal(w_addr, want_w)
    nn.assert_normals_match(z_addr, w_addr, "addresses")
    nn.assert_normals_match(z_words, chosen, "chosen words")
    far = ~nn.is_central(chosen) & (nn.tail_radius(chosen) > 5.0)
    assert far.sum() > 1000  # the far-tail branch, which no draw reaches
    assert z_words[np.flatnonzero(chosen == np.uint64(TOP))[0]] == -z_words[np.flatnonzero(chosen == 0)[0]]
    # antisymmetry of the header itself
    _, _, z_neg = _run(exe, d, addr[:0], ~chosen)
    assert np.array_equal(z_neg, -z_words)


def test_header_on_the_host_under_sanitizers(tmp_path):
    """The same stand-alone program with ``-fsanitize=undefined,address``: shifts, conversions and buffers of the generator and the program."""
    exe, res = _build(tmp_path, "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g")
    if res.returncode != 0 and ("asan" in res.stderr or "ubsan" in res.stderr or "sanitizer" in res.stderr):
        pytest.skip("this toolchain ships no sanitizer runtimes for the host")
    assert res.returncode == 0, res.stderr
    w = np.concatenate([nn.boundary_words(), nn.philox4x64_10(np.arange(64, dtype=np.uint64), 1, 2, 3, 4, 5).ravel()])
    w_addr, z_addr, z_words = _run(exe, tmp_path, _addresses()[::50], w)
    nn.assert_normals_match(z_words, w, "sanitized build")
    nn.assert_normals_match(z_addr, w_addr, "sanitized build, addresses")


# ---- evaluate's checks that come before any device work ------------------------------------------------------------------------------------------
def test_evaluate_argument_checks():
    from gpras_amd import ensemble as ge

    ens = object.__new__(ge.PeakEnsemble)  # (no model, no projector: the checks below read neither)
    x, ranges = np.zeros((4, 2)), [(0, 4)]
    assert ge.DEFAULT_RNG == "host" and ge.RNGS == ("host", "device")
    cases = {
        "rng": dict(rng="philox"),
        "normals": dict(rng="device", normals=[np.zeros((1, 2, 4))]),
        "seed": dict(rng="device", seed=-1),
        "seed ": dict(rng="device", seed=2**64),
        "seed  ": dict(rng="device", seed=1.5),
        "seed   ": dict(rng="host", seed=2**64),
        "stream": dict(rng="device", stream=-1),
        "stream ": dict(rng="device", stream=2**64),
        "stream  ": dict(rng="host", stream=2**64),
        "even": dict(rng="device", antithetic=True, members=3),
        'rng="device"': dict(rng="host", antithetic=True),
    }
    for word, kw in cases.items():
        members = kw.pop("members", 2)
        with pytest.raises(ValueError, match=word.strip()):
            ens.evaluate(x, ranges, members, **kw)
    for good in (0, 2**64 - 1, np.int64(5), np.uint64(2**64 - 1)):
        assert ge.check_seed(good, "seed") == int(good)
    assert "rng" in ge.EnsembleResult.__dataclass_fields__
