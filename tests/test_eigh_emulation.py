"""The device eigensolver's kernel source run on the host (tests/eig_emulation.cpp: ``gpras_amd/csrc/eig_jacobi.h`` compiled for
the CPU, one thread per work-item, a barrier per workgroup, the fp64 MFMA reproduced from its lane layout) against LAPACK and
the numpy restatement, under the bounds tests/test_gpu_eigh.py holds the GPU to.  It covers what a GPU-less checkout cannot
otherwise see: the kernels' indexing, barriers, bounds, schedule and rounding.  The cases are small (the emulation takes seconds per
64 x 64 pair problem): one block, one full pair, a ragged pair with an odd width, and a cluster of equal eigenvalues, the case in
which Jacobi without a threshold loses its quadratic convergence."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import eig_numpy as en

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "gpras_amd", "csrc", "eig_jacobi.h")
HARNESS = os.path.join(ROOT, "tests", "eig_emulation.cpp")
EPS = np.finfo(np.float64).eps
ORTHO_RATIO = 4.824  # tests/test_gpu_eigh.py
# token of the header -> its host stand-in
REWRITES = (
    ('#include "gprx_common.h"', ""),
    ("extern __shared__ double eig_smem[];", "double* eig_smem = g_dyn;"),
    ("__builtin_amdgcn_mfma_f64_16x16x4f64", "emu_mfma"),
)


def _host_compiler():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for cand in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++"):
        if os.path.exists(cand):
            return cand
    raise RuntimeError("the clang++ that ships with hipcc was not found: the kernel source cannot be compiled for the host")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("eig_emu")
    text = open(HEADER).read()
    for old, new in REWRITES:
        assert old in text, f"{old!r} is no longer in eig_jacobi.h: update the emulation"
        text = text.replace(old, new)
    (d / "eig_emu.h").write_text(text)
    exe = d / "emu"
    res = subprocess.run([_host_compiler(), "-std=c++20", "-O1", "-pthread", "-w", f"-I{d}", HARNESS, "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(g):
        n = g.shape[0]
        np.ascontiguousarray(g).tofile(d / "g.bin")
        out = subprocess.run([str(exe), str(n), str(d / "g.bin"), str(d / "o.bin")], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        status, sweeps, off_rel, padding = out.stdout.split()
        r = np.fromfile(d / "o.bin")
        return int(status), int(sweeps), float(off_rel), int(padding), r[:n], r[n:].reshape(n, n)

    return run


@pytest.mark.parametrize("kind, n", [("indefinite", 31), ("diagonal", 33), ("gram", 33), ("repeated", 40), ("indefinite", 64), ("near_diagonal", 36)])
def test_kernel_source_on_the_host_against_lapack(emu, kind, n):
    g = en.make_matrix(kind, n)
    status, sweeps, off_rel, padding, lam, v = emu(g)
    assert status == 0 and padding == 0
    want, u = np.linalg.eigh(g)
    assert np.max(np.abs(lam - want)) <= 1e-12 * np.max(np.abs(want))
    assert np.all(np.diff(lam) >= 0.0)
    res, norm = en.residual(g, lam, v)
    assert res <= 4.0 * n * EPS * norm, res / (n * EPS * norm)
    assert np.max(np.abs(v.T @ v - np.eye(n))) <= 4.0 * ORTHO_RATIO * np.sqrt(n) * EPS
    assert np.all(v[np.argmax(np.abs(v), axis=0), np.arange(n)] > 0.0)
    assert sweeps == en.eigh_jacobi(g)[2], "the kernels take another number of sweeps than the restatement"
    if kind in en.DISTINCT:
        norm2 = max(abs(want[0]), abs(want[-1]))
        for i in range(n):
            gap = min(abs(want[i] - want[j]) for j in (i - 1, i + 1) if 0 <= j < n)
            sign = 1.0 if v[:, i] @ u[:, i] >= 0.0 else -1.0
            assert np.max(np.abs(v[:, i] - sign * u[:, i])) <= 1e-12 * norm2 / gap


def test_emulated_run_reads_only_the_lower_triangle(emu):
    a, b = emu(en.make_matrix("indefinite", 33)), emu(en.make_matrix("upper_garbage", 33))
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])
