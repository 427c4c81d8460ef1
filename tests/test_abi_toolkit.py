"""The host toolkit of the C ABI units (``gpras_amd/csrc/abi_common.h``) without a GPU: tests/abi_toolkit_check.cpp, compiled for the
host with the address and undefined-behaviour sanitizers and run as a program of its own.  It holds the exception guard to its
status codes and texts, and the split-K plan to the arithmetic of the functions it replaced."""

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpras_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "abi_toolkit_check.cpp")


def _host_compiler():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for cand in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++"):
        if os.path.exists(cand):
            return cand, rocm
    raise RuntimeError("the clang++ that ships with hipcc was not found: the toolkit cannot be compiled for the host")


def test_guard_and_splitk_plan_on_the_host(tmp_path):
    cxx, rocm = _host_compiler()
    exe = tmp_path / "abi_toolkit_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           f"-I{os.path.join(rocm, 'include')}", f"-I{CSRC}", CHECK, "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
