"""The host sweep builder of the threshold kernels (vbq_amd/csrc/vbq_sweep_host.h), checked against its definition by a
stand-alone C++ program built under the address and undefined-behaviour sanitizers (tests/host/sweep_table_check.cpp).
Nothing is loaded into Python: the program is a child process and its exit status is the verdict."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_table_builder_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "sweep_table_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "vbq_amd", "csrc"), os.path.join(ROOT, "tests", "host", "sweep_table_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "compiling the check failed:\n" + r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, f"sweep_table_check exited with {r.returncode}:\n" + r.stderr[-4000:]
    assert r.stderr == "", "the sanitizers or the check wrote:\n" + r.stderr[-4000:]
