"""tools/isa_diff.py: a tree compared with itself is identical kernel by kernel, and a build flag that changes the kernels
shows as a difference in the output and in the exit status.  CPU only (hipcc cross-compiles gfx950)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "isa_diff.py")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


def run(*args, trees=(ROOT, ROOT)):
    env = {k: v for k, v in os.environ.items() if k not in ("VBQ_ONLY_N10", "VBQ_EXTRA_HIPCC_FLAGS")}
    return subprocess.run([sys.executable, TOOL, *trees, *args], capture_output=True, text=True, env=env)


def test_same_tree_is_identical():
    r = run("vbq_amd/csrc/vbq_rans_window.hip")
    lines = [ln for ln in r.stdout.splitlines() if not ln.startswith("==")]
    assert r.returncode == 0, r.stdout + r.stderr
    assert lines and all(ln.endswith("lines)") and ": identical (" in ln for ln in lines), r.stdout


def test_a_flag_on_one_side_is_a_difference():
    # vbq_latents.hip instantiates its kernels per bit depth (VBQ_FOR_EACH_N): with the reference's depth alone on one side
    # the other depths exist on the other side only
    r = run("vbq_amd/csrc/vbq_latents.hip", "--b-flags=-DVBQ_ONLY_N10")
    assert r.returncode == 1, r.stdout + r.stderr
    assert "only in A" in r.stdout and ": identical (" in r.stdout, r.stdout


def test_a_moved_function_is_identical_pooled_and_only_in_per_file(tmp_path):
    # the same kernel text under two file names: pooled over each side's list it pairs up, file against file it cannot
    kernel = "#include <hip/hip_runtime.h>\nnamespace {\n__global__ void k_twice(float *x) { x[threadIdx.x] *= 2.0f; }\n}\n"
    trees = []
    for tree, name in (("a", "x.hip"), ("b", "y.hip")):
        csrc = tmp_path / tree / "vbq_amd" / "csrc"
        csrc.mkdir(parents=True)
        (tmp_path / tree / "include").mkdir()
        for n in {name, "x.hip"}:                     # the per-file form needs a file of that name on both sides
            (csrc / n).write_text(kernel if n == name else "#include <hip/hip_runtime.h>\n")
        trees.append(str(tmp_path / tree))
    r = run("--a-sources", "vbq_amd/csrc/x.hip", "--b-sources", "vbq_amd/csrc/y.hip", trees=trees)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "k_twice" in r.stdout and ": identical (" in r.stdout and "only in" not in r.stdout, r.stdout
    r = run("vbq_amd/csrc/x.hip", trees=trees)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "k_twice: only in A" in r.stdout, r.stdout
