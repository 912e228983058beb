"""The budget sweep (include/vbq_budget.h, vbq_amd/budget) without a GPU: the third library's ABI, its refusals, the static
stream and refusal-order rules of the first library applied to its sources, the Python layers' host logic, and the rule
"smallest total_bits within a distortion" on curves of tests/budget_reference.py.

The guard tables of the first library (footprint.COVERED, stream_order.BY_SOURCE) name the functions of include/vbq.h and the
files of vbq_amd/csrc, tests/test_scores_host.py holds the second library; libvbq_budget.so adds to none of them and this
module is its guard.  The names are read FROM the header: a later entry point needs no edit here."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import budget_reference as BR  # noqa: E402
from test_abi import declared_functions  # noqa: E402
from test_refusal_order_host import analyse, late_refusals  # noqa: E402
from test_stream_order_host import (async_violations, call_args, forbidden_found, launch_violations,  # noqa: E402
                                    literal_stream_violations, python_site_violations, stream_positions, stream_variable_violations,
                                    strip_c)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbq_budget.h")
BUDGET = os.path.join(ROOT, "vbq_amd", "budget")
CSRC = os.path.join(ROOT, "vbq_amd", "csrc")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
WHO = "vbqb_budget_sweep_f64"


def _read(path):
    with open(path) as f:
        return f.read()


@pytest.fixture(scope="module")
def budget_lib():
    from vbq_amd import build
    return build.build_budget()


@pytest.fixture(scope="module")
def hb(budget_lib):
    from vbq_amd import _lib_budget
    return _lib_budget.lib()


# ------------------------------------------------------------------------------------------------------------------ the ABI
def _header_functions():
    """{name: [argument texts]} of include/vbq_budget.h."""
    s = strip_c(_read(HEADER))
    return {m.group(1): call_args(s, m.end() - 1) for m in re.finditer(r"\b(vbqb_[a-z0-9_]+)\s*\(", s)}


def test_header_carries_its_own_version_and_error_and_builds_on_vbq_h():
    names = set(_header_functions())
    assert {"vbqb_abi_version", "vbqb_last_error"} < names and all(n.startswith("vbqb_") for n in names)
    assert any(n.endswith("_f64") for n in names) and any(n.endswith("_workspace_bytes") for n in names)
    text = _read(HEADER)
    assert '#include "vbq.h"' in text and "#define VBQB_ABI_VERSION 1" in text
    assert not re.search(r"\bvbqx?_[a-z0-9_]+\s*\(", strip_c(text))          # it declares nothing of the other two libraries


def test_library_exports_exactly_the_header(budget_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", budget_lib], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r"\b[A-Za-z] (vbqb_[A-Za-z0-9_]+)", out)) == sorted(_header_functions())
    assert not re.search(r"\bvbqx?_", out) and "_ZN" not in out and "_Z" not in out, out


def test_the_first_two_libraries_are_unchanged_in_their_exports():
    from vbq_amd import build
    out = subprocess.run(["nm", "-D", "--defined-only", build.build_hip()], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (vbq[a-z0-9]*_[a-z0-9_]+)", out)) == set(declared_functions())
    assert not any(n.startswith("vbqb") for n in declared_functions())
    ext_header = strip_c(_read(os.path.join(ROOT, "include", "vbq_ext.h")))
    out = subprocess.run(["nm", "-D", "--defined-only", build.build_ext()], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r"\b[A-Za-z] (vbq[a-z0-9]*_[A-Za-z0-9_]+)", out)) == sorted(set(re.findall(r"\b(vbqx_[a-z0-9_]+)\s*\(", ext_header)))
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(BUDGET, "*"))) == ["vbqb_api.hip", "vbqb_sweep.hip"]


def test_ctypes_binding_mirrors_the_header(hb):
    from vbq_amd import _lib_budget
    declared = _header_functions()
    assert sorted(_lib_budget.SIGNATURES) == sorted(declared)

    def ctype(arg):
        arg = " ".join(arg.split())
        if "*" in arg:
            return C.c_void_p
        return {"int64_t": C.c_int64, "int32_t": C.c_int32, "size_t": C.c_size_t}[arg.split(" ")[0]]
    text = strip_c(_read(HEADER))
    for name, args in declared.items():
        res, argtypes = _lib_budget.SIGNATURES[name]
        assert argtypes == ([] if args == ["void"] else [ctype(a) for a in args]), name
        returns = re.search(r"([A-Za-z_][A-Za-z0-9_ ]*?\**)\s*" + name + r"\s*\(", text).group(1).split()
        assert res == (C.c_char_p if "char" in returns else C.c_size_t if "size_t" in returns else C.c_int), name
    assert hb.vbqb_abi_version() == 1 == _lib_budget.ABI_VERSION


def test_missing_library_fails_loudly(monkeypatch, tmp_path, budget_lib):
    from vbq_amd import _lib, _lib_budget
    monkeypatch.setattr(_lib_budget, "_LIB", None)
    monkeypatch.setenv("VBQ_BUDGET_LIBRARY", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.VBQError, match="not built"):
        _lib_budget.lib()
    monkeypatch.delenv("VBQ_BUDGET_LIBRARY")
    monkeypatch.setattr(_lib_budget, "_LIB", None)
    assert _lib_budget.lib() is not None


def test_a_current_library_without_an_object_cache_needs_no_compiler(budget_lib, monkeypatch, tmp_path):
    """The tree as it arrives where objects are not shipped: library and flags tag, no vbq_amd/lib/obj/budget."""
    import shutil
    from vbq_amd import build
    lib = tmp_path / "lib"
    lib.mkdir()
    for name in ("libvbq_budget.so", "vbq_budget.flags.txt"):
        shutil.copy2(os.path.join(build.LIBDIR, name), lib / name)
    monkeypatch.setattr(build, "LIBDIR", str(lib))
    monkeypatch.setattr(build, "BUDGET_LIB", str(lib / "libvbq_budget.so"))
    monkeypatch.setattr(shutil, "which", lambda name: pytest.fail("looked for a compiler"))
    monkeypatch.setattr(build.subprocess, "run", lambda *a, **k: pytest.fail("started a process"))
    assert build.build_budget() == str(lib / "libvbq_budget.so") and not (lib / "obj").exists()
    assert "vbq_amd/lib/vbq_budget.flags.txt" in _read(os.path.join(ROOT, ".gitignore")).split()


# ------------------------------------------------------------------------------------------------------------------ refusals
def _call(hb, **kw):
    """vbqb_budget_sweep_f64 with the address 1 for every non-null pointer: nothing may read through them."""
    a = dict(fhat=1, rows=5, K=4, N=3, budgets=[2, 7], bits=1, obj=1, curve=None, curve_len=0, status=None, ws=None, wsb=0)
    a.update(kw)
    budgets = a["budgets"]
    arr = None if budgets is None else (C.c_int32 * len(budgets))(*budgets)
    S = a.get("S", 0 if budgets is None else len(budgets))
    return hb.vbqb_budget_sweep_f64(a["fhat"], a["rows"], a["K"], a["N"], arr, S, a["bits"], a["obj"], a["curve"], a["curve_len"],
                                    a["status"], a["ws"], a["wsb"], None)


def test_the_c_call_refuses_before_any_device_work(hb):
    """On a host without a GPU: every refusal returns before anything could be launched, and names itself and the value."""
    def refused(rc, code, *texts):
        msg = hb.vbqb_last_error().decode()
        assert rc == code and WHO in msg and all(t in msg for t in texts), (rc, msg)

    refused(_call(hb, rows=-1), INVALID, "n_rows=-1")
    refused(_call(hb, K=0), INVALID, "K=0")
    for N in (-1, 53):
        refused(_call(hb, N=N, budgets=[0]), INVALID, f"N={N}")
    refused(_call(hb, budgets=[0] * 65), INVALID, "S=65")
    refused(_call(hb, S=-1), INVALID, "S=-1")
    refused(_call(hb, budgets=None, S=2), INVALID, "null pointer", "budgets")
    for bad, at in (([-1, 3], 0), ([3, 13], 1), ([0, 5, 1 << 30], 2)):
        refused(_call(hb, budgets=bad), INVALID, f"budgets[{at}] = {bad[at]}", "[0, K*N = 12]")
    refused(_call(hb, budgets=[3, 3]), INVALID, "budgets[1] = 3", "budgets[0] = 3", "strictly ascending")
    refused(_call(hb, budgets=[3, 5, 4]), INVALID, "budgets[2] = 4", "budgets[1] = 5", "strictly ascending")
    for n in (-1, 14):
        refused(_call(hb, curve=1, curve_len=n), INVALID, f"curve_len {n}", "[0, K*N + 1 = 13]")
    for name in ("fhat", "bits", "obj"):
        refused(_call(hb, **{name: None}), INVALID, "null pointer")
    refused(_call(hb, curve=None, curve_len=5), INVALID, "curve_len 5", "d_curve null")
    refused(_call(hb, curve=1, curve_len=0), INVALID, "curve_len 0", "d_curve given")
    # two value rows that do not fit the LDS: a curve over 20001 budgets
    refused(_call(hb, K=2000, N=10, budgets=[], curve=1, curve_len=20001), UNSUPPORTED, "width = 20001")
    # the back-pointers of K = 300 at width 601 do not fit the LDS: a workspace is needed, and one slice is 180304 bytes
    per_row = (300 * 601 + 15) // 16 * 16
    refused(_call(hb, K=300, N=4, budgets=[600]), WORKSPACE, "workspace of 0 bytes", str(per_row))
    refused(_call(hb, K=300, N=4, budgets=[600], ws=1, wsb=per_row - 1), WORKSPACE, f"workspace of {per_row - 1} bytes")
    refused(_call(hb, K=300, N=4, budgets=[600], ws=None, wsb=per_row), WORKSPACE, "workspace")
    assert hb.vbqb_budget_sweep_workspace_bytes(5, 300, 4, 601) == 5 * per_row
    assert hb.vbqb_budget_sweep_workspace_bytes(5, 100, 10, 1001) == 0                   # 100 100 bytes: in the LDS
    for bad in (dict(n_rows=0), dict(K=0), dict(N=53), dict(width=0), dict(width=1202)):
        a = dict(n_rows=5, K=300, N=4, width=601)
        a.update(bad)
        assert hb.vbqb_budget_sweep_workspace_bytes(a["n_rows"], a["K"], a["N"], a["width"]) == 0


def test_no_rows_or_nothing_asked_is_no_work(hb):
    assert _call(hb, rows=0) == 0
    assert _call(hb, rows=0, fhat=None, bits=None, obj=None) == 0     # nothing is read or written: the pointers may be null
    assert _call(hb, budgets=[], fhat=None, bits=None, obj=None) == 0
    assert _call(hb, budgets=None, S=0) == 0
    assert _call(hb, rows=0, budgets=[3, 3]) == INVALID               # but sizes and budgets are still checked
    assert _call(hb, rows=0, K=0) == INVALID


# ------------------------------------------------------------------------------------------------------------------ static rules
def _budget_sources():
    files = {os.path.basename(p): _read(p) for p in sorted(glob.glob(os.path.join(BUDGET, "*")))}
    assert sorted(files) == ["vbqb_api.hip", "vbqb_sweep.hip"], sorted(files)
    return files


def test_every_launch_of_the_third_library_names_the_callers_stream():
    files = _budget_sources()
    launches = 0
    for name, text in files.items():
        n, bad = launch_violations(text)
        launches += n
        assert not bad and n == len(re.findall(r"\bhipLaunchKernelGGL\b", strip_c(text))), (name, bad)
        assert async_violations(text)[1] == [], name
        assert stream_variable_violations(text)[1] == [], name
        assert forbidden_found(text) == [] and literal_stream_violations(text) == [], name
    assert launches >= 1 and stream_variable_violations(files["vbqb_sweep.hip"])[0] >= 2
    planted = files["vbqb_sweep.hip"].replace("p.lds_bytes, st, fhat,", "p.lds_bytes, 0, fhat,")
    assert planted != files["vbqb_sweep.hip"] and launch_violations(planted)[1] and literal_stream_violations(planted)
    planted = files["vbqb_sweep.hip"].replace("    SweepBudgets bud = {};", "    SweepBudgets bud = {};\n    hipDeviceSynchronize();")
    assert planted != files["vbqb_sweep.hip"] and forbidden_found(planted) == ["hipDeviceSynchronize"]


def test_no_refusal_of_the_third_library_stands_after_an_enqueue():
    """The walk of tests/test_refusal_order_host.py over vbq_amd/budget and the header it shares with vbq_amd/csrc."""
    files = _budget_sources()
    files["vbq_common.h"] = _read(os.path.join(CSRC, "vbq_common.h"))
    bodies, enq, ref, _ = analyse(files)
    entries = {n for n in _header_functions() if n.endswith("_f64")}
    assert entries and entries <= set(bodies) and entries <= enq and entries <= ref
    assert "sweep_launch" in enq and not {"sweep_check", "sweep_plan"} & enq and "sweep_check" in ref
    assert not {n for n in _header_functions() if not n.endswith("_f64")} & (enq | ref)
    assert late_refusals(files) == []
    text = files["vbqb_sweep.hip"]
    late = text.replace("    const int64_t slices = ", "    hipLaunchKernelGGL(k_late, dim3(1), dim3(64), 0, st, d_status);\n"
                        "    VBQ_REQUIRE(d_status, VBQ_ERR_INVALID_ARGUMENT, \"late\");\n    const int64_t slices = ")
    assert late != text
    assert ("vbqb_sweep.hip", WHO, "VBQ_REQUIRE") in late_refusals({**files, "vbqb_sweep.hip": late})


def test_every_python_call_site_of_the_third_library_passes_the_tensors_stream():
    """The rule of tests/test_stream_order_host.py reads names that start with `vbq_`: the third library's are spelled
    `vbq_b_...` for it, in the header and in the Python text alike."""
    spell = lambda text: text.replace("vbqb_", "vbq_b_")
    pos = stream_positions(spell(_read(HEADER)))
    assert set(pos) == {spell(n) for n in _header_functions() if n.endswith("_f64")} and pos[spell(WHO)] == 13
    total, called = 0, set()
    for path in sorted(glob.glob(os.path.join(ROOT, "vbq_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py"))):
        text = spell(_read(path))
        seen, bad = python_site_violations(text, pos, os.path.basename(path))
        total += seen
        called |= {m for m in re.findall(r"\.(vbq_b_[a-z0-9_]+)\b", text) if m in pos}
        assert not bad, (path, bad)
    assert total >= 1 and called == set(pos)
    ops_text = spell(_read(os.path.join(ROOT, "vbq_amd", "ops.py")))
    planted = ops_text.replace("_ptr(workspace), wsb, _stream(fhat)),\n                      \"vbq_b_budget_sweep_f64\")",
                               "_ptr(workspace), wsb, None),\n                      \"vbq_b_budget_sweep_f64\")")
    assert planted != ops_text and python_site_violations(planted, pos, "ops.py")[1]


# ------------------------------------------------------------------------------------------------------------------ the Python layers
def test_python_layers_refuse_without_a_device(monkeypatch):
    import vbq_amd
    from vbq_amd import embeddings as E, ops, rows_budget
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)    # a host without a device, wherever this runs
    mu, sg = np.zeros((3, 2), np.float32), np.ones((3, 2), np.float32)
    tab = vbq_amd.gaussian_table(np.array([1.0]), N=4)[0]
    with pytest.raises(vbq_amd.VBQError, match="quantize_rows_to_budgets has no CPU implementation"):
        vbq_amd.quantize_rows_to_budgets(mu, sg, [1, 2], table=tab, N=4)
    with pytest.raises(vbq_amd.VBQError, match="budget_curve has no CPU implementation"):
        rows_budget.budget_curve(mu, sg, table=tab, N=4)
    for call in (lambda: E.compress_to_records_sweep(mu, sg, [1, 2], tab, 4), lambda: E.records_distortion_curve(mu, sg, tab, 4),
                 lambda: E.compress_to_records_quality(mu, sg, tab, 0.5, 4),
                 lambda: E.test_total_bits(mu, sg, [1, 2], tab, np.zeros((1, 4), np.int64))):
        with pytest.raises(vbq_amd.VBQError, match="no ROCm device"):
            call()
    with pytest.raises(vbq_amd.VBQError, match="tensor is on cpu"):
        ops.budget_dp_sweep(torch.zeros((5, 3, 2), dtype=torch.float64), 2, [1])
    # what is wrong with the budgets is said before a device is looked for
    with pytest.raises(ValueError, match="total_bits"):
        E.compress_to_records_sweep(mu, sg, [1, 9], tab, 4)
    with pytest.raises(TypeError):
        E.compress_to_records_sweep(mu, sg, [1.5], tab, 4)


def test_budget_lists_are_checked_on_the_host():
    from vbq_amd import rows_budget
    assert rows_budget._budget_list([3, 0, 3], 2, 4) == [3, 0, 3]
    assert rows_budget._budget_list(np.array([8, 1]), 2, 4) == [8, 1]
    assert rows_budget._budget_list(torch.tensor([8, 1]), 2, 4) == [8, 1]
    for bad in ([9], [-1], [0, 1 << 40]):
        with pytest.raises(ValueError, match=r"outside \[0, K\*N = 8\]"):
            rows_budget._budget_list(bad, 2, 4)
    with pytest.raises(TypeError):
        rows_budget._budget_list([1.0], 2, 4)
    assert rows_budget.SWEEP_MAX_BUDGETS == 64 and rows_budget.CURVE_SCRATCH_BYTES == 64 << 20


def test_order_dedup_and_split_at_64_with_a_stubbed_sweep(monkeypatch):
    """ops.budget_dp_sweep replaced by a host stub that records its budget lists and answers bits[s, r, k] = obj[s, r] =
    budgets[s]: the launches get the distinct values ascending, at most 64 each; the slices come back in the caller's order."""
    from vbq_amd import ops, rows_budget
    R, K = 2, 3
    launches = []

    def stub(fhat, k, budgets, *, curve_len=0, status=None, workspace=None):
        budgets = list(budgets)
        assert fhat == "scores" and k == K and status == "status" and curve_len == 0 and workspace is None
        assert budgets == sorted(set(budgets)) and len(budgets) <= 64
        launches.append(budgets)
        b = torch.tensor(budgets, dtype=torch.int32).reshape(-1, 1, 1).expand(len(budgets), R, K).contiguous()
        return b, b[:, :, 0].to(torch.float64), None
    monkeypatch.setattr(ops, "budget_dp_sweep", stub)
    rng = np.random.default_rng(0)
    cases = [[5], [1, 2, 3], [3, 1, 2], [7, 7, 7], [9, 0, 9, 4, 0], list(range(64)), list(range(65)), list(range(199, -1, -1)),
             rng.integers(0, 150, 400).tolist(), []]
    for budgets in cases:
        launches.clear()
        bits, obj = rows_budget._sweep_in_order("scores", K, budgets, "status")
        distinct = sorted(set(budgets))
        assert launches == ([distinct[i:i + 64] for i in range(0, len(distinct), 64)] or [[]]), budgets
        assert tuple(bits.shape) == (len(budgets), R, K) and tuple(obj.shape) == (len(budgets), R)
        assert bits[:, 0, 0].tolist() == budgets and obj[:, 1].tolist() == [float(b) for b in budgets]


# ------------------------------------------------------------------------------------------------------------------ the distortion rule
def _curve_of_reference(rng, K, N, R):
    """(D [K N + 1], the row curves [R, K N + 1]) from budget_dp_rows at every budget, on random non-positive scores."""
    fhat = -np.abs(rng.standard_normal((N + 1, R, K))) * 3
    rows = np.stack([BR.budget_dp_rows(fhat, b)[1] for b in range(K * N + 1)], axis=1)
    return -2.0 * rows.sum(axis=0) / (R * K), rows, fhat


def test_last_value_row_at_full_width_is_the_objective_at_every_budget():
    """What the sweep rests on, in the restatement: the DP run once at width K N + 1 holds, in its last value row, the objective
    of a separate run at every budget, bit for bit -- and a row's curve is not monotone."""
    rng = np.random.default_rng(4)
    seen_non_monotone = False
    for K, N in ((5, 3), (7, 4)):
        _, rows, fhat = _curve_of_reference(rng, K, N, 3)
        R, W = 3, K * N + 1
        T = np.full((R, W), -np.inf)
        T[:, :N + 1] = fhat[:, :, 0].T
        for k in range(1, K):
            cand = np.full((N + 1, R, W), -np.inf)
            for m in range(N + 1):
                cand[m, :, m:] = fhat[m, :, k][:, None] + T[:, :W - m]
            T = cand.max(axis=0)
        assert T.tobytes() == rows.tobytes()
        seen_non_monotone |= bool((np.diff(rows, axis=1) < 0).any() and (np.diff(rows, axis=1) > 0).any())
    assert seen_non_monotone


def test_smallest_total_bits_within_a_distortion():
    from vbq_amd.embeddings import _smallest_bits_within
    rng = np.random.default_rng(8)
    for K, N, R in ((5, 3, 4), (7, 4, 2)):
        D, _, _ = _curve_of_reference(rng, K, N, R)
        for target in list(D) + list(0.5 * (D[:-1] + D[1:])) + [D.max() + 1]:
            want = next(b for b in range(D.size) if D[b] <= target)                       # the rule, restated
            assert _smallest_bits_within(D, target) == want
        with pytest.raises(ValueError, match=re.escape(f"the smallest is {float(D.min())!r}, at total_bits = {int(D.argmin())}")):
            _smallest_bits_within(D, D.min() - 1e-9)
    # hand-made, not monotone: b = 1 qualifies although b = 2 and b = 3 do not; a bisection would land on 4
    D = np.array([9.0, 2.0, 7.0, 5.0, 1.0, 3.0])
    assert _smallest_bits_within(D, 2.5) == 1 and _smallest_bits_within(D, 2.0) == 1 and _smallest_bits_within(D, 1.5) == 4
    assert _smallest_bits_within(D, 9.0) == 0 and _smallest_bits_within(D, np.inf) == 0
    with pytest.raises(ValueError, match=r"the smallest is 1\.0, at total_bits = 4"):     # the minimum is not at the end
        _smallest_bits_within(D, 0.5)
    with pytest.raises(ValueError, match="NaN"):
        _smallest_bits_within(D, np.nan)
