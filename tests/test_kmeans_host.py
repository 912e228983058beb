"""The exact 1-D k-means library (include/vbq_kmeans.h, vbq_amd/kmeans) without a GPU: the restatement of its DP against a
brute force, the fourth library's ABI and refusals, the static stream and refusal-order rules of the first library applied to
its sources, and the host logic of the Python layers.

The guard tables of the first library (footprint.COVERED, stream_order.BY_SOURCE) name the functions of include/vbq.h and the
files of vbq_amd/csrc; tests/test_scores_host.py and tests/test_budget_sweep_host.py hold the second and third library;
libvbq_kmeans.so adds to none of them and this module is its guard.  The names are read FROM the header.

THE BOUND 4 n eps S2[n].  The divide-and-conquer evaluation and the brute force run on the same prefix sums and form the same
rounded cost(i, j) for the same (i, j); they can differ only where rounding breaks the monotonicity the recursion relies on,
that is by no more than rounding moves an objective.  To first order, with u = eps / 2: a prefix sum of j non-negative terms
added in sequence is within j u S2[j] <= n u S2[n] of the real sum.  A segment's cost takes two of them in S2[j] - S2[i-1] and
two of S1 in s * s / m, and by Cauchy-Schwarz s * s / m <= S2[j] - S2[i-1], so the second term's error is bounded like the
first's: 4 n u S2[n] = 2 n eps S2[n] for a cost.  Over the segments of a partition the sums telescope -- the error of a
prefix sum at an interior boundary enters its two neighbours with opposite signs -- so an objective of any number of levels is
within the same 2 n eps S2[n] of its real value, and two evaluations of the optimum within 4 n eps S2[n] of each other."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kmeans_reference as KR  # noqa: E402
from test_abi import declared_functions  # noqa: E402
from test_refusal_order_host import analyse, late_refusals  # noqa: E402
from test_stream_order_host import (async_violations, call_args, forbidden_found, launch_violations,  # noqa: E402
                                    literal_stream_violations, python_site_violations, stream_positions, stream_variable_violations,
                                    strip_c)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbq_kmeans.h")
KMEANS = os.path.join(ROOT, "vbq_amd", "kmeans")
CSRC = os.path.join(ROOT, "vbq_amd", "csrc")
INVALID, WORKSPACE = -1, -4
WHO = "vbqk_kmeans1d_f64"
SHAPES = ((1, 1), (2, 2), (7, 7), (65, 8), (200, 16))


def _read(path):
    with open(path) as f:
        return f.read()


@pytest.fixture(scope="module")
def kmeans_lib():
    from vbq_amd import build
    return build.build_kmeans()


@pytest.fixture(scope="module")
def hk(kmeans_lib):
    from vbq_amd import _lib_kmeans
    return _lib_kmeans.lib()


# ------------------------------------------------------------------------------------------------------------------ the restatement
def _case(name, n, seed=0):
    x = np.sort(KR.family(name, np.random.default_rng([seed, n, KR.FAMILIES.index(name)]), n))
    return (x,) + KR.sums_of(x)


@pytest.mark.parametrize("name", KR.FAMILIES)
def test_the_restatement_against_the_brute_force(name):
    """Objectives within 4 n eps S2[n] of the O(K n^2) DP in every family and shape; boundaries identical on the normal and the
    heavy-tailed family, and on the first three families with Kmax capped at the number of distinct values; the literal
    recursion and its depth-by-depth form identical bit for bit."""
    for n, Kmax in SHAPES:
        x, shift, S1, S2 = _case(name, n)
        sse_r, A_r = KR.dp_recursive(S1, S2, Kmax)
        sse_l, A_l = KR.dp_levels(S1, S2, Kmax)
        sse_b, A_b = KR.dp_brute(S1, S2, Kmax)
        assert sse_r.tobytes() == sse_l.tobytes() and np.array_equal(A_r, A_l), (name, n)
        assert np.abs(sse_l - sse_b).max() <= KR.objective_bound(S2, n), (name, n, sse_l, sse_b)
        cap = min(Kmax, np.unique(x).size)
        if name in ("normal", "student"):
            assert cap == Kmax
        if name in ("normal", "quarters", "student"):
            for k in range(1, cap + 1):
                got, want = KR.walk(A_l, S1, S2, shift, k), KR.walk(A_b, S1, S2, shift, k)
                assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes(), (name, n, k)
                assert np.array_equal(got[2], want[2]) and got[2].sum() == n and (np.diff(got[0]) > 0).all()
        for k in range(1, Kmax + 1):                                   # every family: a valid segmentation, ascending code points
            starts, codes, counts = KR.walk(A_l, S1, S2, shift, k)
            assert starts[0] == 1 and counts.sum() == n and (counts >= 1).all() and (np.diff(codes) >= 0).all()
        assert (np.diff(sse_l) <= KR.objective_bound(S2, n)).all()     # more levels never cost more


def test_the_shift_keeps_the_sums_small():
    """normal + 1000: the sums are those of the centred samples, and the code points come back at 1000."""
    x, shift, S1, S2 = _case("shifted", 200)
    assert 999 < shift < 1001 and S2[200] < 400 and abs(S1[200]) < 200
    starts, codes, counts = KR.walk(KR.dp_levels(S1, S2, 4)[1], S1, S2, shift, 4)
    assert (codes > 995).all() and (codes < 1005).all()
    want = np.array([x[s - 1:s - 1 + c].astype(np.float64).mean() for s, c in zip(starts, counts)])
    assert np.abs(codes - want).max() < 1e-9


def test_the_kernels_node_walk_is_the_recursion():
    """node(t, d, q, n) -- bit d-1-s of t picks the child at step s -- enumerates, depth by depth, exactly the calls of solve,
    in bit_length(n - q + 1) depths."""
    for q, n in ((1, 1), (1, 2), (3, 3), (1, 7), (2, 64), (5, 200), (1, 257), (17, 1000)):
        level = [(q, n)]
        for d in range(KR.depths(q, n)):
            got = [r for r in (KR.node(t, d, q, n) for t in range(1 << d)) if r]
            assert got == level, (q, n, d)
            nxt = []
            for jl, jh in level:
                j = (jl + jh) // 2
                nxt += [r for r in ((jl, j - 1), (j + 1, jh)) if r[0] <= r[1]]
            level = nxt
        assert not level and not any(KR.node(t, KR.depths(q, n), q, n) for t in range(1 << KR.depths(q, n)))


def test_the_launch_plan_restated_is_the_sources(hk):
    text = strip_c(_read(os.path.join(KMEANS, "vbqk_dp.hip")))
    const = lambda name: int(re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text).group(1))
    assert (const("kDpThreads"), const("kDpWaveScan"), const("kDpQueue"), const("kDpMaxLevels"), const("kDpMaxK")) == \
        (KR.THREADS, KR.WAVE_SCAN, KR.QUEUE, KR.MAX_LEVELS, KR.MAX_K)
    assert KR.ROWS_IN_LDS_MAX_N == 4862 and "n <= 4862" in _read(HEADER)
    for n in (1, 64, KR.ROWS_IN_LDS_MAX_N - 1, KR.ROWS_IN_LDS_MAX_N, KR.ROWS_IN_LDS_MAX_N + 1, 100_000):
        for Kmax in (1, 3, 1024):
            if Kmax <= n:
                assert hk.vbqk_kmeans1d_workspace_bytes(n, 1, Kmax) == KR.slice_bytes(n, Kmax), (n, Kmax)
                assert hk.vbqk_kmeans1d_workspace_bytes(n, 3, Kmax) == 3 * KR.slice_bytes(n, Kmax)
    assert KR.slice_bytes(4862, 3) == 12 * 4863 + 12 and KR.slice_bytes(4863, 3) == 12 * 4864 + 16 * 4864      # 12: up to 16
    assert [KR.root_scan_len(2, n) for n in (126, 128, 130)] == [63, 64, 65]


def test_the_optimum_is_no_worse_than_sklearn():
    cluster = pytest.importorskip("sklearn.cluster")
    x, shift, S1, S2 = _case("student", 400)
    for k in (2, 5, 16):
        km = cluster.KMeans(n_clusters=k, n_init=3, random_state=0).fit(x.astype(np.float64).reshape(-1, 1))
        sse = KR.dp_levels(S1, S2, k)[0]
        assert sse[k - 1] <= km.inertia_ * (1 + 1e-9), (k, sse[k - 1], km.inertia_)


# ------------------------------------------------------------------------------------------------------------------ the ABI
def _header_functions():
    """{name: [argument texts]} of include/vbq_kmeans.h."""
    s = strip_c(_read(HEADER))
    return {m.group(1): call_args(s, m.end() - 1) for m in re.finditer(r"\b(vbqk_[a-z0-9_]+)\s*\(", s)}


def test_header_carries_its_own_version_and_error_and_builds_on_vbq_h():
    names = set(_header_functions())
    assert {"vbqk_abi_version", "vbqk_last_error", WHO, "vbqk_kmeans1d_workspace_bytes", "vbqk_nearest_code_channels_f64"} == names
    text = _read(HEADER)
    assert '#include "vbq.h"' in text and "#define VBQK_ABI_VERSION 1" in text
    assert not re.search(r"\bvbq[xb]?_[a-z0-9_]+\s*\(", strip_c(text))       # it declares nothing of the other three libraries


def test_library_exports_exactly_the_header(kmeans_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", kmeans_lib], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r"\b[A-Za-z] (vbqk_[A-Za-z0-9_]+)", out)) == sorted(_header_functions())
    assert not re.search(r"\bvbq[xb]?_", out) and "_ZN" not in out and "_Z" not in out, out


def test_the_first_three_libraries_are_unchanged_in_their_exports_and_files():
    from vbq_amd import build
    exports = lambda lib: subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (vbq[a-z0-9]*_[a-z0-9_]+)", exports(build.build_hip()))) == set(declared_functions())
    assert not any(n.startswith("vbqk") for n in declared_functions())
    for lib, header, prefix in ((build.build_ext(), "vbq_ext.h", "vbqx_"), (build.build_budget(), "vbq_budget.h", "vbqb_")):
        declared = set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", strip_c(_read(os.path.join(ROOT, "include", header)))))
        assert sorted(re.findall(r"\b[A-Za-z] (vbq[a-z0-9]*_[A-Za-z0-9_]+)", exports(lib))) == sorted(declared)
    names = lambda d: sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "vbq_amd", d, "*")))
    assert names("ext") == ["vbqx_api.hip", "vbqx_scores.hip"] and names("budget") == ["vbqb_api.hip", "vbqb_sweep.hip"]
    assert names("kmeans") == ["vbqk_api.hip", "vbqk_dp.hip", "vbqk_nearest.hip"]
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == ["vbq.h", "vbq_budget.h", "vbq_ext.h", "vbq_kmeans.h"]
    assert sorted(os.path.basename(s) for s in build.hip_sources()) == sorted(build.HIP_SOURCES)
    assert not [s for s in build.HIP_SOURCES if "kmeans" in s or s.startswith("vbqk")]


def test_ctypes_binding_mirrors_the_header(hk):
    from vbq_amd import _lib_kmeans
    declared = _header_functions()
    assert sorted(_lib_kmeans.SIGNATURES) == sorted(declared)

    def ctype(arg):
        arg = " ".join(arg.split())
        if "*" in arg:
            return C.c_void_p
        return {"int64_t": C.c_int64, "int32_t": C.c_int32, "size_t": C.c_size_t}[arg.split(" ")[0]]
    text = strip_c(_read(HEADER))
    for name, args in declared.items():
        res, argtypes = _lib_kmeans.SIGNATURES[name]
        assert argtypes == ([] if args == ["void"] else [ctype(a) for a in args]), name
        returns = re.search(r"([A-Za-z_][A-Za-z0-9_ ]*?\**)\s*" + name + r"\s*\(", text).group(1).split()
        assert res == (C.c_char_p if "char" in returns else C.c_size_t if "size_t" in returns else C.c_int), name
    assert hk.vbqk_abi_version() == 1 == _lib_kmeans.ABI_VERSION


def test_missing_library_fails_loudly(monkeypatch, tmp_path, kmeans_lib):
    from vbq_amd import _lib, _lib_kmeans
    monkeypatch.setattr(_lib_kmeans, "_LIB", None)
    monkeypatch.setenv("VBQ_KMEANS_LIBRARY", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.VBQError, match="not built"):
        _lib_kmeans.lib()
    monkeypatch.delenv("VBQ_KMEANS_LIBRARY")
    monkeypatch.setattr(_lib_kmeans, "_LIB", None)
    assert _lib_kmeans.lib() is not None


def test_a_current_library_without_an_object_cache_needs_no_compiler(kmeans_lib, monkeypatch, tmp_path):
    """The tree as it arrives where objects are not shipped: library and flags tag, no vbq_amd/lib/obj/kmeans."""
    import shutil
    from vbq_amd import build
    lib = tmp_path / "lib"
    lib.mkdir()
    for name in ("libvbq_kmeans.so", "vbq_kmeans.flags.txt"):
        shutil.copy2(os.path.join(build.LIBDIR, name), lib / name)
    monkeypatch.setattr(build, "LIBDIR", str(lib))
    monkeypatch.setattr(build, "KMEANS_LIB", str(lib / "libvbq_kmeans.so"))
    monkeypatch.setattr(shutil, "which", lambda name: pytest.fail("looked for a compiler"))
    monkeypatch.setattr(build.subprocess, "run", lambda *a, **k: pytest.fail("started a process"))
    assert build.build_kmeans() == str(lib / "libvbq_kmeans.so") and not (lib / "obj").exists()
    assert "vbq_amd/lib/vbq_kmeans.flags.txt" in _read(os.path.join(ROOT, ".gitignore")).split()
    flags = _read(os.path.join(str(lib), "vbq_kmeans.flags.txt")).split()
    assert "-fvisibility=hidden" in flags and "-ffp-contract=off" in flags and "--offload-arch=gfx950" in flags


# ------------------------------------------------------------------------------------------------------------------ refusals
def _call(hk, **kw):
    """vbqk_kmeans1d_f64 with the address 16 for every non-null pointer: nothing may read through them."""
    a = dict(S1=16, S2=16, shift=16, n=100, C=3, levels=[2, 7], starts=16, codes=16, counts=16, sse=16, status=None, ws=16,
             wsb=1 << 40)
    a.update(kw)
    levels = a["levels"]
    arr = None if levels is None else (C.c_int32 * len(levels))(*levels)
    S = a.get("S", 0 if levels is None else len(levels))
    return hk.vbqk_kmeans1d_f64(a["S1"], a["S2"], a["shift"], a["n"], a["C"], arr, S, a["starts"], a["codes"], a["counts"], a["sse"],
                                a["status"], a["ws"], a["wsb"], None)


def test_the_c_calls_refuse_before_any_device_work(hk):
    """On a host without a GPU: every refusal returns before anything could be launched, and names itself and the value."""
    def refused(rc, code, *texts, who=WHO):
        msg = hk.vbqk_last_error().decode()
        assert rc == code and who in msg and all(t in msg for t in texts), (rc, msg)

    refused(_call(hk, n=0), INVALID, "n=0")
    refused(_call(hk, n=(1 << 30) + 1), INVALID, "n=1073741825", "2^30")
    refused(_call(hk, C=0), INVALID, "C=0")
    refused(_call(hk, levels=[]), INVALID, "S=0")
    refused(_call(hk, levels=list(range(1, 66))), INVALID, "S=65")
    refused(_call(hk, levels=None, S=2), INVALID, "null pointer", "levels")
    refused(_call(hk, levels=[0, 3]), INVALID, "levels[0] = 0", "below 1")
    refused(_call(hk, levels=[3, 3]), INVALID, "levels[1] = 3", "levels[0] = 3", "strictly ascending")
    refused(_call(hk, levels=[3, 5, 4]), INVALID, "levels[2] = 4", "levels[1] = 5", "strictly ascending")
    refused(_call(hk, n=5000, levels=[2, 1025]), INVALID, "Kmax = 1025", "1024")
    refused(_call(hk, n=6, levels=[2, 7]), INVALID, "Kmax = 7", "n = 6")
    for name in ("S1", "S2", "shift", "starts", "codes", "counts", "sse"):
        refused(_call(hk, **{name: None}), INVALID, "null pointer")
    one = KR.slice_bytes(100, 7)
    refused(_call(hk, ws=None, wsb=one), WORKSPACE, "workspace")
    refused(_call(hk, wsb=one - 1), WORKSPACE, f"workspace of {one - 1} bytes", str(one))
    refused(_call(hk, wsb=0), WORKSPACE, "workspace of 0 bytes")
    refused(_call(hk, ws=24), WORKSPACE, "16-byte aligned")
    for bad in (dict(n=0), dict(C=0), dict(Kmax=0), dict(Kmax=1025), dict(n=6)):
        a = dict(n=100, C=3, Kmax=7)
        a.update(bad)
        assert hk.vbqk_kmeans1d_workspace_bytes(a["n"], a["C"], a["Kmax"]) == 0
    who = "vbqk_nearest_code_channels_f64"
    near = lambda **kw: hk.vbqk_nearest_code_channels_f64(*[{**dict(x=16, B=5, C=3, codes=16, k=4, i=16, q=16, cnt=None), **kw}[f]
                                                            for f in ("x", "B", "C", "codes", "k", "i", "q", "cnt")], None)
    refused(near(B=-1), INVALID, "B=-1", who=who)
    refused(near(C=0), INVALID, "C=0", who=who)
    for k in (0, 1025):
        refused(near(k=k), INVALID, f"k={k}", who=who)
    refused(near(x=None), INVALID, "null input", who=who)
    refused(near(codes=None), INVALID, "null input", who=who)
    assert near(B=0, x=None, codes=None) == 0                          # nothing to do: nothing is read


# ------------------------------------------------------------------------------------------------------------------ static rules
def _kmeans_sources():
    files = {os.path.basename(p): _read(p) for p in sorted(glob.glob(os.path.join(KMEANS, "*")))}
    assert sorted(files) == ["vbqk_api.hip", "vbqk_dp.hip", "vbqk_nearest.hip"], sorted(files)
    return files


def test_every_launch_of_the_fourth_library_names_the_callers_stream():
    files = _kmeans_sources()
    launches = 0
    for name, text in files.items():
        n, bad = launch_violations(text)
        launches += n
        assert not bad and n == len(re.findall(r"\bhipLaunchKernelGGL\b", strip_c(text))), (name, bad)
        assert async_violations(text)[1] == [], name
        assert stream_variable_violations(text)[1] == [], name
        assert forbidden_found(text) == [] and literal_stream_violations(text) == [], name
    assert launches == 2 and stream_variable_violations(files["vbqk_dp.hip"])[0] >= 2
    planted = files["vbqk_dp.hip"].replace("p.lds_bytes, st, S1,", "p.lds_bytes, 0, S1,")
    assert planted != files["vbqk_dp.hip"] and launch_violations(planted)[1] and literal_stream_violations(planted)
    planted = files["vbqk_nearest.hip"].replace("    const int kpad = k | 1;", "    const int kpad = k | 1;\n    hipDeviceSynchronize();")
    assert planted != files["vbqk_nearest.hip"] and forbidden_found(planted) == ["hipDeviceSynchronize"]


def test_no_refusal_of_the_fourth_library_stands_after_an_enqueue():
    """The walk of tests/test_refusal_order_host.py over vbq_amd/kmeans and the header it shares with vbq_amd/csrc."""
    files = _kmeans_sources()
    files["vbq_common.h"] = _read(os.path.join(CSRC, "vbq_common.h"))
    bodies, enq, ref, _ = analyse(files)
    entries = {n for n in _header_functions() if n.endswith("_f64")}
    assert len(entries) == 2 and entries <= set(bodies) and entries <= enq and entries <= ref
    assert "dp_launch" in enq and not {"dp_check", "dp_plan"} & enq and "dp_check" in ref
    assert not {n for n in _header_functions() if not n.endswith("_f64")} & (enq | ref)
    assert late_refusals(files) == []
    text = files["vbqk_dp.hip"]
    late = text.replace("    int64_t grid = (int64_t)", "    hipLaunchKernelGGL(k_late, dim3(1), dim3(64), 0, st, d_status);\n"
                        "    VBQ_REQUIRE(d_status, VBQ_ERR_INVALID_ARGUMENT, \"late\");\n    int64_t grid = (int64_t)")
    assert late != text
    assert ("vbqk_dp.hip", WHO, "VBQ_REQUIRE") in late_refusals({**files, "vbqk_dp.hip": late})


def test_every_python_call_site_of_the_fourth_library_passes_the_tensors_stream():
    """The rule of tests/test_stream_order_host.py reads names that start with `vbq_`: the fourth library's are spelled
    `vbq_k_...` for it, in the header and in the Python text alike."""
    spell = lambda text: text.replace("vbqk_", "vbq_k_")
    pos = stream_positions(spell(_read(HEADER)))
    assert pos == {spell(WHO): 14, spell("vbqk_nearest_code_channels_f64"): 8}
    total, called = 0, set()
    for path in sorted(glob.glob(os.path.join(ROOT, "vbq_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py"))):
        text = spell(_read(path))
        seen, bad = python_site_violations(text, pos, os.path.basename(path))
        total += seen
        called |= {m for m in re.findall(r"\.(vbq_k_[a-z0-9_]+)\b", text) if m in pos}
        assert not bad, (path, bad)
    assert total >= 2 and called == set(pos)
    text = spell(_read(os.path.join(ROOT, "vbq_amd", "kmeans1d.py")))
    planted = text.replace("_ptr(counts), _stream(x)),", "_ptr(counts), None),")
    assert planted != text and python_site_violations(planted, pos, "kmeans1d.py")[1]
    # and the quantizer's own quantize goes through the first library's call with the tensor's stream
    base = _read(os.path.join(ROOT, "vbq_amd", "baselines.py"))
    assert "class OptimalKmeansQuantizer(KmeansQuantizer)" in base and base.count("vbq_nearest_code_f64(") == 1


# ------------------------------------------------------------------------------------------------------------------ the Python layers
def test_python_layers_refuse_without_a_device(monkeypatch):
    import vbq_amd
    from vbq_amd import kmeans1d
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)    # a host without a device, wherever this runs
    x = np.zeros((9, 2), np.float32)
    for call in (lambda: kmeans1d.prefix_sums(x), lambda: kmeans1d.fit_channels(x, [2, 3]), lambda: kmeans1d.sse_curve(x, 4),
                 lambda: vbq_amd.OptimalKmeansQuantizer(3).fit(x[:, 0]),
                 lambda: vbq_amd.ChannelwiseOptimalKmeansWrapper(2, [2, 3]).fit_latents(x, 1.0)):
        with pytest.raises(vbq_amd.VBQError, match="no ROCm device"):
            call()
    w = vbq_amd.ChannelwiseOptimalKmeansWrapper(2, [2])
    w.code_points, w.code_lengths = {2: np.zeros((2, 2))}, {2: np.zeros((2, 2))}
    with pytest.raises(vbq_amd.VBQError, match="no ROCm device"):
        w.compress_latents(x)
    for call in (lambda: kmeans1d.kmeans1d_dp(torch.zeros((2, 10), dtype=torch.float64), torch.zeros((2, 10), dtype=torch.float64),
                                              torch.zeros(2, dtype=torch.float64), [1]),
                 lambda: kmeans1d.nearest_code_channels(torch.zeros((5, 2)), torch.zeros((2, 3), dtype=torch.float64))):
        with pytest.raises(vbq_amd.VBQError, match="tensor is on cpu"):
            call()
    # what is wrong with the samples or the levels is said before a device is looked for
    with pytest.raises(ValueError, match=r"n_samples=9 should be >= n_clusters=10"):
        kmeans1d.fit_channels(x, [2, 10])
    with pytest.raises(ValueError, match=r"outside \[1, 1024\]"):
        kmeans1d.fit_channels(np.zeros((5000, 1), np.float32), [1025])
    with pytest.raises(ValueError, match=r"\[B, C\]"):
        kmeans1d.fit_channels(x[:, 0], [2])
    with pytest.raises(TypeError):
        kmeans1d.fit_channels(x, [1.5])
    assert {"OptimalKmeansQuantizer", "ChannelwiseOptimalKmeansWrapper"} <= set(vbq_amd.__all__)


def test_float64_samples_are_refused_as_the_other_baselines_refuse_them(monkeypatch):
    from vbq_amd import kmeans1d, ops
    monkeypatch.setattr(ops, "current_device", lambda who: torch.device("cpu"))
    for x in (np.zeros((9, 2)), torch.zeros((9, 2), dtype=torch.float64)):
        with pytest.raises(ValueError, match="float64 samples are not supported"):
            kmeans1d.fit_channels(x, [2])


def test_level_lists_are_checked_on_the_host():
    from vbq_amd import kmeans1d
    assert kmeans1d._level_list([3, 1, 3], 5) == [3, 1, 3]
    assert kmeans1d._level_list(np.array([5, 1]), 5) == [5, 1] and kmeans1d._level_list(torch.tensor([2]), 5) == [2]
    for bad, text in (([0], "outside"), ([-1], "outside"), ([1025], "outside"), ([6], "n_samples=5"), ([], "no level counts")):
        with pytest.raises(ValueError, match=text):
            kmeans1d._level_list(bad, 5 if bad != [1025] else 5000)
    assert kmeans1d.MAX_LEVELS_PER_LAUNCH == 64 == KR.MAX_LEVELS and kmeans1d.MAX_LEVEL_COUNT == 1024 == KR.MAX_K


def test_order_repeats_and_the_split_at_64_with_a_stubbed_launch(monkeypatch):
    """kmeans1d_dp replaced by a host stub that records its level lists and answers codes[c, :] = counts[c, :] = k: the launches
    get the distinct values ascending, at most 64 each; the answers come back in the caller's order."""
    from vbq_amd import kmeans1d
    Cn = 2
    launches = []

    def stub(S1, S2, shift, levels, *, status=None, workspace=None):
        levels = list(levels)
        assert (S1, S2, shift, status) == ("S1", "S2", "shift", "status") and workspace is None
        assert levels == sorted(set(levels)) and 1 <= len(levels) <= 64
        launches.append(levels)
        full = lambda k, dt: torch.full((Cn, k), k, dtype=dt)
        return ([full(k, torch.int32) for k in levels], [full(k, torch.float64) for k in levels],
                [full(k, torch.int64) for k in levels], torch.zeros((Cn, levels[-1]), dtype=torch.float64))
    monkeypatch.setattr(kmeans1d, "kmeans1d_dp", stub)
    rng = np.random.default_rng(0)
    for levels in ([5], [1, 2, 3], [3, 1, 2], [7, 7, 7], [9, 1, 9, 4, 1], list(range(1, 65)), list(range(1, 66)),
                   list(range(200, 0, -1)), rng.integers(1, 150, 400).tolist()):
        launches.clear()
        codes, counts = kmeans1d._fit_in_order("S1", "S2", "shift", levels, "status")
        distinct = sorted(set(levels))
        assert launches == [distinct[i:i + 64] for i in range(0, len(distinct), 64)], levels
        assert [tuple(c.shape) for c in codes] == [(Cn, k) for k in levels] == [tuple(c.shape) for c in counts]
        assert [float(c[0, 0]) for c in codes] == [float(k) for k in levels] and [int(c[1, -1]) for c in counts] == levels
