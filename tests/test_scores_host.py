"""Listed rows (include/vbq_ext.h, vbq_amd/ext) without a GPU: the exact restatement tests/scores_reference.py against itself,
the second library's ABI, its refusals, the static stream and refusal-order rules of the first library applied to its sources,
and the Python layer's argument errors.

The guard tables of the first library (footprint.COVERED, stream_order.BY_SOURCE, quantizer_histories.PROBED) name the
functions of include/vbq.h and the files of vbq_amd/csrc; libvbq_ext.so adds to neither, and this module is its guard: the
exports are exactly the header's, every launch names the caller's stream, no refusal stands after an enqueue, every Python
call site passes ops._stream(...)."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import scores_reference as SR  # noqa: E402
import topk_reference as TR  # noqa: E402
from test_abi import declared_functions  # noqa: E402
from test_refusal_order_host import analyse, late_refusals  # noqa: E402
from test_stream_order_host import (async_violations, call_args, forbidden_found, launch_violations,  # noqa: E402
                                    literal_stream_violations, python_site_violations, stream_positions, stream_variable_violations,
                                    strip_c)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vbq_ext.h")
EXT = os.path.join(ROOT, "vbq_amd", "ext")
CSRC = os.path.join(ROOT, "vbq_amd", "csrc")
NAMES = ["vbqx_abi_version", "vbqx_last_error", "vbqx_records_scores_f32", "vbqx_scores_f32"]
INVALID, UNSUPPORTED = -1, -2


def _read(path):
    with open(path) as f:
        return f.read()


@pytest.fixture(scope="module")
def ext_lib():
    from vbq_amd import build
    return build.build_ext()


@pytest.fixture(scope="module")
def hx(ext_lib):
    from vbq_amd import _lib_ext
    return _lib_ext.lib()


# ------------------------------------------------------------------------------------------------------------------ the reference
def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def test_fma_rounds_once_where_multiply_then_add_rounds_twice():
    """Planted: a = b = 1 + 2^-12, c = -1.  a * b = 1 + 2^-11 + 2^-24 needs 25 bits: float32 drops the 2^-24, the fma keeps it."""
    a = np.float32(1 + 2.0 ** -12)
    fused = SR.fma32_exact(a, a, np.float32(-1))
    twice = np.float32(a * a) + np.float32(-1)
    assert float(fused) == 2.0 ** -11 + 2.0 ** -24 and float(twice) == 2.0 ** -11 and fused != twice
    assert SR.fma32(a, a, np.float32(-1)).view(np.uint32) == fused.view(np.uint32)


def test_vectorised_fma_equals_the_exact_one_on_random_and_midpoint_cases():
    rng = np.random.default_rng(5)
    n = 400
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    c[::5] = -(a[::5] * b[::5])                                  # near cancellation: the sum's low bits decide
    # midpoints: 1 * x + y with x + y exactly half way between two float32 numbers (ties to even both ways), and one
    # float64 rounding away from such a midpoint: x = 2^24 + 2 (or + 6) and y = 1 +- 2^-40 products
    mid_a = np.array([1, 1, 1, 1, 3, 3], np.float32)
    mid_b = np.array([2.0 ** 24 + 2, 2.0 ** 24 + 4, -(2.0 ** 24 + 2), 2.0 ** 25 + 4, 2.0 ** 23 + 1, 2.0 ** 23 + 3], np.float32)
    mid_c = np.array([1, 1, -1, 2, 0.5, 2.0 ** -30], np.float32)
    # signed zeros and cancellation
    z_a = np.array([0, -0.0, -0.0, 2, 0], np.float32)
    z_b = np.array([1, 1, 1, 3, -5], np.float32)
    z_c = np.array([-0.0, -0.0, 0, -6, 0], np.float32)
    # subnormal results and overflow
    e_a = _f32([0x00800000, 0x00800001, 0x7F7FFFFF, 0x00000001])
    e_b = np.array([0.5, 0.75, 2, 0.5], np.float32)
    e_c = _f32([0x00000001, 0x00000000, 0x7F7FFFFF, 0x00000000])
    a, b, c = (np.concatenate(t) for t in ((a, mid_a, z_a, e_a), (b, mid_b, z_b, e_b), (c, mid_c, z_c, e_c)))
    with np.errstate(over="ignore"):
        got = SR.fma32(a, b, c)
    want = np.array([SR.fma32_exact(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    with np.errstate(over="ignore"):
        two_roundings = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (two_roundings.view(np.uint32) != want.view(np.uint32)).any()        # the cases tell float64-then-float32 apart


@pytest.mark.parametrize("metric", ("dot", "cosine"))
@pytest.mark.parametrize("K,V,Q", [(1, 1, 1), (5, 33, 3), (65, 130, 2), (300, 33, 2)])
def test_reference_stays_within_the_float64_bounds(K, V, Q, metric):
    emb, q, _ = TR.case_data(K, V, Q)
    ids = np.tile(np.arange(V), (Q, 1))
    got, st = SR.scores(q, emb, ids, metric)
    assert st == 0 and got.dtype == np.float32 and got.shape == (Q, V)
    assert (np.abs(got.astype(np.float64) - TR.scores(q, emb, metric)) <= TR.bounds(q, emb, metric)).all()


def test_reference_padding_and_rows_out_of_range():
    emb, q, _ = TR.case_data(5, 33, 3)
    ids = np.array([[0, -1, 32], [33, 1, 1], [-7, 2, 1 << 40]])
    got, st = SR.scores(q, emb, ids, "dot")
    assert st == SR.BAD_ROW and np.isneginf(got[[0, 1, 2, 2], [1, 0, 0, 2]]).all() and np.isfinite(got).sum() == 5
    assert got[1, 1].view(np.uint32) == got[1, 2].view(np.uint32)
    assert SR.scores(q, emb, ids[:1], "cosine")[1] == 0


# ------------------------------------------------------------------------------------------------------------------ the ABI
def _header_functions():
    """{name: [argument texts]} of include/vbq_ext.h."""
    s = strip_c(_read(HEADER))
    return {m.group(1): call_args(s, m.end() - 1) for m in re.finditer(r"\b(vbqx_[a-z0-9_]+)\s*\(", s)}


def test_header_declares_exactly_the_four_functions():
    assert sorted(_header_functions()) == NAMES
    assert '#include "vbq.h"' in _read(HEADER)


def test_library_exports_exactly_the_header(ext_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", ext_lib], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r"\b[A-Za-z] (vbqx_[A-Za-z0-9_]+)", out)) == NAMES
    assert not re.search(r"\bvbq_", out) and "_ZN" not in out and "_Z" not in out, out


def test_first_library_is_unchanged_in_its_exports():
    from vbq_amd import build
    out = subprocess.run(["nm", "-D", "--defined-only", build.build_hip()], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (vbq[a-z0-9]*_[a-z0-9_]+)", out)) == set(declared_functions())
    assert not any(n.startswith("vbqx") for n in declared_functions())
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(EXT, "*.hip"))) == ["vbqx_api.hip", "vbqx_scores.hip"]


def test_ctypes_binding_mirrors_the_header(hx):
    import ctypes as C
    from vbq_amd import _lib_ext
    declared = _header_functions()
    assert sorted(_lib_ext.SIGNATURES) == sorted(declared)

    def ctype(arg):
        arg = " ".join(arg.split())
        if "*" in arg:
            return C.c_void_p
        return {"int64_t": C.c_int64, "int32_t": C.c_int32}[arg.split(" ")[0]]
    for name, args in declared.items():
        res, argtypes = _lib_ext.SIGNATURES[name]
        assert argtypes == ([] if args == ["void"] else [ctype(a) for a in args]), name
        assert res == (C.c_char_p if name == "vbqx_last_error" else C.c_int)
    assert hx.vbqx_abi_version() == 1 == _lib_ext.ABI_VERSION and "#define VBQX_ABI_VERSION 1" in _read(HEADER)


def test_missing_library_fails_loudly(monkeypatch, tmp_path, ext_lib):
    from vbq_amd import _lib, _lib_ext
    monkeypatch.setattr(_lib_ext, "_LIB", None)
    monkeypatch.setenv("VBQ_EXT_LIBRARY", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.VBQError, match="not built"):
        _lib_ext.lib()
    monkeypatch.delenv("VBQ_EXT_LIBRARY")
    monkeypatch.setattr(_lib_ext, "_LIB", None)
    assert _lib_ext.lib() is not None


def test_a_current_library_without_an_object_cache_needs_no_compiler(ext_lib, monkeypatch, tmp_path):
    """The tree as it arrives where objects are not shipped: library and flags tag, no vbq_amd/lib/obj/ext."""
    import shutil
    from vbq_amd import build
    lib = tmp_path / "lib"
    lib.mkdir()
    for name in ("libvbq_ext.so", "vbq_ext.flags.txt"):
        shutil.copy2(os.path.join(build.LIBDIR, name), lib / name)
    monkeypatch.setattr(build, "LIBDIR", str(lib))
    monkeypatch.setattr(build, "EXT_LIB", str(lib / "libvbq_ext.so"))
    monkeypatch.setattr(shutil, "which", lambda name: pytest.fail("looked for a compiler"))
    monkeypatch.setattr(build.subprocess, "run", lambda *a, **k: pytest.fail("started a process"))
    assert build.build_ext() == str(lib / "libvbq_ext.so") and not (lib / "obj").exists()
    assert "vbq_amd/lib/vbq_ext.flags.txt" in _read(os.path.join(ROOT, ".gitignore")).split()


# ------------------------------------------------------------------------------------------------------------------ refusals
def _records(hx, **kw):
    a = dict(words=1, V=10, K=4, N=10, bits=12, table=1, n_tables=1, queries=1, Q=2, ids=1, M=3, metric=1, out=1, status=None)
    a.update(kw)
    return hx.vbqx_records_scores_f32(a["words"] or None, a["V"], a["K"], a["N"], a["bits"], a["table"] or None, a["n_tables"],
                                      a["queries"] or None, a["Q"], a["ids"] or None, a["M"], a["metric"], a["out"] or None,
                                      a["status"], None)


def _dense(hx, **kw):
    a = dict(emb=1, V=10, K=4, queries=1, Q=2, ids=1, M=3, metric=1, out=1, status=None)
    a.update(kw)
    return hx.vbqx_scores_f32(a["emb"] or None, a["V"], a["K"], a["queries"] or None, a["Q"], a["ids"] or None, a["M"],
                              a["metric"], a["out"] or None, a["status"], None)


def test_the_c_calls_refuse_before_any_device_work(hx):
    """On a host without a GPU: every refusal below returns before anything could be launched, and names itself.  The non-null
    pointers are the address 1: nothing may read through them."""
    def refused(rc, code, *texts):
        msg = hx.vbqx_last_error().decode()
        assert rc == code and all(t in msg for t in texts), (rc, msg)

    for call, who in ((_records, "vbqx_records_scores_f32"), (_dense, "vbqx_scores_f32")):
        refused(call(hx, K=0), INVALID, who, "K=0")
        refused(call(hx, V=0), INVALID, who, "V=0")
        refused(call(hx, Q=-1), INVALID, who, "Q=-1")
        refused(call(hx, M=-1), INVALID, who, "M=-1")
        for metric in (-1, 2):
            refused(call(hx, metric=metric), INVALID, who, f"metric {metric}")
        # the grid: one workgroup per group of 64 pairs at K = 4, at most 2^31 - 1 of them
        refused(call(hx, Q=1 << 40, M=1 << 40), INVALID, who, "grid limit", "2147483647 groups of 64 pairs")
        refused(call(hx, Q=(1 << 31) - 1, M=65), INVALID, who, "grid limit")
        refused(call(hx, Q=1 << 62, M=4), INVALID, who, "grid limit")
        for name in ("queries", "ids", "out"):
            refused(call(hx, **{name: 0}), INVALID, who, "null pointer")
        # the LDS: K above what the smallest group of 8 pairs allows
        refused(call(hx, K=20000, bits=0), UNSUPPORTED, who, "K = 20000", "163840", "every K <= 3500 fits")
    refused(_dense(hx, emb=0), INVALID, "null pointer")
    for name in ("words", "table"):
        refused(_records(hx, **{name: 0}), INVALID, "null pointer")
    for N in (0, 11):
        refused(_records(hx, N=N), INVALID, f"N={N}")
    for bits in (-1, 41):
        refused(_records(hx, bits=bits), INVALID, "total_bits", "[0, K*N = 40]")
    for n_tables in (0, 2, 5):
        refused(_records(hx, n_tables=n_tables), INVALID, f"n_tables = {n_tables}")
    assert _records(hx, n_tables=4, Q=0) == 0                   # n_tables = K is allowed
    # every K <= 3500 is planned, whatever N, total_bits and n_tables: the call goes on to its pointer check
    refused(_records(hx, K=3500, bits=35000, out=0), INVALID, "null pointer")
    refused(_records(hx, K=3500, bits=35000, n_tables=3500, out=0), INVALID, "null pointer")
    refused(_dense(hx, K=3500, out=0), INVALID, "null pointer")


def test_no_queries_or_no_ids_is_no_work(hx):
    for call in (_records, _dense):
        for kw in (dict(Q=0), dict(M=0), dict(Q=0, M=0)):
            assert call(hx, **kw) == 0
            assert call(hx, queries=0, ids=0, out=0, **kw) == 0   # nothing is read or written: the pointers may be null
    assert _records(hx, Q=0, K=0) == INVALID                     # but the sizes are still checked


# ------------------------------------------------------------------------------------------------------------------ static rules
def _ext_sources():
    files = {os.path.basename(p): _read(p) for p in sorted(glob.glob(os.path.join(EXT, "*")))}
    assert sorted(files) == ["vbqx_api.hip", "vbqx_scores.hip"], sorted(files)
    return files


def test_every_launch_of_the_second_library_names_the_callers_stream():
    files = _ext_sources()
    launches = 0
    for name, text in files.items():
        n, bad = launch_violations(text)
        launches += n
        assert not bad and n == len(re.findall(r"\bhipLaunchKernelGGL\b", strip_c(text))), (name, bad)
        assert async_violations(text)[1] == [], name
        assert stream_variable_violations(text)[1] == [], name
        assert forbidden_found(text) == [] and literal_stream_violations(text) == [], name
    assert launches == 1 and stream_variable_violations(files["vbqx_scores.hip"])[0] >= 3
    planted = files["vbqx_scores.hip"].replace("lds, st, a);", "lds, 0, a);")
    assert planted != files["vbqx_scores.hip"] and launch_violations(planted)[1] and literal_stream_violations(planted)


def test_no_refusal_of_the_second_library_stands_after_an_enqueue():
    """The walk of tests/test_refusal_order_host.py over vbq_amd/ext and the headers it shares with vbq_amd/csrc."""
    files = _ext_sources()
    for h in ("vbq_records_common.h", "vbq_common.h"):
        files[h] = _read(os.path.join(CSRC, h))
    bodies, enq, ref, _ = analyse(files)
    entries = {"vbqx_records_scores_f32", "vbqx_scores_f32"}
    assert entries <= set(bodies) and entries <= enq and entries <= ref
    assert {"scores_launch", "scores_launch_as"} <= enq and not {"scores_plan", "scores_check", "record_check_words"} & enq
    assert {"scores_plan", "scores_check", "record_check_words", "record_check_total_bits"} <= ref
    assert late_refusals(files) == []
    late = files["vbqx_scores.hip"].replace("    return scores_launch<false>(", "    if (int rc = scores_launch<false>(who, a, metric, lds, "
                                            "reinterpret_cast<hipStream_t>(stream))) return rc;\n    VBQ_REQUIRE(d_status, "
                                            "VBQ_ERR_INVALID_ARGUMENT, \"late\");\n    return scores_launch<false>(")
    assert late != files["vbqx_scores.hip"]
    assert ("vbqx_scores.hip", "vbqx_scores_f32", "VBQ_REQUIRE") in late_refusals({**files, "vbqx_scores.hip": late})


def test_every_python_call_site_of_the_second_library_passes_the_tensors_stream():
    """The rule of tests/test_stream_order_host.py reads names that start with `vbq_`: the second library's are spelled
    `vbq_x_...` for it, in the header and in the Python text alike."""
    spell = lambda text: text.replace("vbqx_", "vbq_x_")
    pos = stream_positions(spell(_read(HEADER)))
    assert pos == {"vbq_x_records_scores_f32": 14, "vbq_x_scores_f32": 10}
    total, called = 0, set()
    for path in sorted(glob.glob(os.path.join(ROOT, "vbq_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py"))):
        text = spell(_read(path))
        seen, bad = python_site_violations(text, pos, os.path.basename(path))
        total += seen
        called |= {m for m in re.findall(r"\.(vbq_x_[a-z0-9_]+)\b", text) if m in pos}
        assert not bad, (path, bad)
    assert total == 2 and called == set(pos)
    planted = spell(_read(os.path.join(ROOT, "vbq_amd", "ops.py"))).replace("_ptr(status), _stream(emb)), \"vbq_x_scores_f32\")",
                                                                             "_ptr(status), None), \"vbq_x_scores_f32\")")
    assert python_site_violations(planted, pos, "ops.py")[1]


# ------------------------------------------------------------------------------------------------------------------ the Python layer
def test_python_layer_refuses_without_a_device():
    """embeddings.scores / similarity / rerank check ids and k on the host before they look for a device; the query checks
    are most_similar's (_query_args), which run where the queries live -- here on the CPU."""
    from vbq_amd import embeddings as E
    emb = np.zeros((5, 3), np.float32)
    q = np.ones((2, 3), np.float32)
    for bad in (np.zeros((2, 2)), np.array([[True, False]] * 2), [[0.5, 1], [1, 2]]):
        with pytest.raises(IndexError, match="integers"):
            E.scores(emb, q, bad)
    with pytest.raises(IndexError, match="integers"):
        E.rerank(emb, q, torch.zeros((2, 2), dtype=torch.float32))
    for bad in ([[0, 5], [1, 1]], [[0, 1], [1 << 40, -1]], torch.tensor([[4, 4], [4, 5]])):
        with pytest.raises(IndexError, match=r"outside \[0, 5\)"):
            E.scores(emb, q, bad)
        with pytest.raises(IndexError, match=r"outside \[0, 5\)"):
            E.rerank(emb, q, bad)
    for bad in ([0, 1], [[0, 1]], [[[0], [1]]], np.zeros((3, 2), np.int64)):
        with pytest.raises(ValueError, match="ids must be"):
            E.scores(emb, q, bad)
    with pytest.raises(ValueError, match="ids must be"):
        E.scores(emb, q[0], [[0, 1], [2, 3]])
    with pytest.raises(ValueError, match=r"\[V, K\]"):
        E.scores(emb.reshape(-1), q, [[0], [1]])
    for k in (0, 3, -1):
        with pytest.raises(ValueError, match=r"outside 1..M = 2"):
            E.rerank(emb, q, [[0, 1], [2, -1]], k=k)
    with pytest.raises(TypeError):
        E.rerank(emb, q, [[0, 1], [2, -1]], k=1.5)
    for a, b in (([0, -1], [1, 2]), ([0, 1], [1, -2]), ([5, 1], [1, 2]), ([0, 1], [1, 5])):
        with pytest.raises(IndexError, match="outside"):
            E.similarity(emb, a, b)
    with pytest.raises(IndexError, match="integers"):
        E.similarity(emb, [0.0, 1.0], [1, 2])
    with pytest.raises(ValueError, match="differ in shape"):
        E.similarity(emb, [0, 1], [[1, 2]])
    with pytest.raises(ValueError, match=r"\[V, K\]"):
        E.similarity(emb[0], [0], [1])
    # the query checks, shared with most_similar
    cpu = torch.device("cpu")
    assert E._search_args(q, 3, 4, "dot", None, cpu)[0].tolist() == E._query_args(q, 3, "dot", cpu).tolist() == q.tolist()
    unit = E._query_args(q[0], 3, "cosine", cpu)
    assert tuple(unit.shape) == (1, 3) and unit.dtype == torch.float32
    assert np.array_equal(unit.numpy(), (q[:1] / (np.float32(1e-8) + np.sqrt(np.float32(3)))).astype(np.float32))
    for bad in (q[:, :2], q[None], np.ones((2, 4), np.float32)):
        with pytest.raises(ValueError, match="queries must be"):
            E._query_args(bad, 3, "cosine", cpu)
    for poison in (np.nan, np.inf, -np.inf):
        bad = q.copy()
        bad[1, 2] = poison
        with pytest.raises(ValueError, match="NaN or an infinity"):
            E._query_args(bad, 3, "dot", cpu)
    for metric in ("l2", 0, None):
        with pytest.raises(ValueError, match="metric"):
            E._query_args(q, 3, metric, cpu)


def test_rerank_order_on_the_host():
    """The two stable sorts on CPU tensors against topk_reference.order: ties by id, -0.0 == 0.0, duplicates, padding last."""
    from vbq_amd import embeddings as E
    s = np.array([[1.0, -0.0, 0.0, 1.0, -np.inf, 2.0, 0.0, -np.inf, -3.0]], np.float32)
    ids = np.array([[9, 4, 2, 3, -1, 7, 2, -5, 0]], np.int64)
    got_ids, got_s = E._rerank(torch.from_numpy(s), torch.from_numpy(ids), 9)
    assert got_ids.tolist() == [[7, 3, 9, 2, 2, 4, 0, -1, -1]]
    assert got_s.numpy().view(np.uint32)[0].tolist() == s[0, [5, 3, 0, 2, 6, 1, 8, 4, 7]].view(np.uint32).tolist()
    by_row = np.full(10, np.nan)
    by_row[ids[0, ids[0] >= 0]] = s[0, ids[0] >= 0]
    assert got_ids[0, :7].tolist() == TR.order(by_row, ids[0, ids[0] >= 0]).tolist()
    assert E._rerank(torch.from_numpy(s), torch.from_numpy(ids), 3)[0].tolist() == [[7, 3, 9]]
    assert E._rerank_k(None, 9) == 9 and E._rerank_k(None, 0) == 0 and E._rerank_k(np.int64(2), 9) == 2
