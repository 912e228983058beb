"""The resident latent store (vbq_amd/store: vbq_store.h, vbqs_*.hip, LatentStore) without a GPU: the restatement of the
planning kernel against bitstream.box_segments, the bound the store sizes its lists by, the validity rule at its edges, the fifth
library's ABI and refusals, and the static rules of the first library's sources applied to the new tree.

The guard tables of the first library (footprint.COVERED, stream_order.BY_SOURCE, dirty_memory's catalogue) name the functions
of include/vbq.h, the files of vbq_amd/csrc and the top-level modules of vbq_amd; libvbq_store.so and vbq_amd/store add to none of
them, and this module with tests/test_gpu_store.py is their guard.  The names are read FROM the header."""
import ctypes as C
import glob
import importlib
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import store_reference as SR  # noqa: E402
from test_stream_order_host import (async_violations, call_args, forbidden_found, launch_violations,  # noqa: E402
                                    literal_stream_violations, python_site_violations, stream_positions, stream_variable_violations,
                                    strip_c)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORE = os.path.join(ROOT, "vbq_amd", "store")
HEADER = os.path.join(STORE, "vbq_store.h")
INVALID = -1
WHO = "vbqs_plan_boxes"


def _read(path):
    with open(path) as f:
        return f.read()


@pytest.fixture(scope="module")
def store_lib():
    from vbq_amd import build
    return build.build_store()


@pytest.fixture(scope="module")
def hs(store_lib):
    from vbq_amd import _lib_store
    return _lib_store.lib()


# ------------------------------------------------------------------------------------------------------------------ the restatement
def _boxes(dims):
    for lo in itertools.product(*(range(d) for d in dims)):
        for hi in itertools.product(*(range(l + 1, d + 1) for l, d in zip(lo, dims))):
            yield lo, hi


def test_the_lists_are_box_segments_exhaustively_on_small_geometries():
    """Every box of every geometry up to 5 x 5 x 6 at segments 1..7: the run-by-run list is bitstream.box_segments entry for
    entry, and no list is longer than the bound."""
    from vbq_amd import bitstream
    cases = 0
    for dims in itertools.product(range(1, 6), range(1, 6), range(1, 7)):
        boxes = list(_boxes(dims))
        for seg in range(1, 8):
            for lo, hi in boxes:
                ext = tuple(h - l for l, h in zip(lo, hi))
                got = SR.box_list(dims, lo, ext, seg)
                assert got == bitstream.box_segments(dims, lo, hi, seg).tolist(), (dims, lo, hi, seg)
                assert len(got) <= SR.max_listed_segments(dims, ext, seg), (dims, lo, hi, seg)
                cases += 1
    assert cases == 35 * 35 * 56 * 7                   # d (d + 1) / 2 boxes per level of extent d, seven segment lengths


def test_the_lists_are_box_segments_on_seeded_larger_geometries_and_the_bound_is_attained():
    from vbq_amd import bitstream
    rng = np.random.default_rng(20)
    attained = 0
    for _ in range(4000):
        dims = tuple(int(v) for v in rng.integers(1, 40, 3))
        seg = int(rng.choice([1, 2, 3, 7, 16, 64, 1024]))
        lo = tuple(int(rng.integers(0, d)) for d in dims)
        hi = tuple(int(rng.integers(l + 1, d + 1)) for l, d in zip(lo, dims))
        ext = tuple(h - l for l, h in zip(lo, hi))
        got = SR.box_list(dims, lo, ext, seg)
        assert got == bitstream.box_segments(dims, lo, hi, seg).tolist(), (dims, lo, hi, seg)
        bound = SR.max_listed_segments(dims, ext, seg)
        assert len(got) <= bound
        attained += len(got) == bound
    assert attained > 1000                      # the bound is met, not merely respected
    # and the package's own copy of the bound is this one
    from vbq_amd import store
    for _ in range(500):
        dims, ext = tuple(int(v) for v in rng.integers(1, 60, 3)), tuple(int(v) for v in rng.integers(0, 30, 3))
        seg = int(rng.integers(1, 80))
        assert store.max_listed_segments(dims, ext, seg) == SR.max_listed_segments(dims, ext, seg)


def test_file_dims_pads_on_the_left_and_merges_the_rest():
    from vbq_amd import store
    assert [store.file_dims(s) for s in ((37, 32), (1, 16, 48, 32), (2, 9, 23, 32), (2, 2, 5, 7, 32), (4,))] == \
        [(1, 1, 37), (1, 16, 48), (2, 9, 23), (4, 5, 7), (1, 1, 1)]


def test_the_validity_rule_at_its_edges():
    rng = np.random.default_rng(3)
    dims = [(2, 9, 23), (1, 16, 48)]
    table = SR.synthetic_table(dims, 8, 7, rng)
    broken = table.copy()
    broken[1, 1] += 1                                                   # n % (D1 D2) != 0
    ext = (1, 4, 5)
    ok = lambda f, o, t=table: SR.valid(t[f] if 0 <= f < 2 else t[0], 2, f, o, ext, 7) is not None
    assert ok(0, (0, 0, 0)) and ok(0, (1, 5, 18)) and ok(1, (0, 12, 43))             # a = D - w at every level
    assert not ok(0, (2, 5, 18)) and not ok(0, (1, 6, 18)) and not ok(0, (1, 5, 19))  # a = D - w + 1, level by level
    assert not ok(0, (-1, 0, 0)) and not ok(0, (0, 0, -1)) and not ok(0, (0, 1 << 62, 0)) and not ok(0, (1 << 62,) * 3)
    assert not ok(-1, (0, 0, 0)) and not ok(2, (0, 0, 0)) and not ok(1 << 40, (0, 0, 0))
    assert ok(0, (0, 0, 0), broken) and not ok(1, (0, 0, 0), broken)
    for bad in ((1, -5), (2, 0), (3, 0), (2, -3)):                                    # n < 0, D1 < 1, D2 < 1
        t = table.copy()
        t[0, bad[0]] = bad[1]
        assert not ok(0, (0, 0, 0), t)
    t = table.copy()
    t[0, 1:4] = (1 << 62, 1 << 32, 1 << 32)                                           # D1 D2 does not fit
    assert not ok(0, (0, 0, 0), t)
    t[0, 1:4] = ((1 << 31) * 7, 1, 7)                                                 # 2^31 segments of 7: one id too many
    assert SR.valid(t[0], 2, 0, (0, 0, 0), (1, 1, 1), 7) is None
    t[0, 1] -= 7
    assert SR.valid(t[0], 2, 0, (0, 0, 0), (1, 1, 1), 7) == (1 << 31) - 1
    # the restated call: an invalid sample is row 0 at origin 0, all -1, bit 7, and touches no neighbour
    ids = np.array([1, 5, 0], np.int64)
    origins = np.array([[0, 12, 43], [0, 0, 0], [1, 5, 18]], np.int64)
    n_sel = max(SR.max_listed_segments(d, ext, 7) for d in dims)
    desc, segs, status = SR.plan_boxes(table, ids, origins, ext, 7, n_sel)
    assert status.tolist() == [0, 128, 0] and (segs[1] == -1).all() and desc[1].tolist() == table[0].tolist()
    assert desc[0].tolist() == table[1, :4].tolist() + [0, 12, 43] + table[1, 7:].tolist()
    assert segs[2][segs[2] >= 0].tolist() == SR.box_list(dims[0], (1, 5, 18), ext, 7)
    short = SR.plan_boxes(table, ids[2:], origins[2:], ext, 7, int((segs[2] >= 0).sum()) - 1)
    assert short[2].tolist() == [32] and short[1][0].tolist() == segs[2][:short[1].shape[1]].tolist()
    assert SR.plan_boxes(table, ids, origins, (1, 0, 5), 7, n_sel) is None and SR.plan_boxes(table, ids, origins, ext, 7, 0) is None


# ------------------------------------------------------------------------------------------------------------------ the ABI
def _header_functions():
    """{name: [argument texts]} of vbq_amd/store/vbq_store.h."""
    s = strip_c(_read(HEADER))
    return {m.group(1): call_args(s, m.end() - 1) for m in re.finditer(r"\b(vbqs_[a-z0-9_]+)\s*\(", s)}


def test_header_carries_its_own_version_and_error_and_builds_on_vbq_h():
    assert set(_header_functions()) == {"vbqs_abi_version", "vbqs_last_error", WHO}
    text = _read(HEADER)
    assert '#include "vbq.h"' in text and "#define VBQS_ABI_VERSION 1" in text and "Planned boxes" in text
    assert not re.search(r"\bvbq[xbk]?_[a-z0-9_]+\s*\(", strip_c(text))       # it declares nothing of the other four libraries


def test_library_exports_exactly_the_header(store_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", store_lib], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r"\b[A-Za-z] (vbqs_[A-Za-z0-9_]+)", out)) == sorted(_header_functions())
    assert not re.search(r"\bvbq[xbk]?_", out) and "_Z" not in out, out


def test_the_new_tree_is_these_files_and_nothing_joined_the_first_library():
    from vbq_amd import build
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(STORE, "*")) if not p.endswith("__pycache__")) == \
        ["__init__.py", "vbq_store.h", "vbqs_api.hip", "vbqs_plan.hip"]
    assert [os.path.basename(s) for s in build.store_sources()] == ["vbqs_api.hip", "vbqs_plan.hip"]
    assert not [s for s in build.HIP_SOURCES if "store" in s or s.startswith("vbqs")]
    assert "vbqs_" not in _read(os.path.join(ROOT, "include", "vbq.h"))
    assert "vbq_amd/lib/vbq_store.flags.txt" in _read(os.path.join(ROOT, ".gitignore")).split()


def test_ctypes_binding_mirrors_the_header(hs):
    from vbq_amd import _lib_store
    declared = _header_functions()
    assert sorted(_lib_store.SIGNATURES) == sorted(declared)

    def ctype(arg):
        arg = " ".join(arg.split())
        if "*" in arg:
            return C.c_void_p
        return {"int64_t": C.c_int64, "int32_t": C.c_int32, "size_t": C.c_size_t}[arg.split(" ")[0]]
    text = strip_c(_read(HEADER))
    for name, args in declared.items():
        res, argtypes = _lib_store.SIGNATURES[name]
        assert argtypes == ([] if args == ["void"] else [ctype(a) for a in args]), name
        returns = re.search(r"([A-Za-z_][A-Za-z0-9_ ]*?\**)\s*" + name + r"\s*\(", text).group(1).split()
        assert res == (C.c_char_p if "char" in returns else C.c_int), name
    assert hs.vbqs_abi_version() == 1 == _lib_store.ABI_VERSION
    assert "torch.empty" not in _read(os.path.join(ROOT, "vbq_amd", "_lib_store.py")) and \
        "np.empty" not in _read(os.path.join(ROOT, "vbq_amd", "_lib_store.py"))


def test_missing_library_fails_loudly_also_at_the_import_of_the_subpackage(monkeypatch, tmp_path, store_lib):
    from vbq_amd import _lib, _lib_store
    import vbq_amd.store as real
    monkeypatch.setattr(_lib_store, "_LIB", None)
    monkeypatch.setenv("VBQ_STORE_LIBRARY", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.VBQError, match="not built"):
        _lib_store.lib()
    monkeypatch.delitem(sys.modules, "vbq_amd.store")
    try:
        with pytest.raises(_lib.VBQError, match="not built"):
            importlib.import_module("vbq_amd.store")
    finally:
        sys.modules.pop("vbq_amd.store", None)
        sys.modules["vbq_amd.store"] = real
        import vbq_amd
        vbq_amd.store = real
    monkeypatch.delenv("VBQ_STORE_LIBRARY")
    monkeypatch.setattr(_lib_store, "_LIB", None)
    assert _lib_store.lib() is not None
    import vbq_amd
    assert vbq_amd.LatentStore is real.LatentStore and "LatentStore" in vbq_amd.__all__


def test_a_current_library_without_an_object_cache_needs_no_compiler(store_lib, monkeypatch, tmp_path):
    """The tree as it arrives where objects are not shipped: library and flags tag, no vbq_amd/lib/obj/store."""
    import shutil
    from vbq_amd import build
    lib = tmp_path / "lib"
    lib.mkdir()
    for name in ("libvbq_store.so", "vbq_store.flags.txt"):
        shutil.copy2(os.path.join(build.LIBDIR, name), lib / name)
    monkeypatch.setattr(build, "LIBDIR", str(lib))
    monkeypatch.setattr(build, "STORE_LIB", str(lib / "libvbq_store.so"))
    monkeypatch.setattr(shutil, "which", lambda name: pytest.fail("looked for a compiler"))
    monkeypatch.setattr(build.subprocess, "run", lambda *a, **k: pytest.fail("started a process"))
    assert build.build_store() == str(lib / "libvbq_store.so") and not (lib / "obj").exists()
    flags = _read(os.path.join(str(lib), "vbq_store.flags.txt")).split()
    assert "-fvisibility=hidden" in flags and "-ffp-contract=off" in flags and "--offload-arch=gfx950" in flags


# ------------------------------------------------------------------------------------------------------------------ refusals
def _call(hs, **kw):
    """vbqs_plan_boxes with the address 16 for every pointer: nothing may read through them."""
    a = dict(table=16, n_files=3, fields=8, ids=16, origins=16, S=5, w0=1, w1=2, w2=3, seg=64, n_sel=4, desc=16, segs=16, status=16)
    a.update(kw)
    return hs.vbqs_plan_boxes(*[a[k] for k in ("table", "n_files", "fields", "ids", "origins", "S", "w0", "w1", "w2", "seg", "n_sel",
                                               "desc", "segs", "status")], None)


def test_the_c_call_refuses_before_any_device_work(hs):
    """On a host without a GPU: every refusal returns before anything could be launched, and names itself and the value."""
    def refused(rc, *texts):
        msg = hs.vbqs_last_error().decode()
        assert rc == INVALID and WHO in msg and all(t in msg for t in texts), (rc, msg)

    for fields in (0, 7, 9, 15, 17, 32):
        refused(_call(hs, fields=fields), f"fields={fields}")
    refused(_call(hs, n_files=0), "n_files=0")
    refused(_call(hs, S=-1), "S=-1")
    refused(_call(hs, w0=-1), "box=-1 x 2 x 3")
    refused(_call(hs, w1=-2), "box=1 x -2 x 3")
    refused(_call(hs, w2=-3), "box=1 x 2 x -3")
    refused(_call(hs, n_sel=-1), "n_sel=-1")
    for seg in (0, -1, 65534):
        refused(_call(hs, seg=seg), f"seg={seg}", "1..65533")
    for name in ("table", "ids", "origins", "desc", "segs", "status"):
        refused(_call(hs, **{name: None}), "null pointer")
    # nothing to do: nothing is launched (and on this host nothing could be)
    assert _call(hs, S=0) == 0 and _call(hs, w1=0) == 0 and _call(hs, n_sel=0) == 0
    refused(_call(hs, S=0, status=None), "null pointer")                    # the checks come before the early return


# ------------------------------------------------------------------------------------------------------------------ static rules
def _store_sources():
    files = {os.path.basename(p): _read(p) for p in sorted(glob.glob(os.path.join(STORE, "*.hip")) + glob.glob(os.path.join(STORE, "*.h")))}
    assert sorted(files) == ["vbq_store.h", "vbqs_api.hip", "vbqs_plan.hip"], sorted(files)
    return files


def test_the_native_tree_allocates_nothing_reads_no_environment_and_names_the_callers_stream():
    files = _store_sources()
    launches = 0
    for name, text in files.items():
        n, bad = launch_violations(text)
        launches += n
        assert not bad and n == len(re.findall(r"\bhipLaunchKernelGGL\b", strip_c(text))), (name, bad)
        assert async_violations(text)[1] == [], name
        assert stream_variable_violations(text)[1] == [], name
        assert forbidden_found(text) == [] and literal_stream_violations(text) == [], name
        s = strip_c(text)
        assert not re.search(r"\bhip(?:Ext)?(?:Malloc|HostAlloc|HostMalloc|HostRegister|MemAlloc)\w*\b|\bgetenv\b|\bprintf\s*\(|\bassert\s*\(|"
                             r"\batomic[A-Z]\w*\b", s), name
    assert launches == 1
    text = files["vbqs_plan.hip"]
    planted = text.replace("0, reinterpret_cast<hipStream_t>(stream),", "0, 0,")
    assert planted != text and launch_violations(planted)[1] and literal_stream_violations(planted)
    planted = text.replace("    VBQ_CHECK_LAUNCH(who);", "    hipDeviceSynchronize();\n    VBQ_CHECK_LAUNCH(who);")
    assert planted != text and forbidden_found(planted) == ["hipDeviceSynchronize"]
    # the refusals stand before the launch, the early return between them
    body = strip_c(text)
    body = body[body.index("int vbqs_plan_boxes"):]
    assert max(m.start() for m in re.finditer(r"VBQ_REQUIRE", body)) < body.index("return VBQ_OK") < body.index("hipLaunchKernelGGL")


def test_the_python_call_site_passes_the_tensors_stream_and_nothing_synchronises():
    """The rule of tests/test_stream_order_host.py reads names that start with `vbq_`: the fifth library's are spelled
    `vbq_s_...` for it, in the header and in the Python text alike."""
    spell = lambda text: text.replace("vbqs_", "vbq_s_")
    pos = stream_positions(spell(_read(HEADER)))
    assert pos == {spell(WHO): 14}
    text = spell(_read(os.path.join(STORE, "__init__.py")))
    seen, bad = python_site_violations(text, pos, "__init__.py")
    assert seen == 1 and not bad
    planted = text.replace("ops._stream(ids)), ", "None), ")
    assert planted != text and python_site_violations(planted, pos, "__init__.py")[1]
    # the first library's calls the store makes itself pass a tensor's stream too
    first = stream_positions(_read(os.path.join(ROOT, "include", "vbq.h")))
    seen, bad = python_site_violations(_read(os.path.join(STORE, "__init__.py")), first, "__init__.py")
    assert seen == 1 and not bad                                            # vbq_rans_segment_offsets_u16, once, at construction
    # crops itself: no read, no synchronisation -- check() and the constructor hold the only .cpu() calls of the class
    src = _read(os.path.join(STORE, "__init__.py"))
    crops = src[src.index("    def crops("):src.index("    def check(")]
    assert not re.search(r"\.cpu\(|\.item\(|\.tolist\(|synchronize|\.numpy\(", crops)
    for top in sorted(glob.glob(os.path.join(ROOT, "vbq_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py"))):
        if os.path.basename(top) not in ("_lib_store.py", "store_bench.py"):
            assert "vbqs_" not in _read(top), top                           # nothing that exists is routed through the store
