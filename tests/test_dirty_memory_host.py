"""tests/dirty_memory.py without a GPU: what Fill does, that four patched names are all the uninitialised memory there is, that the
tables name what exists, and the host-only paths under every fill.

Patching torch.empty / torch.empty_like / np.empty / np.empty_like is sufficient because of two facts held here: vbq_amd/*.py
creates uninitialised memory through these four spellings only, and the native trees allocate nothing.  A NEW SPELLING FAILS HERE:
teach tests/dirty_memory.py to fill it first.

Page-locked memory needs a device: where there is none, torch.empty(pin_memory=True) must raise under a fill exactly what it raises
without one (the argument is forwarded); tests/test_gpu_dirty_memory.py fills pinned and device tensors on the MI355X."""
import hashlib
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dirty_memory as DM  # noqa: E402
import footprint as FP  # noqa: E402
import quantizer_histories as QH  # noqa: E402

ROOT = os.path.dirname(DM.PACKAGE)
SHAPES = ((), (0,), (3, 5))


def _bytes_np(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _bytes_torch(t):
    return t.contiguous().reshape(-1).view(torch.uint8).numpy()


# ====================================================================================================== Fill
@pytest.mark.parametrize("byte", DM.FILLS + (0xA7,))
@pytest.mark.parametrize("dtype", list(FP._NP), ids=lambda d: str(d).split(".")[-1])
def test_fill_fills_all_four_spellings(dtype, byte):
    npd = FP._NP[dtype]
    for shape in SHAPES:
        n = int(np.prod(shape)) * np.dtype(npd).itemsize
        with DM.Fill(byte):
            got = [torch.empty(shape, dtype=dtype), torch.empty_like(torch.zeros(shape, dtype=dtype)),
                   torch.empty(shape, dtype=dtype).new_zeros(shape), np.empty(shape, npd), np.empty_like(np.zeros(shape, npd)),
                   np.empty(shape, dtype=npd, order="F")]
        assert not _bytes_torch(got[2]).any()                                   # nothing but the four names is patched
        for k in (0, 1):
            assert got[k].dtype == dtype and tuple(got[k].shape) == shape
            assert _bytes_torch(got[k]).tolist() == [byte] * n, (k, shape)
        for k in (3, 4, 5):
            assert got[k].dtype == npd and got[k].shape == shape
            assert _bytes_np(got[k]).tolist() == [byte] * n, (k, shape)


def test_fill_reads_as_the_docstring_tabulates():
    with DM.Fill(0x01):
        assert int(np.empty(1, np.uint16)[0]) == 257 and int(np.empty(1, np.int32)[0]) == 16843009
        f32, f64 = float(np.empty(1, np.float32)[0]), float(np.empty(1, np.float64)[0])
        assert abs(f32 / 2.37e-38 - 1) < 5e-3 and abs(f64 / 7.75e-304 - 1) < 5e-3
    with DM.Fill(0x3C):
        assert int(np.empty(1, np.uint16)[0]) == 15420 and int(np.empty(1, np.int32)[0]) == 1010580540
        f32, f64 = float(torch.empty(1)[0]), float(torch.empty(1, dtype=torch.float64)[0])
        assert abs(f32 / 0.01149 - 1) < 5e-3 and abs(f64 / 1.53e-18 - 1) < 5e-3
    for byte in DM.FILLS[1:]:
        for npd in FP._NP.values():
            v = DM._scalar(byte, npd)
            assert np.isfinite(v) and v > 0, (byte, npd)


def test_fill_forwards_out_and_other_arguments_and_permuted_prototypes():
    with DM.Fill(0x3C):
        given = torch.zeros(6, dtype=torch.int32)
        assert torch.empty(6, out=given) is given and given.tolist() == [1010580540] * 6
        proto = torch.zeros((4, 3, 2), dtype=torch.float32).permute(2, 0, 1)
        like = torch.empty_like(proto)
        assert like.stride() == proto.stride() and _bytes_torch(like).tolist() == [0x3C] * 96
        assert torch.empty_like(proto, dtype=torch.int16, memory_format=torch.contiguous_format).is_contiguous()
        nproto = np.zeros((4, 3, 2), np.float64).transpose(2, 0, 1)
        nlike = np.empty_like(nproto)
        assert nlike.strides == nproto.strides and _bytes_np(nlike).tolist() == [0x3C] * 192
        assert np.empty_like(nproto, dtype=np.uint16, shape=(5,)).tolist() == [15420] * 5
        table = np.empty(3, dtype=np.dtype([("a", np.uint8), ("b", np.float64)], align=True))     # padding bytes too
        assert table.view(np.uint8).tolist() == [0x3C] * table.nbytes


def test_fill_with_page_locked_memory():
    def pinned():
        return torch.empty((3, 5), dtype=torch.float32, pin_memory=True)
    if torch.cuda.is_available():
        with DM.Fill(0x01):
            t = pinned()
        assert t.is_pinned() and _bytes_torch(t).tolist() == [0x01] * 60
        return
    with pytest.raises(RuntimeError) as plain:
        pinned()
    with DM.Fill(0x01), pytest.raises(RuntimeError) as filled:
        pinned()
    assert str(filled.value) == str(plain.value)


def test_fill_restores_the_names_and_patches_nothing_else():
    names = lambda: (torch.empty, torch.empty_like, np.empty, np.empty_like)
    others = lambda: (torch.zeros, torch.zeros_like, torch.full, np.zeros, np.zeros_like, np.full, np.ndarray)
    before, rest = names(), others()
    with DM.Fill(0x01):
        assert all(a is not b for a, b in zip(names(), before)) and others() == rest
        assert torch.zeros(3).tolist() == [0, 0, 0] and np.zeros(3).tolist() == [0, 0, 0]
    assert names() == before
    with pytest.raises(KeyError):
        with DM.Fill(0x3C):
            raise KeyError("inside")
    assert names() == before and others() == rest
    with DM.Fill(0x01):
        with pytest.raises(AssertionError):
            DM.Fill(0x3C).__enter__()
    assert names() == before


def test_fill_logs_the_callers_site_under_the_package_only():
    from vbq_amd import coder, tables
    before = DM.sites_reached()
    coder.quantize_frequencies(np.ones((2, 31)))
    assert DM.sites_reached() == before                                          # nothing is logged without a fill
    with DM.Fill(0x01):
        np.empty(3)                                                              # this file is not under vbq_amd/
        coder.quantize_frequencies(np.ones((2, 31)))
        coder.quantize_frequencies(np.ones((0, 31)))
    assert ("coder.py", 38) in DM.sites_reached() and not {s for s in DM.sites_reached() if not s[0].endswith(".py")}
    assert all(s in DM.allocation_sites() for s in DM.sites_reached())
    assert tables.__file__.startswith(DM.PACKAGE)


def test_a_call_that_spans_lines_is_one_site_on_its_first_line(tmp_path):
    src = tmp_path / "spans.py"
    src.write_text("import numpy as np\nimport torch\n\n\ndef f():\n    return np.empty((2,\n                     3),\n"
                   "                    np.float32), torch.empty_like(\n        torch.zeros(2))\n")
    assert DM._calls(str(src)) == [(6, 8), (8, 9)]


def test_first_difference_names_the_leaf_and_the_element():
    a = (b"abc", (np.arange(6, dtype=np.float32).reshape(2, 3), 7))
    b = (b"abc", (np.arange(6, dtype=np.float32).reshape(2, 3), 7))
    assert DM.first_difference(a, b) is None and QH.same(a, b)
    b[1][0][1, 2] = -0.0 + 9
    assert DM.first_difference(a, b).startswith("answer[1][0][1, 2]: 5.0 against 9.0 (1 of 6")
    assert "answer[1][1]: 7 against 8" in DM.first_difference(a, (b"abc", (a[1][0], 8)))
    assert "position 2" in DM.first_difference((b"abc",), (b"abd",))
    assert DM.first_difference((np.zeros(2, np.float32),), (np.zeros(2, np.float64),)) is not None
    z = (np.array([0.0, np.nan], np.float32),)
    assert DM.first_difference(z, (np.array([-0.0, np.nan], np.float32),)).startswith("answer[0][0]")


# ====================================================================================================== the spellings
OTHER_SPELLINGS = (r"\bnew_empty\b", r"\bempty_strided\b", r"\bresize_\b", r"\btorch\.Tensor\(", r"\bnp\.ndarray\(",
                   r"\bnumpy\.ndarray\(", r"\bbytearray\(", r"\btorch\.(Float|Double|Int|Long|Byte|Short|Half)Tensor\(",
                   r"\bnp\.(recarray|memmap)\(", r"\bnew_tensor\b\(\s*\)", r"\.new\(")
NATIVE_ALLOCATIONS = re.compile(r"\bhip(Ext)?(Host)?Malloc\w*|\bhipMemAllocHost\b|\bhipMallocManaged\b|\bhipHostAlloc\b")
NATIVE_TREES = ("vbq_amd/csrc", "vbq_amd/ext", "vbq_amd/budget", "vbq_amd/kmeans", "include")


def test_python_sources_allocate_through_the_four_spellings_only():
    """No bytearray(...) at all: the writers build their files from NumPy arrays and bytes, so none can be uploaded or written."""
    found = []
    for name, path in DM.source_files().items():
        with open(path, encoding="utf-8") as f:
            for k, line in enumerate(f, 1):
                found += [f"vbq_amd/{name}:{k}: {line.strip()}" for pat in OTHER_SPELLINGS if re.search(pat, line)]
    assert not found, f"uninitialised memory that {DM.HELPER} does not fill -- teach Fill this spelling first:\n" + "\n".join(found)
    # the aliases under which the four spellings are reached: `import numpy as np`, `import torch`, nothing imported by name
    for name, path in DM.source_files().items():
        with open(path, encoding="utf-8") as f:
            text = f.read()
        assert not re.search(r"from\s+(numpy|torch)\s+import\s+[^\n]*\bempty", text), f"vbq_amd/{name}: empty imported by name ({DM.HELPER})"
        assert not re.search(r"import\s+numpy\s+as\s+(?!np\b)|import\s+torch\s+as\s+", text), f"vbq_amd/{name}: another alias ({DM.HELPER})"
        assert len(re.findall(r"\b(?:np|torch)\.empty(?:_like)?\(", text)) == len(DM._calls(path)), name


def test_native_trees_allocate_nothing():
    found = []
    for tree in NATIVE_TREES:
        for base, _, files in os.walk(os.path.join(ROOT, tree)):
            for fn in files:
                if fn.endswith((".hip", ".h", ".hpp", ".cpp", ".c", ".inc")):
                    with open(os.path.join(base, fn), encoding="utf-8", errors="replace") as f:
                        for k, line in enumerate(f, 1):
                            if NATIVE_ALLOCATIONS.search(line):
                                found.append(f"{os.path.relpath(os.path.join(base, fn), ROOT)}:{k}: {line.strip()}")
    assert not found, f"a native allocation is memory {DM.HELPER} cannot fill:\n" + "\n".join(found)
    assert all(os.path.isdir(os.path.join(ROOT, t)) for t in NATIVE_TREES)


def test_the_static_list_sees_every_site():
    sites = DM.allocation_sites()
    assert len(sites) >= 100 and not any(f == "build.py" for f, _ in sites)
    for f, line in (("pipeline.py", 273), ("coder.py", 282), ("embeddings.py", 268), ("quantizer.py", 856), ("quantizer.py", 899)):
        assert (f, line) in sites, (f, line)


# ====================================================================================================== the tables
def test_tables_name_what_exists():
    import ast
    sites = DM.allocation_sites()
    for site, reason in DM.EXEMPT_SITES.items():
        assert site in sites, f"{site} is no allocation site (any more)"
        assert reason in DM.EXEMPT_REASONS or (reason.startswith(DM.HOST_ONLY) and reason[len(DM.HOST_ONLY):] in globals()), reason
    with open(os.path.join(os.path.dirname(__file__), "test_gpu_dirty_memory.py"), encoding="utf-8") as f:
        tree = ast.parse(f.read())
    # the calls of section c register themselves by name: @call("<name>")
    registered = {d.args[0].value for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) for d in n.decorator_list
                  if isinstance(d, ast.Call) and getattr(d.func, "id", "") == "call" and d.args and isinstance(d.args[0], ast.Constant)}
    src = open(os.path.join(os.path.dirname(__file__), "test_gpu_stream_order.py"), encoding="utf-8").read()
    cases = set(re.findall(r'^@case\("([^"]+)"', src, re.M))
    for name, sentences in DM.UNSPECIFIED.items():
        assert name in QH.PROBES or name in cases or name in registered, f"{name} is no probe, case or call"
        assert sentences, f"{name}: an entry without a sentence is a finding, not an entry"
        for where, quoted in sentences:
            with open(os.path.join(ROOT, where), encoding="utf-8") as f:
                text = re.sub(r"\s*\n\s*(\*\s*)?", " ", f.read())
            assert quoted in text, f"{name}: {where} does not say {quoted!r}"


# ====================================================================================================== host-only paths
def test_host_only_paths_under_every_fill():
    """The writers of the three pinned files of tests/test_bitstream_host.py, tables.level_major_to_sorted and
    coder.quantize_frequencies (coder.py:38) answer under every fill as they do without one, and pipeline.numpy_log2_f32_loop
    (which checks the library's host routine against NumPy in a buffer of its own, once per process) reaches the same verdict.
    (The xi-space encoder of utils.py:179-218 launches kernels: it is a call of tests/test_gpu_dirty_memory.py.)"""
    import test_bitstream_host as TBH
    from vbq_amd import coder, pipeline, tables
    rng = np.random.default_rng(4)
    table = np.sort(rng.normal(0, 1, (3, 31)).astype(np.float32), axis=1)
    counts = rng.integers(0, 40, (2, 3, 31))
    counts[1, 2] = 0
    counts[0, 1, 5] = 10 ** 6

    def answer():
        files = tuple(build()[-1] for build in (TBH._pinned_segments, TBH._pinned_compact, TBH._pinned_embeddings))
        pipeline._LOG2_LOOP = None                                               # the verdict is kept: ask again
        loop = pipeline.numpy_log2_f32_loop()
        return files + (loop is not None, tables.level_major_to_sorted(table), coder.quantize_frequencies(counts), coder.quantize_frequencies(counts, 0.5))
    want = QH._plain(answer())
    for data, name in zip(want[:3], ("segments", "compact", "embeddings")):
        assert (len(data), hashlib.blake2b(data, digest_size=16).hexdigest()) == TBH.PINNED[name]
    for byte in DM.FILLS:
        with DM.Fill(byte):
            got = QH._plain(answer())
        assert QH.same(got, want), f"fill 0x{byte:02X}: {DM.first_difference(got, want)}"
    assert want[3] is True, "the library's host routine did not reproduce NumPy's float32 log2"
    assert {("coder.py", 38), ("tables.py", 42), ("pipeline.py", 166)} <= DM.sites_reached()
