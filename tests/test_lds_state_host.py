"""tests/lds_state.py without a GPU: the catalogue against a scan of the sources, the scan against hand-made sources, the table
of what a fill reads as, the cross-compile of the test library, and the wrapper that pollutes a call."""
import os
import re

import numpy as np
import pytest

import dirty_memory as DM
import lds_state as LS


def test_every_kernel_with_shared_storage_is_covered_or_exempt():
    scan = LS.kernels()
    assert "k_hist_flat" in scan and "k_prep_planes" in scan                              # (k_prep_planes: through transpose_tile)
    both = set(LS.COVERED) & set(LS.EXEMPT)
    assert not both, f"in COVERED and in EXEMPT: {sorted(both)}"
    missing = sorted(set(scan) - set(LS.COVERED) - set(LS.EXEMPT))
    assert not missing, "kernels with __shared__ storage that stand in neither lds_state.COVERED nor lds_state.EXEMPT (add a case to " \
                        "tests/test_gpu_lds_state.py and list it in COVERED):\n" + "\n".join(f"{k} ({scan[k]})" for k in missing)
    gone = sorted((set(LS.COVERED) | set(LS.EXEMPT)) - set(scan))
    assert not gone, f"catalogued, but no kernel with __shared__ storage of that name exists: {gone}"
    assert all(cases and len(set(cases)) == len(cases) for cases in LS.COVERED.values())


def test_exemptions_give_one_of_the_three_reasons():
    assert LS.EXEMPT_REASONS == ("multi-GPU only", "reached only by inputs above ", "never the first LDS-using launch of any entry point: ")
    for kernel, reason in LS.EXEMPT.items():
        assert reason == LS.MULTI_GPU or any(reason.startswith(r) and len(reason) > len(r) for r in LS.EXEMPT_REASONS[1:]), (kernel, reason)
    scan = LS.kernels()
    for kernel, reason in LS.EXEMPT.items():
        if reason.startswith(LS.NEVER_FIRST):                      # the launch named before it: a catalogued kernel of the same file
            first = re.match(r"(k_\w+) \((\w+)\)", reason[len(LS.NEVER_FIRST):])
            assert first and first.group(1) in LS.COVERED and scan[first.group(1)] == scan[kernel], (kernel, reason)
            with open(os.path.join(LS.ROOT, scan[kernel]), encoding="utf-8") as f:
                text = f.read()
            entry = text[text.index('extern "C" int ' + first.group(2)):]
            a, b = entry.index("hipLaunchKernelGGL(" + first.group(1)), entry.index("hipLaunchKernelGGL(" + kernel)
            assert a < b and "extern \"C\"" not in entry[1:b], (kernel, "is not launched after", first.group(1))


def test_every_catalogued_case_is_a_case_of_the_gpu_module():
    """Without importing the module (it needs torch; its own test_the_cases_are_the_catalogue compares the pairs): every case
    COVERED names is registered there with @case("<name>", ...)."""
    with open(os.path.join(LS.ROOT, "tests", "test_gpu_lds_state.py"), encoding="utf-8") as f:
        registered = set(re.findall(r'^@case\("(\w+)"', f.read(), flags=re.M))
    listed = {c for cases in LS.COVERED.values() for c in cases}
    assert listed == registered, sorted(listed ^ registered)


# ---- the routes tests/launch_plans.py states for the cases of the GPU module
def _src(rel):
    with open(os.path.join(LS.ROOT, "vbq_amd", "csrc", rel), encoding="utf-8") as f:
        return f.read()


def test_route_constants_match_the_sources():
    import launch_plans as LP
    nb, red = _src("vbq_notebook.hip"), _src("vbq_reduce.hip")
    const = lambda text, name: int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))
    assert const(nb, "kMaxBetaChunk") == LP.NB_MAX_BETA_CHUNK and const(nb, "kNbKeys") == LP.NB_KEYS
    assert const(nb, "kNbKeyShift") == LP.NB_KEY_SHIFT and const(red, "kNpBlock") == LP.NP_BLOCK
    assert f"nonneg && Lc <= {LP.NB_PRUNED_MAX_L})" in nb and f"fast_ok && N == 10 && Lc >= {LP.NB_HULL_MIN_L})" in nb
    assert "bc.beta[i] >= 1e-12 && bc.beta[i] <= 1e18" in nb and LP.NB_FAST_RANGE == (1e-12, 1e18)
    assert "build_sweep_table<kNbKeyShift>(b, Lc, 2e-12f, 2e18f, sw)" in nb and LP.NB_SWEEP_RANGE == (2e-12, 2e18)
    assert "b[i] = (float)(2.0 * betas[i]);" in nb
    assert "const int64_t nfull = n / kNpBlock;" in red and "if (nfull > 0) {" in red
    tr = _src("vbq_transpose.hip")
    assert "const bool vec = rows % V == 0 && cols % V == 0 &&" in tr and "const bool v4 = n_rows % 4 == 0 && n_cols % 4 == 0 &&" in tr
    assert "if (n_ch > 1 && layout != out_layout) {" in _src("vbq_latents.hip")


def test_routes_worked_examples():
    import launch_plans as LP
    from oracle import notebook_cases as NC
    nk = LP.notebook_kernel
    assert [nk(10, b) for b in ([0.7], [0.0], [0.02, 30.0], [1e-13, 1e19])] == ["pruned<1>", "pruned<1>", "pruned<2>", "pruned<2>"]
    assert [nk(10, b) for b in ([-1e4], [3.0, -0.5], NC.log_sweep(12) + [1e-13, 1e19])] == ["literal"] * 3
    assert [nk(10, NC.log_sweep(L)) for L in (3, 5, 6, 33, 64)] == ["fast", "fast", "hull", "hull", "hull"] and nk(10, NC.NB50) == "hull"
    assert nk(9, NC.log_sweep(50)) == "fast"                                           # the threshold kernel is built for N = 10
    # what build_sweep_table refuses: too short, a repeated value, two betas in one bucket, more than 24 octaves
    for sweep in (NC.NB50[:5], [1.0, 1.0, 2.0, 3.0, 5.0, 9.0, 17.0], [1.0, 1.0 + 2.0 ** -9, 2.0, 4.0, 8.0, 16.0],
                  [1e-7, 1e-3, 1.0, 1e3, 1e6, 1e9, 1e12]):
        assert nk(10, sweep) == "fast", sweep
    assert LP.sweep_table_ok([1.0, 2.0], 64, 17, 1536, 2e-12, 2e18) and not LP.sweep_table_ok([], 64, 17, 1536, 2e-12, 2e18)
    tk = LP.transpose_kernel
    assert [tk(68, 132, 4), tk(68, 132, 2), tk(8, 72, 2), tk(63, 65, 4), tk(64, 64, 2, aligned=False)] == \
        ["vec", "scalar", "vec", "scalar", "scalar"]
    assert LP.gather_kernel(1, 0, 1) == "k_gather" and LP.gather_kernel(3, 0, 1) == "k_gather_transpose" == LP.gather_kernel(3, 1, 0)
    assert [LP.np_sums_first_kernel(n) for n in (1, 8191, 8192)] == ["k_np_finish", "k_np_finish", "k_np_block_sums"]


SOURCES = {
    "a.hip": """
        // __global__ void in_a_comment() { __shared__ int x; }
        template <typename T> __device__ __forceinline__ void stage(T *p) { __shared__ T tile[64][65]; tile[0][0] = *p; }
        __device__ void through(float *p) { stage<float>(p); }
        __device__ int plain(int a) { return a + 1; }
        __global__ void __launch_bounds__(256) k_static(float *p) { __shared__ float s[4]; s[0] = *p; }
        template <int N>
        __global__ void __launch_bounds__(N * 64)
        k_extern(float *p) { extern __shared__ __align__(16) unsigned char smem[]; }
        __global__ void k_calls(float *p) { through(p); }
        __global__ void k_none(float *p) { *p = plain(1); }
        __global__ void k_declared(float *p);
    """,
    "b.h": "__global__ void k_header(int *p) { /* __shared__ */ stage<int>(p); }",
}


def test_the_scan_on_hand_made_sources():
    assert LS.kernels(SOURCES) == {"k_static": "a.hip", "k_extern": "a.hip", "k_calls": "a.hip", "k_header": "b.h"}
    assert [n for _, n, _ in LS.functions(SOURCES["a.hip"])] == ["stage", "through", "plain", "k_static", "k_extern", "k_calls", "k_none"]


def test_the_scan_sees_every_file_that_declares_shared_storage():
    files = {rel for rel in LS.source_files() if "__shared__" in LS._strip_c(open(os.path.join(LS.ROOT, rel), encoding="utf-8").read())}
    assert files and files == set(LS.kernels().values()), sorted(files ^ set(LS.kernels().values()))
    declared = sum(len(re.findall(r"__shared__", LS._strip_c(open(os.path.join(LS.ROOT, rel), encoding="utf-8").read()))) for rel in files)
    inside = sum(len(re.findall(r"__shared__", body)) for rel in files
                 for _, _, body in LS.functions(open(os.path.join(LS.ROOT, rel), encoding="utf-8").read()))
    assert declared == inside, "a __shared__ declaration stands outside every function the scan found"


def test_what_each_fill_reads_as():
    assert LS.FILLS == DM.FILLS == (0x00, 0x01, 0x3C)
    types = {"u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64, "f32": np.float32, "f64": np.float64}
    for byte in LS.FILLS:
        for name, dt in types.items():
            got = np.frombuffer(bytes([byte]) * np.dtype(dt).itemsize, dt)[0]
            assert got == dt(LS.READS_AS[byte][name]), (hex(byte), name, got)
            assert np.isfinite(got) and got >= 0 and (byte == 0) == (got == 0)
        assert LS.toy_sum(byte) == (256 * int(np.frombuffer(bytes([byte]) * 4, np.uint32)[0])) % 2 ** 32
    doc = LS.__doc__
    for text in ("16 843 009", "1 010 580 540", "15 420", "2.37e-38", "0.01149", "1.53e-18", "7.75e-304"):
        assert text in doc
    assert len({LS.toy_sum(b) for b in LS.FILLS}) == 3


def test_the_fill_library_cross_compiles_for_gfx950(tmp_path):
    import ctypes as C
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.fail("hipcc not found: the test library of tests/lds_fill.hip cannot be compiled")
    lib = LS.compile_library(str(tmp_path))
    assert os.path.dirname(lib) == str(tmp_path) and os.path.getsize(lib) > 0
    with open(lib, "rb") as f:
        blob = f.read()
    for name in LS.SIGNATURES:
        assert name.encode() in blob
    assert b"gfx950" in blob
    src = open(LS.SOURCE, encoding="utf-8").read()
    consts = {k: int(eval(v)) for k, v in re.findall(r"constexpr int (k\w+) = ([^;]+);", src) if "k" not in v}
    assert consts["kLdsBytes"] == LS.LDS_BYTES and consts["kToyWords"] == LS.TOY_WORDS and consts["kThreads"] == 256
    assert "while (" not in LS._strip_c(src) and "kHoldCap" in src              # the hold is a counted loop
    # the same limits the product kernels take a whole CU's LDS by
    for rel in ("vbq_amd/csrc/vbq_budget.hip", "vbq_amd/kmeans/vbqk_dp.hip"):
        assert "160 * 1024" in open(os.path.join(LS.ROOT, rel), encoding="utf-8").read()


def test_stream_entries_are_the_calls_that_take_a_stream():
    import ctypes as C
    import importlib
    got = LS.stream_entries()
    assert set(got) == set(LS._LIBRARIES)
    for module, names in got.items():
        sig = importlib.import_module("vbq_amd." + module).SIGNATURES
        for name in names:
            assert sig[name][1][-1] is C.c_void_p, name
    assert "vbq_histogram_u16" in got["_lib"] and "vbqb_budget_sweep_f64" in got["_lib_budget"]
    assert not [n for names in got.values() for n in names if "workspace_bytes" in n or "host" in n or "comm" in n or "allreduce" in n]


class _Handle:
    def __init__(self):
        self.log = []

    def vbq_histogram_u16(self, *args):
        self.log.append(("real", args))
        return 0


def test_polluted_wraps_and_restores(monkeypatch):
    """The wrapper with a stand-in handle and a stand-in fill: the fill comes first, on the call's last argument; the function
    is put back on exit, also on an exception."""
    import importlib
    h, fills = _Handle(), []
    real = h.vbq_histogram_u16
    monkeypatch.setattr(LS, "stream_entries", lambda: {"_lib": ["vbq_histogram_u16"]})
    monkeypatch.setattr(importlib.import_module("vbq_amd._lib"), "lib", lambda: h)
    monkeypatch.setattr(LS, "pollute", lambda byte, stream: (fills.append((byte, stream)), h.log.append(("fill", byte))))
    with LS.Polluted(0x3C) as p:
        assert h.vbq_histogram_u16(1, 2, "stream") == 0
        with pytest.raises(AssertionError, match="already active"):
            LS.Polluted(0x01).__enter__()
    assert p.calls == {"vbq_histogram_u16": 1} and fills == [(0x3C, "stream")]
    assert [k for k, _ in h.log] == ["fill", "real"] and h.vbq_histogram_u16 == real
    with LS.Polluted(None) as p:
        h.vbq_histogram_u16(7)
    assert p.calls == {"vbq_histogram_u16": 1} and len(fills) == 1
    with pytest.raises(RuntimeError):
        with LS.Polluted(0x01):
            raise RuntimeError("inside")
    assert h.vbq_histogram_u16 == real and LS.Polluted._active is None


def test_bitmaps():
    bits = np.zeros(LS.SEEN_WORDS, np.int32)
    for i in (0, 31, 32, 4095):
        bits.view(np.uint32)[i >> 5] |= np.uint32(1 << (i & 31))
    assert LS.cus_of(bits) == {0, 31, 32, 4095}
