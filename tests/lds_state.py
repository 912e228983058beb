"""No kernel's answer depends on what the LDS held: the fill, the pollution of a call, the scan of the sources and the catalogue.

The LDS is not cleared between the dispatches of a process: a workgroup starts on what the last workgroup on its CU left there.
A kernel that clears its counters on the flush and skips its first clear, one that zeroes only the bins it later reads, one that
reads an entry past what it staged -- each is bit-exact in a process where the same kernel ran last on that CU (a graph replay is
such a process), and whether it fails a test depends on which test ran before and where the workgroup landed.  The most
forgiving content of the LDS is the kernel's own clean leftovers, as zero is the most forgiving content of fresh memory
(tests/dirty_memory.py); here it is made deterministic and hostile instead.

THE FILL.  tests/lds_fill.hip is a test-only library (compiled by `compile_library()` into a temporary directory with the compiler
flags of vbq_amd/build.py; no part of vbq_amd and no product library).  lds_fill(byte) runs workgroups that take ALL 160 KiB of a CU as
dynamic LDS -- one fits a CU -- store `byte` into every LDS byte, OR their CU's identity (XCC id, SE / SH / CU fields of the
hardware id register) into a bitmap and keep the CU for HOLD_TICKS of the 100 MHz clock, so that a grid of GRID_FACTOR x the CU
count reaches every CU.  lds_probe counts, per workgroup and before writing anything, the LDS bytes equal to a byte; lds_toy is a
deliberately wrong kernel that sums 1 KiB of LDS it never wrote (the sensitivity control).  No workgroup waits for another.

    byte   u8    u16     i32 / u32      i64 / u64      f32         f64
    0x00   0     0       0              0              0.0         0.0
    0x01   1     257     16 843 009     7.23e16        2.37e-38    7.75e-304
    0x3C   60    15 420  1 010 580 540  4.34e18        0.01149     1.53e-18

FILLS are those of tests/dirty_memory.py, for its reason: finite, positive, no NaN, not all-ones, no canary -- a dependence on
old LDS shows as a wrong value, not as a wild index.  0x00 is the forgiving baseline, kept so that a failure can say "differs
from a zeroed LDS".

POLLUTING A CALL.  `pollute(byte, stream)` enqueues the fill on a stream and keeps its bitmap; `Polluted(byte)` wraps every C
entry point of the five libraries that takes a stream, so that every call of one is preceded, on the stream the call itself was
given (its last argument), by a fill -- nothing else runs between the fill and the entry point's first launch.
`assert_covered()` reads the bitmaps of every fill since the last check -- after the case's own readback, so nothing synchronises
before the call -- and asserts that each holds `multi_processor_count` distinct CUs: every use of the fill proves its own
coverage.

THE CATALOGUE.  `kernels()` reads every __global__ kernel of vbq_amd/csrc, ext/, budget/, kmeans/ and store/ that declares
__shared__ storage, static or extern, itself or through a device function it calls (a source scan, as tests/written_buffers.py
reads the headers).  Each stands in COVERED (kernel -> the cases of tests/test_gpu_lds_state.py that launch it FIRST in an entry
point) or in EXEMPT with one of EXEMPT_REASONS.  A NEW KERNEL WITH __shared__ STORAGE GOES INTO COVERED WITH A CASE OF THE GPU
MODULE; tests/test_lds_state_host.py fails when the scan and the two tables disagree, the GPU module when its cases and COVERED
do.  Importable without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

FILLS = (0x00, 0x01, 0x3C)
READS_AS = {
    # byte -> what an element of each type reads as in a filled LDS (the table above; the host test recomputes it)
    0x00: {"u8": 0, "u16": 0, "u32": 0, "u64": 0, "f32": 0.0, "f64": 0.0},
    0x01: {"u8": 1, "u16": 257, "u32": 16843009, "u64": 72340172838076673, "f32": 2.3694278276172396e-38, "f64": 7.748604185489348e-304},
    0x3C: {"u8": 60, "u16": 15420, "u32": 1010580540, "u64": 4340410370284600380, "f32": 0.01148897036910057, "f64": 1.5306383611560062e-18},
}

LDS_BYTES = 160 * 1024          # kLdsBytes of tests/lds_fill.hip: the LDS of one CU
SEEN_WORDS = 128                # 4096 CU identities: XCC_ID[3:0] above HW_ID[15:8]
TOY_WORDS = 256                 # kToyWords: lds_toy sums 1 KiB
# The two tuned numbers (EXPERIMENTS.md, "LDS carry-over"): on an MI355X (256 CUs) every pair tried, from one workgroup per CU
# with no hold upwards, covered all 256 CUs in five fills out of five -- storing 160 KiB keeps a workgroup on its CU for some
# 25 us, longer than the dispatcher needs to place the grid.  The grid is the two per CU the design asks for; the hold is the
# smallest non-zero one tried, kept as a margin.  One fill then takes 36 us (32 us with no hold, 71 us with 2000 ticks).
GRID_FACTOR = 2                 # workgroups of a fill or a probe per CU
HOLD_TICKS = 250                # 100 MHz ticks (2.5 us) a workgroup keeps its CU after filling it

_TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_TESTS)
SOURCE = os.path.join(_TESTS, "lds_fill.hip")
SIGNATURES = {
    "lds_fill": [C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p],
    "lds_probe": [C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p],
    "lds_toy": [C.c_int, C.c_void_p, C.c_void_p],
}


# ------------------------------------------------------------------------------------------------------------------ the library
def compile_library(directory):
    """tests/lds_fill.hip -> <directory>/liblds_fill.so for gfx950, with vbq_amd.build's flags; needs hipcc, no GPU."""
    import shutil

    from vbq_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    obj, lib = os.path.join(directory, "lds_fill.o"), os.path.join(directory, "liblds_fill.so")
    build._compile_one(hipcc, SOURCE, obj, [], build.HIPCC_FLAGS)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", obj, "-o", lib], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("link of liblds_fill.so failed:\n" + r.stdout + r.stderr)
    return lib


_LIB = None
_PENDING = []                   # (byte, bitmap tensor) of every fill since the last assert_covered()


def load(path):
    """The module fixture of the GPU tests compiles the library and hands it over here."""
    global _LIB
    h = C.CDLL(path)
    for name, args in SIGNATURES.items():
        fn = getattr(h, name)
        fn.restype, fn.argtypes = C.c_int, args
    _LIB = h
    return h


def cu_count():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _raw(stream):
    """A stream as the integer a C entry point takes: a torch stream, a ctypes pointer, an integer or None (the null stream)."""
    if stream is None:
        return 0
    if isinstance(stream, C.c_void_p):
        return stream.value or 0
    return int(getattr(stream, "cuda_stream", stream))


def _on(stream_raw):
    import torch
    return torch.cuda.ExternalStream(stream_raw) if stream_raw else torch.cuda.default_stream()


def pollute(byte, stream=None, hold_ticks=None, grid_factor=None):
    """Enqueue lds_fill(byte) on `stream` (default: torch's current one); the bitmap is kept for assert_covered()."""
    import torch
    assert _LIB is not None, "lds_state.load() has not been called"
    raw = _raw(torch.cuda.current_stream() if stream is None else stream)
    with torch.cuda.stream(_on(raw)):
        seen = torch.zeros(SEEN_WORDS, dtype=torch.int32, device="cuda")           # (zeroed on the same stream, before the fill)
    grid = (GRID_FACTOR if grid_factor is None else grid_factor) * cu_count()
    e = _LIB.lds_fill(int(byte), grid, HOLD_TICKS if hold_ticks is None else int(hold_ticks), C.c_void_p(seen.data_ptr()), C.c_void_p(raw))
    assert e == 0, f"lds_fill: hipError {e}"
    _PENDING.append((int(byte), seen))
    return seen


def cus_of(bitmap):
    """The set of CU identities a bitmap (or a list of identities) holds."""
    bits = np.unpackbits(np.ascontiguousarray(bitmap).view(np.uint8), bitorder="little")
    return set(int(i) for i in np.flatnonzero(bits))


def assert_covered():
    """Every fill since the last call reached every CU of the device -> how many fills that were."""
    import torch
    torch.cuda.synchronize()
    pending, want = list(_PENDING), cu_count()
    del _PENDING[:]
    for k, (byte, seen) in enumerate(pending):
        got = len(cus_of(seen.cpu().numpy()))
        assert got == want, f"fill {k} of {len(pending)} (0x{byte:02X}) reached {got} of {want} CUs: the hold is too short or the " \
                            f"grid too small (lds_state.HOLD_TICKS, GRID_FACTOR)"
    return len(pending)


def probe(byte, stream=None):
    """lds_probe -> (CU identity u32 [grid], bytes equal to `byte` u32 [grid]) of every workgroup; synchronises."""
    import torch
    raw = _raw(torch.cuda.current_stream() if stream is None else stream)
    grid = GRID_FACTOR * cu_count()
    with torch.cuda.stream(_on(raw)):
        out = torch.zeros((grid, 2), dtype=torch.int32, device="cuda")
    e = _LIB.lds_probe(int(byte), grid, HOLD_TICKS, C.c_void_p(out.data_ptr()), C.c_void_p(raw))
    assert e == 0, f"lds_probe: hipError {e}"
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    return got[:, 0].copy(), got[:, 1].copy()


def toy(stream=None, grid=None):
    """lds_toy -> u32 [grid] device tensor: per workgroup the sum (mod 2^32) of 256 LDS words it never wrote."""
    import torch
    raw = _raw(torch.cuda.current_stream() if stream is None else stream)
    grid = cu_count() if grid is None else grid
    with torch.cuda.stream(_on(raw)):
        out = torch.zeros(grid, dtype=torch.int32, device="cuda")
    e = _LIB.lds_toy(grid, C.c_void_p(out.data_ptr()), C.c_void_p(raw))
    assert e == 0, f"lds_toy: hipError {e}"
    return out


def toy_sum(byte):
    """What lds_toy reports on a CU whose LDS holds `byte` everywhere."""
    return (TOY_WORDS * READS_AS[byte]["u32"]) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------ a polluted call
_LIBRARIES = ("_lib", "_lib_ext", "_lib_budget", "_lib_kmeans", "_lib_store")


def stream_entries():
    """library module -> the entry points whose last parameter is `void *stream`, read from the five headers."""
    import written_buffers as WB
    out = {}
    for header, module in zip(WB.HEADERS, _LIBRARIES):
        with open(os.path.join(ROOT, header), encoding="utf-8") as f:
            decl = WB.declarations(f.read())
        out[module] = sorted(fn for fn, args in decl.items() if args and re.fullmatch(r"void\s*\*\s*stream", args[-1])
                             and not fn.startswith(("vbq_comm", "vbq_allreduce")))           # (communicator calls: multi-GPU)
    return out


class Polluted:
    """`with Polluted(0x3C) as p:` -- every call of a C entry point that takes a stream (stream_entries()) is preceded, on
    that stream, by lds_fill(byte): nothing runs between the fill and the entry point's first launch.  byte None only counts the
    calls.  p.calls: entry point -> calls seen.  The wrapper stands in the attribute of the ctypes handle, where vbq_amd looks the
    function up at every call; the functions are put back on exit, also on an exception.  One at a time."""
    _active = None

    def __init__(self, byte):
        assert byte is None or 0 <= int(byte) <= 255
        self.byte, self.calls, self._saved = byte, {}, []

    def __enter__(self):
        import importlib
        assert Polluted._active is None, "a Polluted is already active"
        Polluted._active = self
        for module, names in stream_entries().items():
            h = importlib.import_module("vbq_amd." + module).lib()
            for name in names:
                real = getattr(h, name)
                self._saved.append((h, name, real))
                self.calls[name] = 0
                setattr(h, name, self._wrap(name, real))
        return self

    def _wrap(self, name, real):
        def polluted_entry(*args):
            self.calls[name] += 1
            if self.byte is not None:
                pollute(self.byte, args[-1])
            return real(*args)
        return polluted_entry

    def __exit__(self, *exc):
        for h, name, real in self._saved:
            setattr(h, name, real)
        Polluted._active = None
        return False


# ------------------------------------------------------------------------------------------------------------------ the scan
SOURCE_DIRS = ("vbq_amd/csrc", "vbq_amd/ext", "vbq_amd/budget", "vbq_amd/kmeans", "vbq_amd/store")
_SKIP = ("__launch_bounds__", "__align__", "__attribute__")


def _strip_c(text):
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    return re.sub(r"//[^\n]*", lambda m: " " * len(m.group(0)), text)


def _close(s, i, left, right):
    """The position after the bracket that closes the one at s[i]."""
    depth = 0
    while True:
        depth += s[i] == left
        depth -= s[i] == right
        i += 1
        if depth == 0:
            return i


def functions(text):
    """[(qualifier, name, body)] of every __global__ / __device__ function DEFINED in a source text (comments stripped)."""
    s, out = _strip_c(text), []
    for m in re.finditer(r"__(global|device)__", s):
        i = m.end()
        while True:                                                # attributes with arguments stand between the qualifier and the name
            par = s.find("(", i)
            words = re.findall(r"[A-Za-z_]\w*", s[i:par])
            if par < 0 or not words or words[-1] not in _SKIP:
                break
            i = _close(s, par, "(", ")")
        if par < 0 or not words:
            continue
        k = _close(s, par, "(", ")")
        while s[k] in " \t\n":
            k += 1
        if s[k] != "{":
            continue                                               # a declaration
        out.append((m.group(1), words[-1], s[k:_close(s, k, "{", "}")]))
    return out


def source_files():
    out = []
    for d in SOURCE_DIRS:
        out += [os.path.join(d, fn) for fn in sorted(os.listdir(os.path.join(ROOT, d))) if fn.endswith((".hip", ".h"))]
    return out


def kernels(texts=None):
    """kernel -> file, of every __global__ kernel that declares __shared__ storage itself or calls a device function (of any
    scanned file) that does.  `texts`: {file: source} instead of the tree."""
    if texts is None:
        texts = {}
        for rel in source_files():
            with open(os.path.join(ROOT, rel), encoding="utf-8") as f:
                texts[rel] = f.read()
    found = [(rel, q, name, body) for rel, text in texts.items() for q, name, body in functions(text)]
    uses = {name for _, q, name, body in found if q == "device" and "__shared__" in body}
    while True:                                                    # device functions that reach one through another
        more = {name for _, q, name, body in found if q == "device" and name not in uses
                and any(re.search(r"\b" + u + r"\s*[<(]", body) for u in uses)}
        if not more:
            break
        uses |= more
    out = {}
    for rel, q, name, body in found:
        if q == "global" and ("__shared__" in body or any(re.search(r"\b" + u + r"\s*[<(]", body) for u in uses)):
            assert out.get(name, rel) == rel, f"{name} is defined in {out[name]} and in {rel}"
            out[name] = rel
    return out


# ------------------------------------------------------------------------------------------------------------------ the catalogue
MULTI_GPU = "multi-GPU only"
ABOVE = "reached only by inputs above "                      # followed by the size
NEVER_FIRST = "never the first LDS-using launch of any entry point: "      # followed by the launch that runs before it
EXEMPT_REASONS = (MULTI_GPU, ABOVE, NEVER_FIRST)
"""The closed set."""

COVERED = {
    "k_bag": ["bags"],
    "k_bmshj_cdf_pdf": ["bmshj"],
    "k_bmshj_icdf_chain": ["bmshj"],
    "k_bmshj_nll_grad": ["bmshj", "bmshj_nll_grad_of_several_workgroups"],
    "k_budget_dp": ["budget_dp"],
    "k_budget_sweep": ["budget_sweep"],
    "k_gather_latents": ["gather_latents"],
    "k_gather_latents_vec": ["gather_latents_vector_tiles"],
    "k_gather_transpose": ["gather_transpose"],
    "k_hist_flat": ["histogram_flat_and_tiled", "histogram_with_fused_models"],
    "k_hist_tiled": ["histogram_flat_and_tiled"],
    "k_il_decode": ["interleaved_coder"],
    "k_il_decode_files": ["compact_files"],
    "k_il_encode": ["interleaved_coder"],
    "k_il_encode_files": ["compact_files"],
    "k_il_rates_files": ["compact_files"],
    "k_intervals": ["n_bit_intervals"],
    "k_kmeans1d": ["kmeans_dp"],
    "k_level_counts_hull": ["level_counts_hull"],
    "k_lookup_lds": ["lookup_from_the_lds"],
    "k_moments_bc": ["moments_one_workgroup_per_output", "moments_of_several_workgroups"],
    "k_moments_flat": ["moments_one_workgroup_per_output", "moments_of_several_workgroups"],
    "k_nearest_code": ["nearest_code"],
    "k_nearest_code_channels": ["nearest_code"],
    "k_normalize_t": ["image_metrics"],
    "k_np_block_sums": ["numpy_order_sums"],
    "k_np_finish": ["numpy_order_sums"],
    "k_prep_planes": ["prep_planes"],
    "k_quant_fast": ["solve_fast_indices", "solve_fast_values_and_lengths", "solve_fast_level_counters"],
    "k_quant_flat": ["solve_literal_flat"],
    "k_quant_hull_idx": ["solve_hull_indices"],
    "k_quant_notebook": ["notebook_literal"],
    "k_quant_notebook_fast": ["notebook_fast"],
    "k_quant_notebook_hull": ["notebook_hull"],
    "k_quant_notebook_pruned": ["notebook_pruned"],
    "k_quant_pruned": ["solve_pruned"],
    "k_quant_tiled": ["solve_literal_tiled"],
    "k_rans_decode": ["segment_coder", "segment_decoders_on_damaged_input"],
    "k_rans_decode_values": ["segment_coder", "segment_decoders_on_damaged_input"],
    "k_rans_decode_window": ["window_decodes", "window_decodes_of_a_table_that_does_not_sum"],
    "k_rans_encode": ["segment_coder"],
    "k_rans_encode_files": ["segment_files"],
    "k_rans_map_decode": ["mapped_coder"],
    "k_rans_map_decode_window": ["window_decodes", "window_decodes_of_a_table_that_does_not_sum"],
    "k_rans_map_encode": ["mapped_coder"],
    "k_rans_map_encode_files": ["mapped_files"],
    "k_rans_map_rates_files": ["mapped_files"],
    "k_rans_sizes": ["segment_coder"],
    "k_rans_sizes_files": ["segment_files"],
    "k_rd_sums": ["rd_sums_one_workgroup", "rd_sums_of_several_workgroups"],
    "k_records_pack": ["records"],
    "k_records_unpack": ["records"],
    "k_scan_groups": ["segment_coder"],
    "k_scores": ["scores"],
    "k_ssim_tile": ["image_metrics"],
    "k_topk": ["topk"],
    "k_transpose_batched": ["transposes"],
    "k_transpose_batched_vec": ["transposes"],
}
"""kernel -> the cases of tests/test_gpu_lds_state.py that launch it as the FIRST LDS-using launch of an entry point."""

EXEMPT = {
    "k_ssim_finish": NEVER_FIRST + "k_ssim_tile (vbq_ssim_scale_f64)",
    "k_rank_gemm": NEVER_FIRST + "k_normalize_t (vbq_analogy_ranks_f32)",
}
"""kernel -> why no case can put a fill in front of it (one of EXEMPT_REASONS).  An honest, named gap: their own oracle tests
(tests/test_gpu_metrics.py, tests/test_gpu_evaluators.py) hold their answers, on whatever their predecessor left in the LDS."""
