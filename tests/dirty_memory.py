"""No call's answer depends on what its fresh memory held: the fill, the site log and the tables.

The native libraries allocate nothing; every output, workspace, staging buffer and descriptor table comes from the Python layer
through torch.empty / torch.empty_like / np.empty / np.empty_like (tests/test_dirty_memory_host.py holds the sources to these four
spellings and the native trees to no allocation of their own).  A young process gets such memory fresh from the driver, where it
usually reads as zero -- the most forgiving value there is: a histogram that adds into an un-zeroed buffer is still right, a slot
nobody wrote reads as "size 0", a file's unwritten tail is zero bytes.  A process an hour old gets recycled blocks.

`Fill(byte)` makes the condition deterministic: while it is active the four names return memory whose every byte is `byte`.
Device tensors are filled through a uint8 view with fill_ (ordered on the current stream of the tensor's device, and capturable in
a graph), pinned and pageable host tensors and NumPy arrays on the host; zero-size results pass through; out= and every other
argument is forwarded unchanged; nothing else is patched (torch.zeros stays torch.zeros); the names are restored on exit, also on
an exception.  tests/test_gpu_dirty_memory.py answers every catalogued call unpatched and under each of FILLS and holds the four
answers to be the same, bit for bit.

FILLS and what an element of each dtype the library allocates reads as:

    byte   u8    u16     i32 / u32      i64 / u64      f32         f64
    0x00   0     0       0              0              0.0         0.0
    0x01   1     257     16 843 009     7.23e16        2.37e-38    7.75e-304
    0x3C   60    15 420  1 010 580 540  4.34e18        0.01149     1.53e-18

All finite, all positive, and no index of any table: NaN patterns, all-ones and the canaries of tests/footprint.py are deliberately
not used -- the rule tests/stream_order.py states for its stale inputs: a dependence on old memory must show as a wrong value,
never as a wild index.  0x00 is the forgiving baseline, kept so that a failure can say "differs from zero-filled memory".

THE SITE LOG.  Every filled allocation records the (file, line) of its caller when that file lies under vbq_amd/ (file: the name
inside vbq_amd, line: the line the call starts on); `sites_reached()` returns the set, `allocation_sites()` the static list of
every such call in vbq_amd/*.py (build.py excluded), read from the sources with ast.  The last test of the GPU module holds
allocation_sites() - sites_reached() - EXEMPT_SITES to be empty.  A NEW PUBLIC CALL GOES INTO A CATALOGUE (quantizer_histories.
PROBES, test_gpu_stream_order.CASES or section c of the GPU module); A NEW ALLOCATION SITE IS THEN REACHED, OR THE SUITE FAILS.

UNSPECIFIED names the parts of results a contract leaves open, each with the sentence that says so; EXEMPT_SITES the allocation
sites no GPU call of the module reaches, each with one of EXEMPT_REASONS.  Importable without a GPU."""
import ast
import os
import sys

import numpy as np

FILLS = (0x00, 0x01, 0x3C)

_TESTS = os.path.dirname(os.path.abspath(__file__))
PACKAGE = os.path.join(os.path.dirname(_TESTS), "vbq_amd")
HELPER = "tests/dirty_memory.py"
SPELLINGS = (("torch", "empty"), ("torch", "empty_like"), ("np", "empty"), ("np", "empty_like"))

_REACHED = set()
_SPANS = {}


# ------------------------------------------------------------------------------------------------------------------ the sites
def source_files():
    """The Python sources of the package, by their name inside vbq_amd; build.py (which runs the compiler, not the GPU) is left out."""
    return {name: os.path.join(PACKAGE, name) for name in sorted(os.listdir(PACKAGE)) if name.endswith(".py") and name != "build.py"}


def _calls(path):
    """(first line, last line) of every call of one of the four spellings in one file."""
    with open(path, encoding="utf-8") as f:
        tree = ast.parse(f.read(), path)
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and isinstance(node.func.value, ast.Name) \
                and (node.func.value.id, node.func.attr) in SPELLINGS:
            out.append((node.lineno, node.end_lineno))
    return sorted(out)


def _spans():
    if not _SPANS:
        for name, path in source_files().items():
            _SPANS[name] = _calls(path)
    return _SPANS


def allocation_sites():
    """Every torch.empty( / torch.empty_like( / np.empty( / np.empty_like( of vbq_amd/*.py as (file, line)."""
    return {(name, first) for name, spans in _spans().items() for first, _ in spans}


def sites_reached():
    return set(_REACHED)


def _log(frame):
    path = frame.f_code.co_filename
    if os.path.dirname(os.path.abspath(path)) != PACKAGE:
        return
    name, line = os.path.basename(path), frame.f_lineno
    # (a call that spans lines may be reported on any of them: the site is the line it starts on)
    starts = [first for first, last in _spans().get(name, ()) if first <= line <= last]
    _REACHED.add((name, max(starts) if starts else line))


# ------------------------------------------------------------------------------------------------------------------ the fill
def _scalar(byte, np_dtype):
    return np.frombuffer(bytes([byte]) * np.dtype(np_dtype).itemsize, dtype=np_dtype)[0]


def _fill_numpy(a, byte):
    if a.size == 0 or a.dtype.hasobject:
        return
    if a.flags.c_contiguous or a.flags.f_contiguous:
        a.reshape(-1, order="A").view(np.uint8)[...] = byte                     # padding bytes of a structured dtype included
    else:                                                                         # empty_like of a permuted prototype
        a[...] = _scalar(byte, a.dtype)


def _fill_torch(t, byte):
    import torch
    if not isinstance(t, torch.Tensor) or t.numel() == 0 or t.is_meta:
        return
    if t.is_contiguous():
        t.reshape(-1).view(torch.uint8).fill_(byte)
    else:                                                                         # empty_like of a permuted prototype
        from footprint import _NP
        t.fill_(_scalar(byte, _NP[t.dtype]).item())


class Fill:
    """See the module docstring.  `with Fill(0x3C): ...`; fills nest in no way: one at a time."""
    _active = None

    def __init__(self, byte):
        assert 0 <= int(byte) <= 255
        self.byte = int(byte)

    def _wrap(self, real, fill):
        byte = self.byte

        def patched(*args, **kwargs):
            out = real(*args, **kwargs)
            fill(out, byte)
            if (out.numel() if hasattr(out, "numel") else getattr(out, "size", 0)):      # zero-size results pass through
                _log(sys._getframe(1))
            return out
        patched.__name__ = real.__name__
        patched.__wrapped__ = real
        return patched

    def __enter__(self):
        import torch
        assert Fill._active is None, "a Fill is already active"
        self._saved = (torch.empty, torch.empty_like, np.empty, np.empty_like)
        Fill._active = self
        torch.empty, torch.empty_like = self._wrap(self._saved[0], _fill_torch), self._wrap(self._saved[1], _fill_torch)
        np.empty, np.empty_like = self._wrap(self._saved[2], _fill_numpy), self._wrap(self._saved[3], _fill_numpy)
        return self

    def __exit__(self, *exc):
        import torch
        torch.empty, torch.empty_like, np.empty, np.empty_like = self._saved
        Fill._active = None
        return False


# ------------------------------------------------------------------------------------------------------------------ comparison
def first_difference(a, b, path="answer"):
    """Where two plain answers (quantizer_histories._plain) first differ, as text: the leaf and, in an array, the element."""
    if isinstance(a, tuple) or isinstance(b, tuple):
        if not (isinstance(a, tuple) and isinstance(b, tuple)):
            return f"{path}: {type(a).__name__} against {type(b).__name__}"
        if len(a) != len(b):
            return f"{path}: {len(a)} against {len(b)} entries"
        for k, (x, y) in enumerate(zip(a, b)):
            d = first_difference(x, y, f"{path}[{k}]")
            if d:
                return d
        return None
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        if not (isinstance(a, np.ndarray) and isinstance(b, np.ndarray)):
            return f"{path}: {type(a).__name__} against {type(b).__name__}"
        if a.dtype != b.dtype or a.shape != b.shape:
            return f"{path}: {a.dtype}{a.shape} against {b.dtype}{b.shape}"
        if a.tobytes() == b.tobytes():
            return None
        ua, ub = (np.ascontiguousarray(v).reshape(-1).view(np.uint8).reshape(v.size, -1) for v in (a, b))
        k = int(np.flatnonzero((ua != ub).any(axis=1))[0])
        at = tuple(int(v) for v in np.unravel_index(k, a.shape)) if a.ndim else ()
        return f"{path}{list(at)}: {a.reshape(-1)[k].item()!r} against {b.reshape(-1)[k].item()!r} ({int((ua != ub).any(axis=1).sum())} of {a.size} elements differ)"
    if isinstance(a, (bytes, str)) and isinstance(b, (bytes, str)) and type(a) is type(b) and a != b:
        k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        return f"{path}: lengths {len(a)} and {len(b)}, first difference at position {k}"
    return None if (type(a) is type(b) and a == b) else f"{path}: {a!r} against {b!r}"


# ------------------------------------------------------------------------------------------------------------------ the tables
UNSPECIFIED = {
    # call of tests/test_gpu_dirty_memory.py -> ((file, the sentence of its docstring or header that leaves part of the result
    # open), ...); the module masks exactly that part (its MASKS has the same keys).  An entry without such a sentence is a
    # finding, not an entry.
    "coder_packed_forms": (
        ("vbq_amd/coder.py", "whose first `total` words are valid"),
        ("include/vbq.h", "The decoder only reads the first size[g] words of a segment: d_words need not be zeroed.")),
    "kmeans1d_dp_with_a_nan_channel": (
        ("include/vbq_kmeans.h", "That channel's outputs are unspecified but within bounds (starts in [1, n])"),),
}

EMPTY_RESULT = "returns an empty result (zero elements)"
MULTI_GPU = "multi-GPU only"
HOST_ONLY = "host-only, covered in test_dirty_memory_host.py::"
EVALUATION = "evaluation harness (utils.evaluate_*), frozen"
EXEMPT_REASONS = (EMPTY_RESULT, MULTI_GPU, HOST_ONLY, EVALUATION)
"""The closed set.  HOST_ONLY is followed by the name of the test."""

_HOST_TEST = HOST_ONLY + "test_host_only_paths_under_every_fill"
EXEMPT_SITES = {
    # (file, line) -> reason
    ("coder.py", 38): _HOST_TEST,                      # quantize_frequencies
    ("tables.py", 42): _HOST_TEST,                     # level_major_to_sorted
    ("pipeline.py", 166): _HOST_TEST,                 # numpy_log2_f32_loop's self-test of the host routine, once per process
    ("embeddings.py", 403): EMPTY_RESULT,              # CompressedEmbeddings.rows([])
    ("embeddings.py", 874): EMPTY_RESULT,              # RecordEmbeddings.rows([])
    ("quantizer.py", 828): EMPTY_RESULT,               # a window call with no file, no channel or an empty extent
    ("quantizer.py", 1325): EMPTY_RESULT,              # decompress_latents_compact_batch([])
    ("rows_budget.py", 77): EMPTY_RESULT,              # quantize_rows_to_budget of no rows
    ("rows_budget.py", 170): EMPTY_RESULT,             # quantize_rows_to_budgets of no rows or no budgets
    ("rows_budget.py", 171): EMPTY_RESULT,
    ("rows_budget.py", 203): EMPTY_RESULT,             # budget_curve of no rows
    ("utils.py", 255): EVALUATION,
    ("utils.py", 359): EVALUATION,
    ("utils.py", 361): EVALUATION,
}
