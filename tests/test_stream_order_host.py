"""The tables of tests/stream_order.py hold, and the sources keep the stream discipline the late-input harness cannot see
(no GPU needed).

Tables: every probe of quantizer_histories.PROBES is in exactly one of LATE and HOST; every vbq_amd/csrc/*.hip is a key of
BY_SOURCE; every symbol a case names is declared in include/vbq.h and defined in the file it is listed under (`entry >
launcher`: the entry point is declared in the header, the launcher -- a function that takes the hipStream_t -- is defined in
the file and called from the file that defines the entry point); every exemption is the closed set's reason for that file.
The pure helpers of the harness: the stale / fresh recipes are valid and differ, the delay rule holds.

Static stream discipline -- what covers the blocking calls, which the harness cannot arm:
  * every hipLaunchKernelGGL of vbq_amd/csrc passes `st` or `reinterpret_cast<hipStream_t>(stream)` as its stream, every
    hipMemsetAsync / hipMemcpyAsync the same as its last argument, and every `hipStream_t st` is a function parameter or is
    initialised from exactly that cast; no other stream variable exists;
  * no kernel<<<>>> launch, synchronous copy or memset, device or stream synchronisation, allocation, per-thread stream, and no
    literal 0 / nullptr in a stream position (ALLOWED carries a written reason per file and construct; it is empty);
  * every Python call site `.vbq_<name>(` of a function whose header declaration has a `void *stream` parameter passes
    ops._stream(<expr>) / _stream(<expr>) at that position.
Every check is tried on a planted string first: a rule that matches nothing does not pass."""
import glob
import os
import re

import numpy as np
import pytest

import quantizer_histories as QH
import stream_order as SO
from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vbq_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "vbq.h")
CAST = "reinterpret_cast<hipStream_t>(stream)"
STREAM_FORMS = ("st", CAST)


def _read(path):
    with open(path) as f:
        return f.read()


def sources():
    return {os.path.basename(p): _read(p) for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))}


# ------------------------------------------------------------------------------------------------------------------ parsing
def strip_c(text):
    """C / C++ text without comments, string and character literals blanked (their length kept)."""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if text.startswith("//", i):
            j = text.find("\n", i)
            j = n if j < 0 else j
            out.append(" " * (j - i))
            i = j
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            j = n if j < 0 else j + 2
            out.append(re.sub(r"[^\n]", " ", text[i:j]))
            i = j
        elif c in "\"'":
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            out.append(c + " " * (j - i - 1) + c)
            i = j + 1
        else:
            out.append(c)
            i += 1
    return "".join(out)


def strip_py(text):
    """Python text without comments, string literals blanked (triple-quoted ones too)."""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if c == "#":
            j = text.find("\n", i)
            j = n if j < 0 else j
            i = j
        elif c in "\"'":
            q = text[i:i + 3] if text[i:i + 3] in ('"""', "'''") else c
            j = i + len(q)
            while j < n and not text.startswith(q, j):
                j += 2 if text[j] == "\\" else 1
            out.append(q + re.sub(r"[^\n]", " ", text[i + len(q):j]) + q)
            i = j + len(q)
        else:
            out.append(c)
            i += 1
    return "".join(out)


def call_args(text, open_paren):
    """The arguments of the call whose `(` is at text[open_paren], split at top-level commas by bracket matching (round, square
    and curly brackets; angle brackets are not brackets: template arguments with commas stand in parentheses)."""
    assert text[open_paren] == "("
    depth, args, start = 0, [], open_paren + 1
    for i in range(open_paren, len(text)):
        c = text[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                last = text[start:i].strip()
                return args + [last] if last or args else args
        elif c == "," and depth == 1:
            args.append(text[start:i].strip())
            start = i + 1
    raise AssertionError("unbalanced call at offset %d" % open_paren)


def calls(text, name):
    """[(offset, [arguments])] of every call of `name` in stripped text."""
    return [(m.start(), call_args(text, m.end() - 1)) for m in re.finditer(r"(?<![A-Za-z0-9_])" + re.escape(name) + r"\s*\(", text)]


def _norm(arg):
    return re.sub(r"\s+", "", arg)


# ------------------------------------------------------------------------------------------------------------------ the rules
def launch_violations(text):
    """hipLaunchKernelGGL(kernel, grid, block, lds, STREAM, ...) -> (number of launches, the ones whose stream is not a form)."""
    found = calls(strip_c(text), "hipLaunchKernelGGL")
    return len(found), [(off, a[4] if len(a) > 4 else None) for off, a in found if len(a) < 5 or _norm(a[4]) not in STREAM_FORMS]


def async_violations(text):
    """hipMemsetAsync / hipMemcpyAsync (and their 2D / 3D / D8.. kin): the stream is the last argument."""
    s = strip_c(text)
    found = [(name, off, a) for name in sorted(set(re.findall(r"\bhipMem(?:set|cpy)\w*Async\b", s))) for off, a in calls(s, name)]
    return len(found), [(name, off, a[-1] if a else None) for name, off, a in found if not a or _norm(a[-1]) not in STREAM_FORMS]


def stream_variable_violations(text):
    """Every `hipStream_t` token is the cast, an unnamed parameter of a function type, the parameter `st`, or `st` initialised
    from exactly the cast."""
    s = strip_c(text)
    bad, n = [], 0
    for m in re.finditer(r"\bhipStream_t\b", s):
        n += 1
        before, after = s[max(0, m.start() - 17):m.start()], s[m.end():m.end() + 80]
        if before.endswith("reinterpret_cast<") and re.match(r">\s*\(\s*stream\s*\)", after):
            continue
        if re.match(r"\s*[,)]", after):                                   # unnamed: a prototype or a function-pointer type
            continue
        if re.match(r"\s+st\s*[,)]", after):                              # the parameter
            continue
        if re.match(r"\s+st\s*=\s*reinterpret_cast<hipStream_t>\(stream\)\s*;", after):
            continue
        bad.append((m.start(), (before + "hipStream_t" + after.split("\n")[0]).strip()))
    return n, bad


FORBIDDEN = {
    "<<<": r"<<<",
    "hipMemcpy(": r"\bhipMemcpy\s*\(",
    "hipMemset(": r"\bhipMemset\s*\(",
    "hipDeviceSynchronize": r"\bhipDeviceSynchronize\b",
    "hipStreamSynchronize": r"\bhipStreamSynchronize\b",
    "hipMalloc": r"\bhipMalloc\w*\b",
    "hipFree": r"\bhipFree\w*\b",
    "hipStreamPerThread": r"\bhipStreamPerThread\b",
}
ALLOWED = {}
"""(file, construct) -> the written reason it may occur there.  Empty: vbq_comm.hip hands its stream to the collective library
through the same cast and allocates nothing."""


def forbidden_found(text):
    s = strip_c(text)
    return sorted(name for name, pat in FORBIDDEN.items() if re.search(pat, s))


STREAM_TAKERS = ("hipLaunchKernelGGL", "hipEventRecord", "hipStreamWaitEvent", "hipLaunchHostFunc", "hipGraphLaunch",
                 "hipStreamBeginCapture", "hipLaunchCooperativeKernel", "hipModuleLaunchKernel", "hipExtLaunchKernelGGL")


def literal_stream_violations(text):
    """A literal 0 / NULL / nullptr / hipStreamLegacy where a stream goes: argument 5 of a launch, the last argument of an
    asynchronous memset or copy, any argument of the other runtime calls that take a stream whose text is such a literal and
    that stands where the stream does (the first for host functions and captures, the second for events and graphs)."""
    s = strip_c(text)
    lit = re.compile(r"^(?:\(\s*hipStream_t\s*\)\s*)?(?:0|NULL|nullptr|hipStreamLegacy|hipStreamDefault)$")
    where = {"hipLaunchKernelGGL": 4, "hipExtLaunchKernelGGL": 4, "hipEventRecord": 1, "hipStreamWaitEvent": 0,
             "hipLaunchHostFunc": 0, "hipGraphLaunch": 1, "hipStreamBeginCapture": 0, "hipLaunchCooperativeKernel": 5,
             "hipModuleLaunchKernel": 8}
    bad = []
    for name in STREAM_TAKERS:
        for off, a in calls(s, name):
            if len(a) > where[name] and lit.match(a[where[name]].strip()):
                bad.append((name, off, a[where[name]]))
    for name in sorted(set(re.findall(r"\bhipMem(?:set|cpy)\w*Async\b", s))):
        bad += [(name, off, a[-1]) for off, a in calls(s, name) if a and lit.match(a[-1].strip())]
    return bad


def stream_positions(header_text):
    """{function: index of its `void *stream` parameter} for every declaration of the header that has one."""
    s = strip_c(header_text)
    out = {}
    for m in re.finditer(r"\b(vbq_[a-z0-9_]+)\s*\(", s):
        args = call_args(s, m.end() - 1)
        at = [i for i, a in enumerate(args) if re.fullmatch(r"void\s*\*\s*stream", a)]
        assert len(at) <= 1, (m.group(1), args)
        if at:
            out[m.group(1)] = at[0]
    return out


STREAM_ARG = re.compile(r"^(?:ops\.)?_stream\(.+\)$", re.S)
ALIASED = {("ops.py", "vbq_histogram_u16"): "fn", ("ops.py", "vbq_histogram_u16_i32"): "fn"}
"""(file, function) -> the local name the bound function is called through where the call site is not `.vbq_<name>(`."""


def python_site_violations(py_text, positions, fname="", aliased=ALIASED):
    """-> (call sites of stream functions seen, those that do not pass [ops.]_stream(<expr>) at the header's position)."""
    s = strip_py(py_text)
    seen, bad = 0, []
    for m in re.finditer(r"\.(vbq_[a-z0-9_]+)\b", s):
        name = m.group(1)
        if name not in positions:
            continue
        rest = s[m.end():]
        if re.match(r"\s*\(", rest):
            sites = [call_args(s, m.end() + rest.index("("))]
        else:
            alias = aliased.get((fname, name))
            if alias is None:
                bad.append((name, "mentioned without a call and not listed in ALIASED"))
                continue
            sites = [a for _, a in calls(s[m.end():], alias)]
            if not sites:
                bad.append((name, f"no call through {alias!r} follows"))
        for args in sites:
            seen += 1
            p = positions[name]
            if len(args) <= p or not STREAM_ARG.match(_norm(args[p])):
                bad.append((name, args[p] if len(args) > p else f"{len(args)} arguments"))
    return seen, bad


# ------------------------------------------------------------------------------------------------------------------ self-tests
GOOD_LAUNCH = """
// hipLaunchKernelGGL(k, g, b, 0, 0) in a comment does not count
void f(void *stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL((k_two<N, CountT>), dim3((unsigned)gx, (unsigned)L), dim3(256), lds ? lds : 0, st, a, b[i, j], "x, y)");
    hipLaunchKernelGGL(k_one, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                       d_x, (long)n);
    if (hipMemsetAsync(d, 0, sizeof(int) * (size_t)n, st) != hipSuccess) return;
}
int g(const float *x, hipStream_t st);
typedef int (*fn_t)(const float *, hipStream_t);
"""


def test_the_parsers_read_a_planted_source():
    assert call_args("f((a, b), c[1, 2], {3, 4}, g(h(5, 6)))", 1) == ["(a, b)", "c[1, 2]", "{3, 4}", "g(h(5, 6))"]
    assert call_args("f()", 1) == [] and call_args("f(x)", 1) == ["x"]
    assert "comment" not in strip_c(GOOD_LAUNCH) and "x, y)" not in strip_c(GOOD_LAUNCH)
    assert len(strip_c(GOOD_LAUNCH)) == len(GOOD_LAUNCH)
    assert launch_violations(GOOD_LAUNCH) == (2, [])
    assert async_violations(GOOD_LAUNCH) == (1, [])
    assert stream_variable_violations(GOOD_LAUNCH) == (5, [])
    assert forbidden_found(GOOD_LAUNCH) == [] and literal_stream_violations(GOOD_LAUNCH) == []


@pytest.mark.parametrize("planted,rule", [
    ("hipLaunchKernelGGL(k_one, dim3(1), dim3(64), 0, 0, d_x);", "launch"),
    ("hipLaunchKernelGGL(k_one, dim3(1), dim3(64), 0, nullptr, d_x);", "launch"),
    ("hipLaunchKernelGGL((k<A, B>), dim3(1), dim3(64), 0, other, d_x);", "launch"),
    ("hipLaunchKernelGGL(k_one, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream2), d_x);", "launch"),
    ("hipLaunchKernelGGL(k_one, dim3(1), dim3(64), 0);", "launch"),
    ("hipMemsetAsync(d, 0, n, 0);", "async"),
    ("hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, mine);", "async"),
    ("hipMemcpy2DAsync(d, p, s, q, w, h, hipMemcpyDeviceToDevice);", "async"),
    ("hipStream_t st = nullptr;", "variable"),
    ("hipStream_t st = reinterpret_cast<hipStream_t>(other);", "variable"),
    ("hipStream_t mine;", "variable"),
    ("static hipStream_t side = make();", "variable"),
    ("hipStream_t st;", "variable"),
    ("k_one<<<1, 64, 0, st>>>(d_x);", "forbidden"),
    ("hipMemcpy(d, s, n, hipMemcpyDeviceToHost);", "forbidden"),
    ("hipMemset (d, 0, n);", "forbidden"),
    ("hipDeviceSynchronize();", "forbidden"),
    ("hipStreamSynchronize(st);", "forbidden"),
    ("hipMalloc(&p, n);", "forbidden"),
    ("hipMallocAsync(&p, n, st);", "forbidden"),
    ("hipFree(p);", "forbidden"),
    ("hipLaunchKernelGGL(k, g, b, 0, hipStreamPerThread, x);", "forbidden"),
    ("hipEventRecord(ev, 0);", "literal"),
    ("hipLaunchHostFunc(nullptr, fn, p);", "literal"),
    ("hipLaunchKernelGGL(k, g, b, 0, (hipStream_t)0, x);", "literal"),
    ("hipMemsetAsync(d, 0, n, NULL);", "literal"),
])
def test_each_rule_fails_on_a_planted_violation(planted, rule):
    text = GOOD_LAUNCH + "\nvoid h(void *stream) {\n    " + planted + "\n}\n"
    got = {"launch": launch_violations(text)[1], "async": async_violations(text)[1],
           "variable": stream_variable_violations(text)[1], "forbidden": forbidden_found(text),
           "literal": literal_stream_violations(text)}
    assert got[rule], (planted, got)
    # and a violation inside a comment or a string is none
    quiet = GOOD_LAUNCH + "\n// " + planted + "\nconst char *s = \"" + planted.replace('"', "'") + "\";\n"
    assert not launch_violations(quiet)[1] and not async_violations(quiet)[1] and not stream_variable_violations(quiet)[1]
    assert not forbidden_found(quiet) and not literal_stream_violations(quiet)


PLANTED_HEADER = """
/* int vbq_gone(void *stream); */
int vbq_a_f32(const float *d_x, int64_t n,   // comment, with a comma
              float *d_out, void *stream);
int vbq_b_u16(const uint16_t *d_idx, void *stream, int32_t tail);
size_t vbq_b_workspace_bytes(int64_t n);
const char *vbq_last_error(void);
"""
PLANTED_PY = '''
def a(x, out):
    """docstring naming h.vbq_a_f32(x, 1, out, None)"""
    check(_lib.lib().vbq_a_f32(_ptr(x), x.numel(),          # a comment, _stream(y)
                               _ptr(out), _stream(x)), "vbq_a_f32")
    check(h.vbq_b_u16(ops._ptr(idx), ops._stream(idx if idx is not None else words), 3), "vbq_b_u16")
    n = h.vbq_b_workspace_bytes(5)
'''


def test_the_python_rule_reads_a_planted_module_and_fails_on_planted_violations():
    pos = stream_positions(PLANTED_HEADER)
    assert pos == {"vbq_a_f32": 3, "vbq_b_u16": 1}
    assert python_site_violations(PLANTED_PY, pos) == (2, [])
    for good, bad in [("_stream(x)), \"vbq_a_f32\")", "None), \"vbq_a_f32\")"),
                      ("_stream(x)), \"vbq_a_f32\")", "C.c_void_p(0)), \"vbq_a_f32\")"),
                      ("_stream(x)), \"vbq_a_f32\")", "stream), \"vbq_a_f32\")"),
                      ("_ptr(out), _stream(x))", "_stream(x), _ptr(out))"),                       # the wrong position
                      ("ops._stream(idx if idx is not None else words), 3)", "3, ops._stream(idx))"),
                      ("ops._stream(idx if idx is not None else words), 3)", "ops.raw_stream(idx.device), 3)")]:
        assert good in PLANTED_PY
        seen, found = python_site_violations(PLANTED_PY.replace(good, bad), pos)
        assert seen == 2 and len(found) == 1, (bad, found)
    # a bound function that is not called where it is named must be listed
    alias = "fn = h.vbq_a_f32\ncheck(fn(_ptr(x), 1, _ptr(out), _stream(x)))\n"
    assert python_site_violations(alias, pos, "m.py")[1] == [("vbq_a_f32", "mentioned without a call and not listed in ALIASED")]
    assert python_site_violations(alias, pos, "m.py", {("m.py", "vbq_a_f32"): "fn"}) == (1, [])
    assert python_site_violations(alias.replace("_stream(x)", "0"), pos, "m.py", {("m.py", "vbq_a_f32"): "fn"})[1]


# ------------------------------------------------------------------------------------------------------------------ the sources
def test_every_launch_names_the_callers_stream():
    total = 0
    for name, text in sources().items():
        n, bad = launch_violations(text)
        total += n
        assert not bad, f"{name}: launches whose stream argument is neither `st` nor the cast of `stream`: {bad}"
        assert n == len(re.findall(r"\bhipLaunchKernelGGL\b", strip_c(text))), f"{name}: a launch the parser did not read"
    assert total >= 100, f"only {total} launches found: the sources moved, or the rule reads nothing"


def test_every_async_memset_and_copy_names_the_callers_stream():
    total = 0
    for name, text in sources().items():
        n, bad = async_violations(text)
        total += n
        assert not bad, f"{name}: {bad}"
    assert total >= 4, total


def test_every_stream_variable_is_the_callers_stream():
    total = 0
    for name, text in sources().items():
        n, bad = stream_variable_violations(text)
        total += n
        assert not bad, f"{name}: a hipStream_t that is neither the parameter `st`, `st` = the cast of `stream`, nor the cast itself: {bad}"
    assert total >= 80, total


def test_no_forbidden_construct_occurs():
    files = sources()
    for (name, what), reason in ALLOWED.items():
        assert name in files and what in FORBIDDEN and len(reason.split()) >= 4, (name, what, reason)
        assert what in forbidden_found(files[name]), f"ALLOWED lists {what} in {name}, which no longer holds it: drop the entry"
    assert set(n for n, _ in ALLOWED) <= {"vbq_comm.hip"}
    for name, text in files.items():
        found = [w for w in forbidden_found(text) if (name, w) not in ALLOWED]
        assert not found, f"{name}: {found}"
        assert not literal_stream_violations(text), f"{name}: {literal_stream_violations(text)}"


def test_every_python_call_site_passes_the_tensors_stream():
    pos = stream_positions(_read(HEADER))
    declared = set(declared_functions())
    assert len(pos) >= 70 and set(pos) <= declared, (len(pos), sorted(set(pos) - declared))
    for must, at in (("vbq_transpose_f32", 4), ("vbq_check_inputs_f32", 4)):
        assert pos[must] == at
    total, called = 0, set()
    for path in sorted(glob.glob(os.path.join(ROOT, "vbq_amd", "*.py"))):
        text = _read(path)
        seen, bad = python_site_violations(text, pos, os.path.basename(path))
        total += seen
        called |= {m for m in re.findall(r"\.(vbq_[a-z0-9_]+)\b", strip_py(text)) if m in pos}
        assert not bad, f"{os.path.basename(path)}: call sites that do not pass [ops.]_stream(<expr>) where the header has `void *stream`: {bad}"
    assert total >= 70, total
    assert called == set(pos), f"stream functions of the header with no Python call site: {sorted(set(pos) - called)}"
    for (fname, name), alias in ALIASED.items():
        assert name in pos and re.search(r"\." + name + r"\b(?!\s*\()", strip_py(_read(os.path.join(ROOT, "vbq_amd", fname)))), (fname, name)


# ------------------------------------------------------------------------------------------------------------------ the tables
def test_every_probe_is_late_or_host():
    assert not set(SO.LATE) & set(SO.HOST), sorted(set(SO.LATE) & set(SO.HOST))
    assert set(SO.LATE) | set(SO.HOST) == set(QH.PROBES), (sorted(set(QH.PROBES) - set(SO.LATE) - set(SO.HOST)),
                                                          sorted((set(SO.LATE) | set(SO.HOST)) - set(QH.PROBES)))
    assert all(isinstance(v, str) and v for v in list(SO.LATE.values()) + list(SO.HOST.values()))
    # what the issue fixes: the file, batch, latent and image probes are late; rows, intervals, the codec and the readers are not
    assert set(SO.LATE) == set(QH.ONE_FILE) | set(QH.BATCHES) | set(QH.WITH_VAE) | {"latents", "latents_mapped"}


def _defined(name, text):
    """`name` is defined (not merely declared or called) in the stripped source: `name(...) {` at brace depth of a definition."""
    for off, _ in calls(text, name):
        close = off + len(name)
        close = text.index("(", close)
        depth = 0
        for i in range(close, len(text)):
            depth += text[i] == "("
            depth -= text[i] == ")"
            if depth == 0:
                if re.match(r"\s*\{", text[i + 1:]):
                    return True
                break
    return False


def test_by_source_names_every_file_and_only_symbols_that_exist():
    files = {n: strip_c(t) for n, t in sources().items()}
    hips = sorted(n for n in files if n.endswith(".hip"))
    assert sorted(SO.BY_SOURCE) == hips, (sorted(set(hips) - set(SO.BY_SOURCE)), sorted(set(SO.BY_SOURCE) - set(hips)))
    declared = set(declared_functions())
    entry_file = {}
    for n in hips:
        for sym in re.findall(r'extern\s+"\s*"\s+[^;{()]*?\b(vbq_[a-z0-9_]+)\s*\(', files[n]):
            if _defined(sym, files[n]):
                entry_file[sym] = n
    assert len(entry_file) >= 90, len(entry_file)
    assert set(SO.EXEMPT_REASONS.values()) == {SO.SEVERAL_RANKS, SO.NO_DEVICE_WORK}
    for name, row in SO.BY_SOURCE.items():
        if isinstance(row, str):
            assert SO.EXEMPT_REASONS.get(name) == row, f"{name}: {row!r} is not the closed set's reason for this file"
            if row == SO.NO_DEVICE_WORK:
                assert launch_violations(files[name])[0] == 0 and "hipStream_t" not in files[name], name
            continue
        assert name not in SO.EXEMPT_REASONS and row, name
        for case, symbols in row.items():
            assert symbols, (name, case)
            if case.startswith("probe:"):
                assert case[6:] in QH.PROBES, (name, case)
            for sym in symbols:
                entry, _, launcher = (s.strip() for s in sym.partition(">"))
                assert entry in declared, f"{name} / {case}: {entry} is not declared in include/vbq.h"
                if not launcher:
                    assert entry_file.get(entry) == name, f"{name} / {case}: {entry} is defined in {entry_file.get(entry)}"
                else:
                    assert _defined(launcher, files[name]) and re.search(r"\b" + launcher + r"\s*(<[^;{}]*?>)?\s*\([^;{}]*hipStream_t st\)\s*\{",
                                                                        files[name]), f"{name} / {case}: {launcher} is no launcher defined here"
                    home = files[entry_file[entry]]
                    assert entry_file[entry] != name and len(calls(home, launcher)) + len(re.findall(r"\b" + launcher + r"\s*<", home)) > 0, \
                        f"{name} / {case}: {entry_file[entry]}, which defines {entry}, never calls {launcher}"


def test_cases_named_in_by_source_exist_in_the_gpu_module():
    import ast
    tree = ast.parse(_read(os.path.join(ROOT, "tests", "test_gpu_stream_order.py")))
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
    keys = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "id", None) == "case" and node.args and isinstance(node.args[0], ast.Constant):
            keys.add(node.args[0].value)
    assert len(keys) >= 30, sorted(keys)
    named = {c for row in SO.BY_SOURCE.values() if isinstance(row, dict) for c in row if not c.startswith("probe:")}
    missing = sorted(c for c in named if c not in keys and "test_" + c not in tests)
    assert not missing, f"BY_SOURCE names cases the GPU module does not have: {missing}"


# ------------------------------------------------------------------------------------------------------------------ the helpers
def test_the_delay_rule():
    assert SO.SLACK == 4.0 and SO.CAP_MS == 400.0 and 0 < SO.FLOOR_MS <= SO.CAP_MS
    assert SO.delay_ms(0.0) == SO.FLOOR_MS and SO.delay_ms(SO.FLOOR_MS / 4) == SO.FLOOR_MS
    assert SO.delay_ms(SO.FLOOR_MS) == 4 * SO.FLOOR_MS if 4 * SO.FLOOR_MS <= SO.CAP_MS else SO.delay_ms(SO.FLOOR_MS) == SO.CAP_MS
    assert SO.delay_ms(99.0) == 396.0 and SO.delay_ms(100.0) == 400.0 and SO.delay_ms(101.0) == 400.0 and SO.delay_ms(1e9) == SO.CAP_MS
    assert SO.fits_cap(100.0) and not SO.fits_cap(100.1)
    assert SO.cycles_per_ms(100_000, 1.5, 1_000_000, 10.5) == pytest.approx(100_000)
    for c1, m1, c2, m2 in [(10, 1.0, 100, 1.0), (10, 2.0, 100, 1.0), (100, 1.0, 10, 2.0), (10, 0.0, 100, 1.0)]:
        with pytest.raises(ValueError):
            SO.cycles_per_ms(c1, m1, c2, m2)
    with pytest.raises(AssertionError):
        SO.Spin("sleep", 1e5).enqueue(SO.CAP_MS + 1)


def test_the_stale_recipe_of_the_probes_is_valid_and_differs():
    fresh, stale = QH.latents(QH.FILE_SHAPES), QH.latents(QH.FILE_SHAPES, seed=SO.STALE_SEED)
    SO.check_recipe([list(p) for p in fresh], [list(p) for p in stale])
    for (m, lv), (ms, lvs) in zip(fresh, stale):
        assert m.tobytes() != ms.tobytes() and lv.tobytes() != lvs.tobytes()
    with pytest.raises(AssertionError, match="equal the fresh"):
        SO.check_recipe([list(p) for p in fresh], [list(p) for p in QH.latents(QH.FILE_SHAPES)])
    with pytest.raises(AssertionError):
        SO.check_recipe([np.zeros(3, np.float32)], [np.zeros(4, np.float32)])
    with pytest.raises(AssertionError):
        SO.check_recipe([np.zeros(3, np.float32)], [np.array([0, np.nan, 1], np.float32)])
    with pytest.raises(AssertionError):
        SO.check_recipe([np.zeros(3, np.float32)], [np.ones(3, np.float64)])


def test_outcomes_compare_by_bit_pattern():
    a = ("ok", (np.array([0.0, np.nan], np.float32), b"x", 3))
    assert QH.same(SO.bits(a), SO.bits(("ok", (np.array([0.0, np.nan], np.float32), b"x", 3))))
    assert not QH.same(SO.bits(a), SO.bits(("ok", (np.array([-0.0, np.nan], np.float32), b"x", 3))))
    assert SO.bits(a)[1][0].dtype == np.uint32
