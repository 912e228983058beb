"""A call that refuses has enqueued nothing: the static half of the rule of include/vbq.h (no GPU needed; the other half is
tests/test_gpu_refused_calls.py, which looks at the bytes).

Every function body of vbq_amd/csrc is walked as text (comments and strings blanked, tests/test_stream_order_host.py's parser).
Its FIRST ENQUEUE is the first hipLaunchKernelGGL, hipMemsetAsync / hipMemcpyAsync, or call of a function of these sources that
itself enqueues (a `launch_*` helper, a `vbq_*` entry point, a shared `*_entry`).  After it the body may hold none of
  * a VBQ_REQUIRE;
  * a set_error whose return code is not VBQ_ERR_LAUNCH;
  * a call of a function that can itself refuse: one whose body (or a callee's) holds one of the two above, or -- a
    launch_* helper -- a `return 1`.
EXCEPTIONS is the closed table (function, what) -> reason, and a reason is one of two: NOT_A_REFUSAL (a helper's "returns 1:
not of this kind" enqueues nothing and the caller goes on to the next kernel) or PREEMPTED + the name of the check that, before
the first enqueue, refuses everything the inner call could refuse.  A NEW LATE REFUSAL FAILS HERE UNTIL IT IS MOVED UP, OR
LISTED WITH ONE OF THE TWO.  Every rule is tried on a planted source first."""
import re

import pytest

from test_stream_order_host import calls, sources, strip_c

NOT_A_REFUSAL = "returns 1: not of this kind -- nothing was enqueued and the caller takes the next kernel"
PREEMPTED = "the inner call's refusals are pre-empted by "
REASONS = (NOT_A_REFUSAL, PREEMPTED)

KEYWORDS = {"if", "for", "while", "switch", "return", "sizeof", "catch", "defined", "alignas", "decltype", "static_assert"}
ENQUEUE_CALLS = ("hipLaunchKernelGGL", "hipMemsetAsync", "hipMemcpyAsync")


# ------------------------------------------------------------------------------------------------------------------ parsing
def _match(text, i, open_c, close_c):
    depth = 0
    for j in range(i, len(text)):
        depth += text[j] == open_c
        depth -= text[j] == close_c
        if depth == 0:
            return j
    raise AssertionError("unbalanced %s at offset %d" % (open_c, i))


def _no_directives(text):
    """Stripped text with the preprocessor directives OUTSIDE function bodies blanked (continuation lines too): a macro defined
    inside a body belongs to that body's text, one defined at file level to nobody's."""
    out, depth, i, n = list(text), 0, 0, len(text)
    scopes = []                                   # True: a namespace / extern "C" block, which does not count as depth
    line_start = True
    while i < n:
        c = text[i]
        if c == "#" and line_start and depth == 0:
            j = i
            while True:
                k = text.find("\n", j)
                k = n if k < 0 else k
                if k == n or text[j:k].rstrip()[-1:] != "\\":
                    break
                j = k + 1
            for p in range(i, k):
                out[p] = " "
            i = k
            continue
        if c == "{":
            transparent = bool(re.search(r'(\bnamespace\b[\s\w:]*|\bextern\s*"\s*"\s*)$', text[max(0, i - 80):i]))
            scopes.append(transparent)
            depth += not transparent
        elif c == "}" and scopes:
            depth -= not scopes.pop()
        if c == "\n":
            line_start = True
        elif not c.isspace():
            line_start = False
        i += 1
    return "".join(out)


def function_bodies(text):
    """{name: body text} of every function DEFINED in the source (kernels, helpers, entry points), from stripped text.  A
    definition is `name(...) [const] {` outside every other body; namespaces and extern "C" blocks are looked into."""
    s = _no_directives(strip_c(text))
    out, i, n = {}, 0, len(s)
    while i < n:
        if s[i] != "{":
            i += 1
            continue
        before = s[max(0, i - 80):i]
        if re.search(r'(\bnamespace\b[\s\w:]*|\bextern\s*"\s*"\s*)$', before):
            i += 1                                                            # look inside
            continue
        end = _match(s, i, "{", "}")
        head = s[:i].rstrip()
        m = re.search(r"\)\s*(const\s*)?(noexcept\s*)?$", head)
        if m:
            close = head.rindex(")")
            depth, j = 0, close
            while j >= 0:
                depth += head[j] == ")"
                depth -= head[j] == "("
                if depth == 0:
                    break
                j -= 1
            name = re.search(r"([A-Za-z_]\w*)\s*(<[^;{}()]*>)?\s*$", head[:j])
            if name and name.group(1) not in KEYWORDS:
                out[name.group(1)] = s[i:end + 1]
        i = end + 1
    return out


def _code_after(body, off):
    """The code of the `return` that follows a set_error at `off`: VBQ_ERR_..., or the returned expression."""
    m = re.search(r"\breturn\s+([^;]+);", body[off:])
    return m.group(1).strip() if m else None


def own_refusals(body):
    """[(offset, what)] of the refusals written in this body: VBQ_REQUIRE, set_error + a code other than VBQ_ERR_LAUNCH."""
    found = [(off, "VBQ_REQUIRE") for off, _ in calls(body, "VBQ_REQUIRE")]
    for off, _ in calls(body, "set_error"):
        code = _code_after(body, off)
        if code != "VBQ_ERR_LAUNCH":
            found.append((off, f"set_error -> {code}"))
    return sorted(found)


def analyse(files):
    """-> (bodies {function: (file, body)}, enqueues {function}, refuses {function}) over all sources, closed over calls."""
    bodies = {}
    for fname, text in files.items():
        for name, body in function_bodies(text).items():
            bodies[name] = (fname, body)
    called = {n: {c for c in re.findall(r"(?<![A-Za-z0-9_.>])([A-Za-z_]\w*)\s*(?:<[^;{}()]*>)?\s*\(", b) if c in bodies and c != n}
              for n, (_, b) in bodies.items()}
    enq = {n for n, (_, b) in bodies.items() if any(calls(b, e) for e in ENQUEUE_CALLS)}
    ref = {n for n, (_, b) in bodies.items() if own_refusals(b)}
    grew = True
    while grew:
        grew = False
        for n in bodies:
            if n not in enq and called[n] & enq:
                enq.add(n)
                grew = True
            if n not in ref and called[n] & ref:
                ref.add(n)
                grew = True
    # a helper's `return 1` ("not of this kind") is an answer to its direct caller alone: it does not make the caller a refuser
    ref |= {n for n, (_, b) in bodies.items() if n.startswith("launch_") and re.search(r"\breturn\s+1\s*;", b)}
    return bodies, enq, ref, called


def _calls_of(body, name):
    """Offsets of the calls of `name`, plain or with explicit template arguments."""
    offs = [off for off, _ in calls(body, name)]
    offs += [m.start() for m in re.finditer(r"(?<![A-Za-z0-9_])" + re.escape(name) + r"\s*<[^;{}()]*>\s*\(", body)]
    return sorted(set(offs))


def late_refusals(files):
    """[(file, function, what)]: every refusal that stands after the first enqueue of its function body."""
    bodies, enq, ref, called = analyse(files)
    out = []
    for name, (fname, body) in sorted(bodies.items()):
        first = [off for e in ENQUEUE_CALLS for off, _ in calls(body, e)]
        first += [off for c in called[name] & enq for off in _calls_of(body, c)]
        if not first:
            continue
        first = min(first)
        seen = set()
        for off, what in own_refusals(body):
            if off > first:
                out.append((fname, name, what))
        for c in sorted(called[name] & ref):
            if any(off > first for off in _calls_of(body, c)) and c not in seen:
                seen.add(c)
                out.append((fname, name, c))
    return out


# ------------------------------------------------------------------------------------------------------------------ the table
OWN_HEAD = "its own VBQ_REQUIREs"
BY_LATENTS_CHECK = PREEMPTED + ("latents_call_refusal and " + OWN_HEAD + ": pointers, sizes, grids, N and -- through quantize_kernel_refusal -- "
                                "the kernel of every lambda chunk, asked before the planes are written")
BY_OWN_HEAD = PREEMPTED + OWN_HEAD + ": sizes, pointers, the 32-bit counter bound and n_is_built(N), asked before d_counts is zeroed"
BY_KERNEL_CHECK = PREEMPTED + ("quantize_kernel_refusal -- N built at all, N built for the layout and every lambda chunk's kernel, asked by "
                               "quantize_entry before it dispatches: launch_quantize's own N > 10 refusal, itself ahead of the first chunk, "
                               "cannot be reached (the f32 and the f64 instance are two calls in the text, one at run time)")
EXCEPTIONS = {
    ("quantize_entry", "launch_quantize"): BY_KERNEL_CHECK,
    ("launch_quantize", "launch_level_counts_hull10"): NOT_A_REFUSAL,
    ("launch_quantize", "launch_quant_hull_idx10"): NOT_A_REFUSAL,
    ("launch_quantize", "launch_quant_pruned"): NOT_A_REFUSAL,
    ("launch_notebook", "launch_notebook_hull10"): NOT_A_REFUSAL,
    ("vbq_compress_latents_f32", "vbq_quantize_f32"): BY_LATENTS_CHECK,
    ("vbq_compress_latents_f32", "vbq_gather_latents_u16"): BY_LATENTS_CHECK,
    ("vbq_build_entropy_models_f32", "vbq_level_counts_f32"): BY_LATENTS_CHECK,
    ("vbq_build_entropy_models_f32", "vbq_code_lengths_from_counts"): BY_LATENTS_CHECK,
    ("vbq_build_entropy_models_f32", "vbq_quantize_rows_f32"): BY_LATENTS_CHECK,
    ("vbq_build_entropy_models_f32", "vbq_histogram_models_u16"): BY_LATENTS_CHECK,
    ("vbq_histogram_models_u16", "vbq_histogram_rows_u16"): BY_OWN_HEAD,
    ("vbq_histogram_models_u16", "vbq_code_lengths_from_counts"): BY_OWN_HEAD,
}
"""(function, what) -> reason.  `what` is the callee's name, "VBQ_REQUIRE" or "set_error -> <code>"."""


# ------------------------------------------------------------------------------------------------------------------ self-tests
PLANTED = """
#define OUTSIDE(x) { hipLaunchKernelGGL(k, g, b, 0, st, x); }
namespace vbq {
namespace {
struct S { int a; };
__global__ void k_one(float *x) { x[0] = 1; }
int launch_maybe(int L, hipStream_t st) {
    if (L > 4) return 1;
    hipLaunchKernelGGL(k_one, dim3(1), dim3(64), 0, st, nullptr);
    VBQ_CHECK_LAUNCH("one");
    return VBQ_OK;
}
template <int N>
int launch_always(float *x, hipStream_t st) {
    hipLaunchKernelGGL(k_one, dim3(1), dim3(64), 0, st, x);
    return VBQ_OK;
}
}  // namespace
}  // namespace vbq
extern "C" size_t vbq_bytes(int n) { return n; }
extern "C" int vbq_inner(float *d_x, int n, void *stream) {
    VBQ_REQUIRE(n > 0, VBQ_ERR_INVALID_ARGUMENT, "vbq_inner: n");
    hipLaunchKernelGGL(k_one, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), d_x);
    if (bad) { set_error("late but a launch failure"); return VBQ_ERR_LAUNCH; }
    return VBQ_OK;
}
extern "C" int vbq_good(float *d_x, int n, void *stream) {
    VBQ_REQUIRE(n > 0, VBQ_ERR_INVALID_ARGUMENT, "vbq_good: n");
    if (n > 9) { set_error("vbq_good: large"); return VBQ_ERR_UNSUPPORTED; }
    const size_t b = vbq_bytes(n);
    return launch_always<4>(d_x, reinterpret_cast<hipStream_t>(stream));
}
"""


def test_the_parser_reads_a_planted_source():
    bodies = function_bodies(PLANTED)
    assert sorted(bodies) == ["k_one", "launch_always", "launch_maybe", "vbq_bytes", "vbq_good", "vbq_inner"]
    assert "OUTSIDE" not in _no_directives(strip_c(PLANTED))
    _, enq, ref, _ = analyse({"p.hip": PLANTED})
    assert enq == {"launch_maybe", "launch_always", "vbq_inner", "vbq_good"} and ref == {"launch_maybe", "vbq_inner", "vbq_good"}
    assert late_refusals({"p.hip": PLANTED}) == []


@pytest.mark.parametrize("planted,what", [
    ("hipMemsetAsync(d_x, 0, 4, st);\n    VBQ_REQUIRE(n < 5, VBQ_ERR_UNSUPPORTED, \"late\");", "VBQ_REQUIRE"),
    ("launch_always<4>(d_x, st);\n    if (n == 3) { set_error(\"late\"); return VBQ_ERR_UNSUPPORTED; }", "set_error -> VBQ_ERR_UNSUPPORTED"),
    ("launch_always<4>(d_x, st);\n    if (n == 3) { set_error(\"late\"); return rc; }", "set_error -> rc"),
    ("hipLaunchKernelGGL(k_one, dim3(1), dim3(64), 0, st, d_x);\n    return vbq_inner(d_x, n, stream);", "vbq_inner"),
    ("int rc = vbq_inner(d_x, n, stream);\n    if (rc) return rc;\n    return vbq_inner(d_x, n - 1, stream);", "vbq_inner"),
    ("hipMemcpyAsync(d_x, d_x, 4, hipMemcpyDeviceToDevice, st);\n    return launch_maybe(n, st);", "launch_maybe"),
])
def test_each_rule_fails_on_a_planted_late_refusal(planted, what):
    text = PLANTED + "\nextern \"C\" int vbq_late(float *d_x, int n, void *stream) {\n    hipStream_t st = " \
        "reinterpret_cast<hipStream_t>(stream);\n    " + planted + "\n    return VBQ_OK;\n}\n"
    assert late_refusals({"p.hip": text}) == [("p.hip", "vbq_late", what)]
    quiet = PLANTED + "\n// " + planted.replace("\n", "\n// ") + "\n"
    assert late_refusals({"p.hip": quiet}) == []


# ------------------------------------------------------------------------------------------------------------------ the sources
def test_no_refusal_stands_after_the_first_enqueue():
    files = {n: t for n, t in sources().items()}
    bodies, enq, ref, called = analyse(files)
    assert len(bodies) >= 300 and len(enq) >= 80 and len(ref) >= 90, (len(bodies), len(enq), len(ref))
    for must in ("quantize_entry", "vbq_build_entropy_models_f32", "vbq_compress_latents_f32", "launch_quant_pruned", "gather_latents"):
        assert must in bodies and must in enq and must in ref, must
    assert "launch_quantize" in enq and "quantize_kernel_refusal" in ref and "quantize_kernel_refusal" not in enq
    found = late_refusals(files)
    unlisted = [f for f in found if (f[1], f[2]) not in EXCEPTIONS]
    assert not unlisted, ("refusals after the first enqueue of their function (move them before it, or list them in EXCEPTIONS with "
                          "one of the two reasons):\n" + "\n".join("  %s: %s: %s" % f for f in unlisted))
    stale = sorted(k for k in EXCEPTIONS if k not in {(f[1], f[2]) for f in found})
    assert not stale, f"EXCEPTIONS lists sites that are no longer late refusals: {stale}"


def test_every_exception_carries_one_of_the_two_reasons():
    files = sources()
    bodies, _, _, _ = analyse(files)
    for (function, what), reason in EXCEPTIONS.items():
        assert reason == NOT_A_REFUSAL or (reason.startswith(PREEMPTED) and len(reason) > len(PREEMPTED)), (function, what, reason)
        if reason == NOT_A_REFUSAL:
            # the helper refuses nothing: no VBQ_REQUIRE, no set_error but a launch failure's -- only `return 1`
            assert what.startswith("launch_") and not own_refusals(bodies[what][1]) and re.search(r"\breturn\s+1\s*;", bodies[what][1]), \
                (function, what)
        else:
            # the named check: a function that exists, can refuse, enqueues nothing and is called before the inner call -- or the
            # function's own VBQ_REQUIREs, of which some stand before its first enqueue
            check = reason[len(PREEMPTED):].split(" ")[0]
            body = bodies[function][1]
            if reason[len(PREEMPTED):].startswith(OWN_HEAD):
                first = min(off for e in ENQUEUE_CALLS for off, _ in calls(body, e))
                assert [off for off, w in own_refusals(body) if w == "VBQ_REQUIRE" and off < first], function
                continue
            assert check in bodies and own_refusals(bodies[check][1]), (function, what, check)
            assert not any(calls(bodies[check][1], e) for e in ENQUEUE_CALLS), check
            at = _calls_of(body, check)
            assert at and at[0] < min(_calls_of(body, what)), f"{function} does not call {check} before {what}"
