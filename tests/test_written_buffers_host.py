"""tests/written_buffers.py against the headers and the code (no GPU needed).

The enumeration: WRITTEN, read from the five headers, is every key of BINDING and nothing else; no key stands twice in the
table's text; every ARG and HANDED row names a function and a parameter that exist.

The code, by a walk of every call site of every entry point (as tests/test_stream_order_host.py walks them for the stream):
  * the expression at every written position is `_ptr(e)` / `ops._ptr(e)` or None;
  * `e` traces back, through assignments, tuple results of the module's helpers and the callbacks a helper calls, to the shared
    written-buffer check applied to the parameter the row names (ARG), to a private helper's parameter (HANDED: every call of
    the helper hands it a new tensor), or to torch.empty / zeros / full (INTERNAL) -- at EVERY call site, not at one;
  * and never to `_dev(`, `.contiguous()`, `.to(`, `.reshape(` or `.clone()`: those may copy, and a kernel that writes into a
    copy leaves the caller's tensor as it was.
The walk is by text, not by control flow: an `if` is followed into both branches (the two branches of one `if` do not see each
other's assignments), a loop is not unrolled.  Every rule is tried on planted text first: a planted `status = _dev(status, ...)`
and a planted unchecked `out` are reported.

The pure half of the check itself -- ops._laid_out and ops._apart read strides, addresses and sizes only -- runs here on host
tensors: stride-0 views, every second element, one-element tensors with a foreign stride, ranges that touch but do not
intersect."""
import ast
import os
import re

import pytest

import written_buffers as WB

torch = pytest.importorskip("torch")


def _read(rel):
    with open(os.path.join(WB.ROOT, rel), encoding="utf-8") as f:
        return f.read()


@pytest.fixture(scope="module")
def positions():
    out = {}
    for entry, i, param in WB.written():
        out.setdefault(entry, {})[i] = param
    return out


@pytest.fixture(scope="module")
def modules():
    return {name: WB.Module(name, text) for name, text in WB.package_sources().items()}


# ------------------------------------------------------------------------------------------------------------------ the headers
PLANTED_HEADER = """
/* int vbq_gone(float *d_x, void *stream); */
int vbq_a_f32(const float *d_x, int64_t n,   // a comment, with a comma and a float *d_y
              float *d_out, uint32_t *d_status, void *stream);
size_t vbq_a_workspace_bytes(int64_t n);
int vbqx_b_u16(const uint16_t *d_idx, void *d_workspace, size_t workspace_bytes, const double h_l[], int64_t h_grid[], void *stream);
const char *vbq_last_error(void);
"""


def test_the_header_parser_reads_a_planted_header():
    assert WB.written_params(PLANTED_HEADER) == [("vbq_a_f32", 2, "d_out"), ("vbq_a_f32", 3, "d_status"),
                                                 ("vbqx_b_u16", 1, "d_workspace"), ("vbqx_b_u16", 4, "h_grid")]
    assert WB.declarations(PLANTED_HEADER)["vbq_last_error"] == [] and "vbq_gone" not in WB.declarations(PLANTED_HEADER)


def test_written_is_what_the_five_headers_declare(positions):
    from test_abi import declared_functions
    found = WB.written()
    assert len(found) >= 190 and len(positions) >= 86, (len(found), len(positions))
    assert len(set(found)) == len(found)
    main = {e for e in positions if e.startswith("vbq_")}
    assert main <= set(declared_functions())
    assert {e[:5] for e in positions if not e.startswith("vbq_")} == {"vbqx_", "vbqb_", "vbqk_", "vbqs_"}
    for must in (("vbq_moments_f32", 4, "d_out"), ("vbq_bmshj_icdf_chain_f32", 7, "d_flags"), ("vbqs_plan_boxes", 13, "d_status"),
                 ("vbq_rans_il_decode_files_u16", 13, "d_idx"), ("vbqb_budget_sweep_f64", 11, "d_workspace")):
        assert must in found, must
    assert not [f for f in found if f[2] == "stream"]


def test_every_written_pair_is_in_the_table_exactly_once():
    pairs = {(e, p) for e, _, p in WB.written()}
    assert set(WB.BINDING) == pairs, (sorted(pairs - set(WB.BINDING)), sorted(set(WB.BINDING) - pairs))
    # a dict display keeps the last of two equal keys without a word: count them in the text
    tree = ast.parse(_read("tests/written_buffers.py"))
    table = next(n.value for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "BINDING")
    keys = [ast.literal_eval(k) for k in table.keys]
    assert len(keys) == len(set(keys)) == len(pairs)
    for pair, rows in WB.BINDING.items():
        assert rows and len(rows) == len(set(rows)), pair
        for r in rows:
            assert r in (WB.INTERNAL, WB.HOST, WB.COMM) or (isinstance(r, tuple) and r[0] in ("ARG", "HANDED")), (pair, r)
        if WB.HOST in rows or WB.COMM in rows:
            assert len(rows) == 1, pair
    for pair in [p for p, rows in WB.BINDING.items() if WB.HOST in rows]:
        assert pair[0].startswith("vbq_host_") or pair[1].startswith("h_") or pair[1] == "buf", pair
    for pair in [p for p, rows in WB.BINDING.items() if WB.COMM in rows]:
        assert pair[0].startswith("vbq_comm_") or pair[0] == "vbq_allreduce_hist", pair           # as tests/footprint.py has them


def test_every_row_names_a_function_and_a_parameter_that_exist(modules):
    rows = [r for rs in WB.BINDING.values() for r in rs if isinstance(r, tuple)]
    assert len(WB.arg_rows()) >= 85 and len(rows) > len(WB.arg_rows())
    for kind, face, param, via in rows:
        mod, _, qual = face.partition(".")
        assert mod in modules and qual in modules[mod].functions, face
        assert param in WB._params(modules[mod].functions[qual]), (face, param)
        assert (kind == "HANDED") == qual.split(".")[-1].startswith("_"), f"{face}: a private helper is HANDED, a public face an ARG"
        if via and via.startswith("@"):
            tmod, _, tqual = via[1:].partition(".")
            assert tmod == mod and tqual.split(".")[0] == qual.split(".")[0] and tqual in modules[tmod].functions, via
        elif via:
            target, keyword = via.split(":")
            tmod, _, tqual = target.partition(".")
            assert keyword in WB._params(modules[tmod].functions[tqual]), via
    # the faces the issue names
    faces = {f for _, _, f, _, _ in WB.arg_rows()}
    for must in ("ops.moments", "ops.rd_sums", "ops.bmshj_nll_grad", "ops.numpy_row_sums", "ops.bmshj_icdf_step", "ops.bmshj_icdf_chain",
                 "kmeans1d.kmeans1d_dp", "coder.RansCodec.unpack_device", "store.plan_boxes", "store.LatentStore.crops",
                 "dist.CountsAllReduce.start"):
        assert must in faces, must


def test_in_place_names_arg_rows_and_quotes_the_header(positions):
    args = {(e, p) for e, p, _, _, _ in WB.arg_rows()}
    where = {}
    for h in WB.HEADERS:
        text = re.sub(r"\s*\n\s*\*?\s*", " ", _read(h))
        for e in WB.declarations(_read(h)):
            where[e] = text
    for pair, (kind, words) in WB.IN_PLACE.items():
        assert pair in args, f"{pair}: IN_PLACE is about buffers a caller can supply"
        assert kind in ("state", "add", "or", "keep") and words in where[pair[0]], (pair, words)
    # every status a caller can hand in is OR-ed into, and says so
    for e, p in args:
        if p == "d_status":
            assert WB.IN_PLACE.get((e, p), ("",))[0] == "or", (e, p)
    main = _read("include/vbq.h")
    assert "/* Buffers." in main and "must not overlap anything else the call reads or writes" in main
    for h in WB.HEADERS[1:]:
        assert 'vbq.h, "Buffers"' in _read(h), h


# ------------------------------------------------------------------------------------------------------------------ the walk
PLANTED_POSITIONS = {"vbq_a_f32": {2: "d_out", 3: "d_status"}, "vbqx_b_u16": {1: "d_workspace"}}
PLANTED_BINDING = {
    ("vbq_a_f32", "d_out"): [WB.ARG("m.a", "out"), WB.HANDED("m.K._run", "buf"), WB.INTERNAL],
    ("vbq_a_f32", "d_status"): [WB.ARG("m.a", "status"), WB.INTERNAL],
    ("vbqx_b_u16", "d_workspace"): [WB.ARG("m.b", "workspace")],
}
PLANTED_PY = '''
def _args(x, out, status):
    x = _dev(x, torch.float32, "x")
    out = _out(out, (3,), torch.float32, x.device, "out", True, (("x", x),))
    if status is not None:
        status = _status(status, 1, x.device)
    return x, out, status


def a(x, out=None, status=None):
    """docstring naming lib.vbq_a_f32(x, 1, out, None)"""
    x, out, status = _args(x, out, status)
    check(_lib.lib().vbq_a_f32(_ptr(x), x.numel(),          # a comment, _ptr(y)
                               _ptr(out), _ptr(status), _stream(x)), "vbq_a_f32")
    out = out.reshape(-1)                                   # after the call: the result's shape, not the library's pointer
    return out


def b(idx, workspace=None):
    ws = ops._workspace(workspace, 16, idx.device)
    check(h.vbqx_b_u16(ops._ptr(idx), ops._ptr(ws), 16, None, None, ops._stream(idx)), "vbqx_b_u16")


def fresh(x):
    if x.numel():
        out = torch.zeros(3, dtype=torch.float32, device=x.device).view(3)
    else:
        out = torch.empty(3, dtype=torch.float32, device=x.device)
    both = torch.empty(4, dtype=torch.uint8, device=x.device)
    check(lib.vbq_a_f32(_ptr(x), 3, _ptr(out), _ptr(both[:4].view(torch.uint32)) if x.numel() else None, _stream(x)), "vbq_a_f32")


class K:
    def _done(self, n, launch):
        out = torch.empty(n, dtype=torch.float32, device="cuda")
        launch(out)
        return out

    def _run(self, x, buf):
        check(lib.vbq_a_f32(_ptr(x), 3, _ptr(buf), None, _stream(x)), "vbq_a_f32")

    def go(self, x):
        return self._done(3, lambda buf: self._run(x, buf))

    def again(self, x):
        def launch(buf):
            self._run(x, buf)
        return self._done(3, launch)
'''


def _walk(text, binding=PLANTED_BINDING):
    mods = {"m": WB.Module("m", text)}
    seen, bad, used = WB.violations(mods, PLANTED_POSITIONS, binding)
    return seen, bad + WB.handed_violations(mods, binding)[1], used


def test_the_walk_reads_a_planted_module():
    seen, bad, used = _walk(PLANTED_PY)
    assert seen == 4 and bad == [], bad
    assert {(u[3], u[4]) for u in used} == {("m.a", "out"), ("m.a", "status"), ("m.b", "workspace"), ("m.K._run", "buf")}
    assert WB.handed_violations({"m": WB.Module("m", PLANTED_PY)}, PLANTED_BINDING)[0] == 2


@pytest.mark.parametrize("good,planted,expect", [
    # what this suite was written for
    ("        status = _status(status, 1, x.device)", "        status = _dev(status, torch.uint32, 'status')", "copy: _dev"),
    ('    out = _out(out, (3,), torch.float32, x.device, "out", True, (("x", x),))', "    pass", "does not reach the library through the shared check"),
    # the other ways to a copy
    ('    x, out, status = _args(x, out, status)', "    x, out, status = _args(x, out, status)\n    out = out.contiguous()", "copy: .contiguous"),
    ('    x, out, status = _args(x, out, status)', "    x, out, status = _args(x, out, status)\n    status = status.to(x.device)", "copy: .to"),
    ('    x, out, status = _args(x, out, status)', "    x, out, status = _args(x, out, status)\n    out = out.reshape(-1)", "copy: .reshape"),
    ('    x, out, status = _args(x, out, status)', "    x, out, status = _args(x, out, status)\n    out = out.clone()", "copy: .clone"),
    ("    ws = ops._workspace(workspace, 16, idx.device)", "    ws = workspace", "does not reach the library through the shared check"),
    ("    ws = ops._workspace(workspace, 16, idx.device)", "    ws = ops._workspace(workspace.contiguous(), 16, idx.device)", "other: check of"),
    # not a pointer of a tensor at all, and a site no row covers
    ("_ptr(out), _ptr(status), _stream(x)), \"vbq_a_f32\")", "C.c_void_p(out.data_ptr()), _ptr(status), _stream(x)), \"vbq_a_f32\")", "not _ptr(...)"),
    ("def fresh(x):", "def fresh(x, out=None):", None),                                      # (harmless: both branches assign it)
    ("def fresh(x):\n    if x.numel():\n        out = torch.zeros(3, dtype=torch.float32, device=x.device).view(3)\n    else:",
     "def fresh(x, out=None):\n    if out is not None:\n        pass\n    else:", "param: out"),            # an unchecked `out`, INTERNAL row
    ("        out = torch.empty(n, dtype=torch.float32, device=\"cuda\")", "        out = self.kept", "other: self.kept"),
    ("        return self._done(3, lambda buf: self._run(x, buf))", "        return self._run(x, x)", "param: x"),
])
def test_the_walk_reports_a_planted_defect(good, planted, expect):
    assert PLANTED_PY.count(good) == 1, good
    seen, bad, _ = _walk(PLANTED_PY.replace(good, planted))
    assert seen == 4
    if expect is None:
        assert bad == [], bad
    else:
        assert bad and any(expect in b for b in bad), (planted, bad)
    # and the same text in a comment or a docstring is none
    assert _walk(PLANTED_PY + "\n# " + planted.replace("\n", "\n# ") + '\n"""' + planted + '"""\n')[1] == []


def test_internal_holds_for_every_call_site_not_for_one():
    second = PLANTED_PY + "\n\ndef elsewhere(x, out):\n    check(lib.vbq_a_f32(_ptr(x), 3, _ptr(out), None, _stream(x)), 'vbq_a_f32')\n"
    seen, bad, _ = _walk(second)
    assert seen == 5 and any("m.elsewhere" in b and "param: out" in b for b in bad), bad
    no_internal = {k: [r for r in v if r != WB.INTERNAL] for k, v in PLANTED_BINDING.items()}
    seen, bad, _ = _walk(PLANTED_PY, no_internal)
    assert any("m.fresh" in b and "no row of BINDING covers this call site" in b for b in bad), bad


def test_every_call_site_of_the_package_keeps_the_table(modules, positions):
    seen, bad, used = WB.violations(modules, positions, WB.BINDING)
    assert not bad, "\n".join(bad)
    assert seen >= 85, seen
    called = {entry for _, _, entry, _ in WB.sites(modules, positions)}
    uncalled = set(positions) - called
    assert uncalled == {"vbq_solve_grid", "vbq_device_name", "vbq_host_stage_run"}, sorted(uncalled)       # (reached through _lib.py)
    direct = {(e, p, "ARG", face, name) for e, p, face, name, via in WB.arg_rows() if not via or via.startswith("@")}
    handed = {(e, p, "HANDED", r[1], r[2]) for (e, p), rows in WB.BINDING.items() for r in rows if isinstance(r, tuple) and r[0] == "HANDED"}
    assert (direct | handed) == used, sorted((direct | handed) ^ used)
    n, bad = WB.handed_violations(modules, WB.BINDING)
    assert not bad and n >= 30, (n, bad)
    n, bad = WB.via_violations(modules, WB.BINDING)
    assert not bad and n >= 5, (n, bad)
    for (face, name), entries in WB.ALIASED.items():
        assert all(e in positions for e in entries)
    for (face, expr), why in WB.UPLOADS.items():
        mod, _, qual = face.partition(".")
        assert expr in ast.unparse(modules[mod].functions[qual]) and len(why.split()) >= 4, face


@pytest.mark.parametrize("good,planted,expect", [
    ('status = _status(status, 1, fhat.device, (("fhat", fhat),))\n    h = _lib.lib()', 'status = _dev(status, torch.uint32, "status")\n    h = _lib.lib()',
     "ops.budget_dp: vbq_budget_dp_f64(d_status): copy: _dev"),
    ('        out = _out(out, (Cc, 2), torch.float64, x.device, "out", True, (("x", x),))', "        pass",
     "ops.moments: vbq_moments_f32(d_out): `out` does not reach the library through the shared check"),
    ('        status = _status(status, F, idx.device, (("idx", idx), ("files", files), ("items", items), ("freq", freq)))',
     '        status = _dev(status, torch.uint32, "status")', "ops.rans_il_decode_files: vbq_rans_il_decode_files_u16(d_status): copy: _dev"),
    ("    ws = _workspace(workspace, wsb, x.device, 4, ((\"x\", x),))", "    ws = workspace if workspace is not None else torch.empty(4)",
     "ops.numpy_row_sums: vbq_numpy_row_sums_f32(d_workspace): `workspace` does not reach"),
])
def test_the_plants_of_the_issue_are_reported_in_the_real_source(positions, good, planted, expect):
    text = WB.package_sources()["ops"]
    assert text.count(good) == 1, good
    mods = {"ops": WB.Module("ops", text.replace(good, planted))}
    _, bad, _ = WB.violations(mods, positions, WB.BINDING)
    assert any(b.startswith(expect) for b in bad), bad


def test_no_written_buffer_goes_through_an_input_check_anywhere(modules, positions):
    """The eighteen sites of the issue, by name: no `status`, `sizes`, `words`, `totals`, `workspace` or `out*` that reaches a
    written position is bound from _dev."""
    origins = WB.Origins(modules)
    for mod, face, entry, call in WB.sites(modules, positions):
        for pos, param in positions[entry].items():
            arg = call.args[pos] if pos < len(call.args) else None
            if isinstance(arg, ast.Call) and WB._callee(arg) == "_ptr":
                assert not [o for o in origins.of(mod, arg.args[0], 0, call) if o[0] == "copy"], (face, entry, param)


# ------------------------------------------------------------------------------------------------------------------ the check
def test_laid_out_reads_the_strides_not_is_contiguous():
    from vbq_amd import ops
    wide = torch.zeros((4, 6))
    assert ops._laid_out(wide) and ops._laid_out(wide[1:3]) and ops._laid_out(wide.view(2, 2, 6)) and ops._laid_out(torch.zeros(()))
    assert ops._laid_out(torch.zeros((0, 3))) and ops._laid_out(torch.zeros((3, 0))) and ops._laid_out(torch.zeros((3, 1, 2)))
    assert not ops._laid_out(wide[:, ::2]) and not ops._laid_out(wide.t()) and not ops._laid_out(wide[:, :3])
    assert not ops._laid_out(torch.zeros(1).expand(5)) and not ops._laid_out(torch.zeros((1, 6)).expand(4, 6))
    one = torch.zeros(2)[::2]                                            # one element, stride 2: "contiguous" to torch
    assert one.is_contiguous() and tuple(one.shape) == (1,) and not ops._laid_out(one)
    column = torch.zeros((3, 2))[:, :1]
    assert column.numel() == 3 and not ops._laid_out(column)


def test_apart_is_half_open_interval_arithmetic():
    from vbq_amd import ops
    raw = torch.zeros(64, dtype=torch.uint8)
    a, b = raw[:16].view(torch.float32), raw[16:32].view(torch.float32)          # back to back: b starts at a's last byte + 1
    assert b.data_ptr() == a.data_ptr() + 16
    ops._apart("out", b, (("x", a),))
    ops._apart("out", a, (("x", b), ("none", None), ("empty", raw[:0]), ("empty too", raw[8:8])))
    ops._apart("out", raw[8:8], (("x", raw),))                                     # an empty tensor intersects nothing
    for other in (raw[12:20], raw[15:16], raw[:1], raw[:64], a, raw[4:8].view(torch.int16)):
        with pytest.raises(ValueError, match=r"^out overlaps x: a tensor the call writes must share no memory with anything else"):
            ops._apart("out", a, (("first", b), ("x", other)))
    with pytest.raises(ValueError, match="^status overlaps out_mu: "):
        ops._apart("status", raw[28:32].view(torch.uint32), (("out_mu", b),))


def test_the_checks_refuse_on_the_host_what_needs_no_device():
    """Everything but the device test itself can be seen on host tensors: they are refused for being host tensors, in the one
    wording, whatever else is right or wrong with them."""
    from vbq_amd import ops
    for given in (torch.zeros((2, 3)), torch.zeros((2, 3), dtype=torch.float64), torch.zeros(6), "no tensor", 3):
        with pytest.raises(ValueError, match=r"^out: expected a contiguous torch\.float32 device tensor of shape \(2, 3\)$"):
            ops._out(given, (2, 3), torch.float32, None, "out")
    with pytest.raises(ValueError, match=r"^status: expected a contiguous torch\.uint32 device tensor of shape \(1,\)$"):
        ops._status(torch.zeros(0, dtype=torch.uint32), 1, None)
    with pytest.raises(ValueError, match=r"^workspace must be a device tensor of at least 8 bytes$"):
        ops._workspace(torch.zeros(8, dtype=torch.uint8), 8, None)
    assert ops._out(None, (2, 3), torch.float32, "cpu", "out", False) is None and ops._status(None, 1, "cpu") is None
