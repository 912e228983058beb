"""Every buffer the native libraries write, and how a caller of the Python binding reaches it.

WRITTEN is read from the five headers: every (entry point, parameter) whose pointer is not `const`, the stream left out.
BINDING maps each pair to the rows that say where its memory comes from:

    ARG(face, param)        `face` ("module.function" or "module.Class.method" under vbq_amd) has the parameter `param` through
                            which a caller can supply the buffer; it passes the shared written-buffer check (vbq_amd/ops.py:
                            _out, _status, _workspace) in that function and its pointer goes to the library as it came.
                            ARG(face, param, via="module.function:keyword") is a face that hands the checked tensor, or a
                            slice or view of it, to another face instead of to the library; via="@module.Class.method" one
                            that keeps the checked tensor in an attribute of its object, from where that other method of
                            the class hands it to the library.
    HANDED(face, param)     `face` is a private helper (its name starts with an underscore) that takes the buffer from its
                            callers inside the package, and every one of them hands it a new tensor.
    INTERNAL                the binding allocates it (torch.empty / zeros / full) at every call site no other row covers.
    HOST, COMM              as in tests/footprint.py: host memory, or a communicator's.

A function with several Python faces has one row per face.  IN_PLACE names the pairs whose EARLIER CONTENT the call reads, with
the sentence of the header that says so: these are the only overlaps include/vbq.h ("Buffers") allows, and each is a buffer
with itself -- no entry point allows two different arguments to share memory.

THE RULE: a new entry point with a non-const pointer, or a new Python parameter that reaches one, goes into BINDING;
tests/test_written_buffers_host.py holds the table against the headers and, by a walk of the call sites, against the code;
tests/test_gpu_written_buffers.py runs every ARG row.  Importable without a GPU."""
import ast
import os
import re

from footprint import COMM, HOST  # noqa: F401  (the two reasons, in footprint's words)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.join(ROOT, "vbq_amd")
HEADERS = ("include/vbq.h", "include/vbq_ext.h", "include/vbq_budget.h", "include/vbq_kmeans.h", "vbq_amd/store/vbq_store.h")
ENTRY = r"vbq[a-z]?_[a-z0-9_]+"
INTERNAL = "allocated by the binding at every call site"


def ARG(face, param, via=None):
    return ("ARG", face, param, via)


def HANDED(face, param):
    return ("HANDED", face, param, None)


# ------------------------------------------------------------------------------------------------------------------ the headers
def _strip_c(text):
    """Comments blanked (the headers hold no string literals with comment marks in them)."""
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    return re.sub(r"//[^\n]*", lambda m: " " * len(m.group(0)), text)


def declarations(header_text):
    """{entry point: [parameter declarations]} of every function the header declares."""
    s, out = _strip_c(header_text), {}
    for m in re.finditer(r"\b(" + ENTRY + r")\s*\(", s):
        depth, start, args = 0, m.end(), []
        for i in range(m.end() - 1, len(s)):
            depth += s[i] == "("
            depth -= s[i] == ")"
            if depth == 0 or (s[i] == "," and depth == 1):
                args.append(" ".join(s[start:i].split()))
                start = i + 1
                if depth == 0:
                    break
        out[m.group(1)] = [a for a in args if a and a != "void"]
    return out


def written_params(header_text):
    """[(entry point, position, parameter name)] of every pointer parameter that is not const and is not the stream."""
    out = []
    for fn, args in declarations(header_text).items():
        for i, a in enumerate(args):
            if ("*" in a or "[" in a) and not re.search(r"\bconst\b", a) and not re.fullmatch(r"void\s*\*\s*stream", a):
                out.append((fn, i, re.search(r"(\w+)\s*(\[\s*\])?$", a).group(1)))
    return out


def written():
    out = []
    for h in HEADERS:
        with open(os.path.join(ROOT, h), encoding="utf-8") as f:
            out += written_params(f.read())
    return out


# ------------------------------------------------------------------------------------------------------------------ the sources
CHECKS = ("_out", "_status", "_workspace")
FRESH = ("empty", "zeros", "full", "empty_like", "zeros_like", "full_like")
COPIES = ("contiguous", "to", "reshape", "clone", "cpu", "cuda", "float", "double", "long", "int", "flatten", "ravel")
VIEWS = ("view",)
CACHES = ("kept", "_kept")
"""Calls that keep what a factory made: kept(key, lambda: torch.empty(...)) is the factory's tensor."""
UPLOADS = {("quantizer.ChannelwisePriorCDFQuantizer._encode_batch_upload", "b.host.to(dev)"):
           "the plan's host array, uploaded: the device tensor is new at every call"}
"""(function, expression) -> why the expression is a new device tensor although the walk cannot see an allocation."""
ALIASED = {("ops.histogram", "fn"): ("vbq_histogram_u16", "vbq_histogram_u16_i32")}
"""(function, local name) -> the entry points that are called through that name there."""


def package_sources():
    out = {}
    for base, _, files in os.walk(PACKAGE):
        for fn in files:
            if fn.endswith(".py"):
                path = os.path.join(base, fn)
                mod = os.path.relpath(path, PACKAGE)[:-3].replace(os.sep, ".")
                mod = mod[:-len(".__init__")] if mod.endswith(".__init__") else mod
                with open(path, encoding="utf-8") as f:
                    out[mod] = f.read()
    return out


class Module:
    """One parsed module: its functions by qualified name ("f", "Class.f"), each node knowing its parent."""

    def __init__(self, name, text):
        self.name, self.tree, self.functions = name, ast.parse(text), {}
        for node in ast.walk(self.tree):
            for child in ast.iter_child_nodes(node):
                child.parent = node
        for node in self.tree.body:
            if isinstance(node, ast.FunctionDef):
                self.functions[node.name] = node
            elif isinstance(node, ast.ClassDef):
                for sub in node.body:
                    if isinstance(sub, ast.FunctionDef):
                        self.functions[node.name + "." + sub.name] = sub

    def owner(self, node):
        """(qualified name, FunctionDef) of the module- or class-level function a node stands in."""
        chain = []
        while node is not None:
            if isinstance(node, ast.FunctionDef):
                chain.append(node)
            node = getattr(node, "parent", None)
        top = chain[-1]
        for q, f in self.functions.items():
            if f is top:
                return q, f
        raise AssertionError(f"{self.name}: {top.name} is no module- or class-level function")


def _callee(call):
    """The name a call goes through: `f(...)` -> "f", `a.b.f(...)` -> "f"."""
    return call.func.id if isinstance(call.func, ast.Name) else call.func.attr if isinstance(call.func, ast.Attribute) else None


def _params(fdef):
    a = fdef.args
    return [x.arg for x in a.posonlyargs + a.args] + [x.arg for x in a.kwonlyargs]


def _positional(fdef):
    names = [x.arg for x in fdef.args.posonlyargs + fdef.args.args]
    return names[1:] if names[:1] in (["self"], ["cls"]) else names


def _scopes(node):
    """The lambdas and functions around a node, innermost first."""
    out = []
    while node is not None:
        if isinstance(node, (ast.Lambda, ast.FunctionDef)):
            out.append(node)
        node = getattr(node, "parent", None)
    return out


def _ancestors(node):
    out = []
    while getattr(node, "parent", None) is not None:
        node = node.parent
        out.append(node)
    return out


def _exclusive(a, b):
    """The two nodes stand in the two branches of one `if`: what one binds the other never sees."""
    up_a, up_b = [a] + _ancestors(a), [b] + _ancestors(b)
    for i in (n for n in up_a if isinstance(n, ast.If) and n in up_b):
        in_body = lambda chain: any(x in chain for x in i.body)
        in_else = lambda chain: any(x in chain for x in i.orelse)
        if (in_body(up_a) and in_else(up_b)) or (in_else(up_a) and in_body(up_b)):
            return True
    return False


def _binds(stmt, name):
    """The statement assigns `name` on every path through it: an assignment, or an `if` whose two branches both do."""
    if isinstance(stmt, ast.Assign):
        return any(isinstance(t, ast.Name) and t.id == name for target in stmt.targets for t, _ in _targets(target))
    if isinstance(stmt, ast.If):
        return any(_binds(x, name) for x in stmt.body) and any(_binds(x, name) for x in stmt.orelse)
    return False


def _rebound(fdef, name, limit):
    """A parameter is no longer what the caller gave once a statement of the function's own body has assigned it on every path
    (before the position `limit`, where there is one)."""
    return any(_binds(stmt, name) for stmt in fdef.body if limit is None or (stmt.end_lineno, stmt.end_col_offset) <= limit)


def _targets(t):
    if isinstance(t, (ast.Tuple, ast.List)):
        return [(e, (i,) + rest) for i, x in enumerate(t.elts) for e, rest in _targets(x)]
    return [(t, ())]


class Origins:
    """Where the memory behind an expression comes from: a set of
    ("check", param)   the shared check, applied to the function's own parameter `param`
    ("fresh",)         a new tensor, or a view or slice of one
    ("none",)          None
    ("param", name)    a parameter of the module- or class-level function, as it came
    ("copy", what)     something that may copy: _dev(...), .contiguous(), .to(...), .reshape(...), .clone()
    ("other", text)    anything else."""

    def __init__(self, modules):
        self.modules = modules

    # ---- expressions
    def of(self, mod, expr, depth=0, before=None):
        assert depth < 12, ast.unparse(expr)
        if isinstance(expr, ast.Constant) and expr.value is None:
            return {("none",)}
        if isinstance(expr, ast.IfExp):
            return self.of(mod, expr.body, depth + 1, before) | self.of(mod, expr.orelse, depth + 1, before)
        if isinstance(expr, ast.Subscript):
            return self.of(mod, expr.value, depth + 1, before)
        if isinstance(expr, ast.Name):
            return self.name(mod, expr, expr.id, depth + 1, before)
        if isinstance(expr, ast.Attribute) and isinstance(expr.value, ast.Name) and expr.value.id == "self":
            return self.attribute(mod, expr, depth + 1)
        if isinstance(expr, ast.ListComp):
            return self.of(mod, expr.elt, depth + 1, before)
        if (mod.name + "." + mod.owner(expr)[0], ast.unparse(expr)) in UPLOADS:
            return {("fresh",)}
        if isinstance(expr, ast.Call):
            callee = _callee(expr)
            if callee in CACHES and expr.args and isinstance(expr.args[-1], ast.Lambda):
                return self.of(mod, expr.args[-1].body, depth + 1)
            if callee in CHECKS and expr.args:
                given = expr.args[0]
                if isinstance(given, ast.Constant) and given.value is None:
                    return {("fresh",), ("none",)}
                if isinstance(given, ast.Name):
                    inner = self.name(mod, given, given.id, depth + 1, before=before or expr)
                    if inner <= {("param", given.id), ("none",)} and ("param", given.id) in inner:
                        return {("check", given.id)}
                    return {("other", "check of " + ast.unparse(given))} | {o for o in inner if o[0] in ("copy", "other")}
                return {("other", "check of " + ast.unparse(given))}
            if callee == "_dev":
                return {("copy", "_dev")}
            if isinstance(expr.func, ast.Attribute) and isinstance(expr.func.value, ast.Name) and expr.func.value.id == "torch" \
                    and callee in FRESH:
                return {("fresh",)}
            if isinstance(expr.func, ast.Attribute) and callee in VIEWS:
                return self.of(mod, expr.func.value, depth + 1, before)
            if isinstance(expr.func, ast.Attribute) and callee in COPIES:
                return {("copy", "." + callee)} | {o for o in self.of(mod, expr.func.value, depth + 1, before) if o[0] != "fresh"}
            helper = self.helper(mod, expr)
            if helper is not None:
                return self.returned(mod, expr, helper, None, depth + 1)
        return {("other", ast.unparse(expr))}

    def helper(self, mod, call):
        """The function of the same module a call goes to: f(...) or self.f(...)."""
        callee = _callee(call)
        if isinstance(call.func, ast.Name) and callee in mod.functions:
            return mod.functions[callee]
        if isinstance(call.func, ast.Attribute) and isinstance(call.func.value, ast.Name) and call.func.value.id == "self":
            cls = mod.owner(call)[0].split(".")[0]
            return mod.functions.get(cls + "." + callee)
        return None

    def returned(self, mod, call, helper, index, depth):
        """What a helper returns (element `index` of its tuple), its own parameters traced back to the caller's arguments."""
        out = set()
        for node in ast.walk(helper):
            if not isinstance(node, ast.Return) or node.value is None:
                continue
            value = node.value
            if index is not None:
                if not isinstance(value, ast.Tuple) or len(value.elts) <= index[0]:
                    out.add(("other", "return of " + helper.name))
                    continue
                value = value.elts[index[0]]
            for o in self.of(mod, value, depth + 1):
                if o[0] in ("param", "check"):
                    arg = self.argument(call, helper, o[1])
                    if arg is None:
                        out.add(("none",) if o[0] == "param" else ("other", f"{helper.name}: {o[1]} not passed"))
                    elif o[0] == "param":
                        out |= self.name(mod, arg, arg.id, depth + 1, before=call) if isinstance(arg, ast.Name) \
                            else self.of(mod, arg, depth + 1)
                    elif isinstance(arg, ast.Name):
                        inner = self.name(mod, arg, arg.id, depth + 1, before=call)
                        out |= {("check", arg.id)} if inner <= {("param", arg.id), ("none",)} and ("param", arg.id) in inner \
                            else {("other", "check of " + ast.unparse(arg))}
                    elif isinstance(arg, ast.Constant) and arg.value in (None, False):
                        out.add(("none",))
                    else:
                        out.add(("other", "check of " + ast.unparse(arg)))
                else:
                    out.add(o)
        return out or {("other", "no return in " + helper.name)}

    @staticmethod
    def argument(call, fdef, param):
        pos = _positional(fdef)
        if param in pos and pos.index(param) < len(call.args):
            return call.args[pos.index(param)]
        for kw in call.keywords:
            if kw.arg == param:
                return kw.value
        return None

    # ---- names
    def name(self, mod, at, name, depth, before=None):
        """Every binding of `name` visible at the node `at` (`before`: only those that stand before that node in the text --
        what a check is applied to is the name as it was)."""
        scopes = _scopes(at)
        limit = (before.lineno, before.col_offset) if before is not None else None
        around = set(_ancestors(before)) if before is not None else set()
        for k, scope in enumerate(scopes):
            params = _params(scope) if isinstance(scope, ast.FunctionDef) else [a.arg for a in scope.args.args]
            found = set()
            if isinstance(scope, ast.FunctionDef):
                for node in ast.walk(scope):
                    if limit is not None and hasattr(node, "lineno") and ((node.lineno, node.col_offset) >= limit or node in around
                                                                           or _exclusive(node, before)):
                        continue
                    if isinstance(node, ast.Assign):
                        for target in node.targets:
                            for t, index in _targets(target):
                                if isinstance(t, ast.Name) and t.id == name and _scopes(node)[0] is scope:
                                    found |= self.assigned(mod, node.value, index, depth, node)
                    elif isinstance(node, (ast.AugAssign, ast.AnnAssign)) and isinstance(node.target, ast.Name) \
                            and node.target.id == name and _scopes(node)[0] is scope:
                        found.add(("other", ast.unparse(node)))
                    elif isinstance(node, (ast.For, ast.comprehension)) and _scopes(node)[0] is scope:
                        if any(isinstance(t, ast.Name) and t.id == name for t, _ in _targets(node.target)):
                            found |= self.of(mod, node.iter, depth, node)
            if name in params:
                if k == len(scopes) - 1:
                    if not _rebound(scope, name, limit):
                        found.add(("param", name))
                else:
                    found |= self.callback(mod, scope, params.index(name), depth)
            if found:
                return found
        return {("other", "unbound " + name)}

    def assigned(self, mod, value, index, depth, before=None):
        if not index:
            return self.of(mod, value, depth, before)
        if isinstance(value, (ast.Tuple, ast.List)) and len(value.elts) > index[0]:
            return self.assigned(mod, value.elts[index[0]], index[1:], depth, before)
        if isinstance(value, ast.Call):
            helper = self.helper(mod, value)
            if helper is not None and len(index) == 1:
                return self.returned(mod, value, helper, index, depth)
        return {("other", "element of " + ast.unparse(value))}

    def callback(self, mod, scope, position, depth):
        """A parameter of a lambda or nested function: the argument its one user calls it with.  The callable is handed, by
        itself or by its name, to a function of the same module, which calls the parameter that receives it."""
        if isinstance(scope, ast.FunctionDef):
            outer = _scopes(scope.parent)[0]
            uses = [n for n in ast.walk(outer) if isinstance(n, ast.Name) and n.id == scope.name and isinstance(n.ctx, ast.Load)]
        else:
            uses = [scope]
        out = set()
        for use in uses:
            call = use.parent
            helper = self.helper(mod, call) if isinstance(call, ast.Call) else None
            if helper is None or use not in call.args:
                return {("other", "callback handed to " + ast.unparse(call)[:60])}
            receiver = _positional(helper)[call.args.index(use)]
            inner = [n for n in ast.walk(helper) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == receiver]
            if not inner:
                return {("other", f"{helper.name} never calls {receiver}")}
            for n in inner:
                out |= self.of(mod, n.args[position], depth + 1) if position < len(n.args) else {("other", "too few arguments")}
        return out or {("other", "callback never used")}

    def attribute(self, mod, expr, depth):
        """self.<attr>: every assignment to it in the class, or the property of that name."""
        cls = mod.owner(expr)[0].split(".")[0]
        out = set()
        for q, f in mod.functions.items():
            if not q.startswith(cls + "."):
                continue
            for node in ast.walk(f):
                if isinstance(node, ast.Assign):
                    for target in node.targets:
                        for t, index in _targets(target):
                            if isinstance(t, ast.Attribute) and t.attr == expr.attr and isinstance(t.value, ast.Name) and t.value.id == "self":
                                out |= self.assigned(mod, node.value, index, depth)
        return out or {("other", "self." + expr.attr + " is assigned nowhere in " + cls)}


def sites(modules, positions):
    """[(module, face, entry point, call node)] of every call of an entry point of `positions` in the package: `.entry(...)`, or
    a call through a local name listed in ALIASED."""
    out = []
    for mod in modules.values():
        for node in ast.walk(mod.tree):
            if not isinstance(node, ast.Call):
                continue
            callee = _callee(node)
            if isinstance(node.func, ast.Attribute) and callee in positions:
                out.append((mod, mod.name + "." + mod.owner(node)[0], callee, node))
            elif isinstance(node.func, ast.Name) and any(isinstance(x, ast.FunctionDef) for x in _scopes(node)):
                face = mod.name + "." + mod.owner(node)[0]
                for entry in ALIASED.get((face, callee), ()):
                    out.append((mod, face, entry, node))
    return out


def violations(modules, positions, binding):
    """What the call sites say against the table -> (sites seen, [text]).  At every written position of every call site the
    expression is `_ptr(e)` / `ops._ptr(e)` or None; `e` traces back to what the row of that face says and to nothing that may
    copy."""
    origins, bad, seen, used = Origins(modules), [], 0, set()
    for mod, face, entry, call in sites(modules, positions):
        seen += 1
        for pos, param in positions[entry].items():
            rows = binding.get((entry, param), [])
            where = f"{face}: {entry}({param})"
            if any(r in (HOST, COMM) for r in rows):
                continue
            if pos >= len(call.args):
                bad.append(f"{where}: the call has no argument {pos}")
                continue
            got = set()
            for arg in ([call.args[pos].body, call.args[pos].orelse] if isinstance(call.args[pos], ast.IfExp) else [call.args[pos]]):
                if isinstance(arg, ast.Constant) and arg.value is None:
                    got.add(("none",))
                elif isinstance(arg, ast.Call) and _callee(arg) == "_ptr" and len(arg.args) == 1:
                    got |= origins.of(mod, arg.args[0], 0, call)
                else:
                    got.add(("other", "not _ptr(...): " + ast.unparse(arg)))
            mine = [r for r in rows if isinstance(r, tuple) and ((r[1] == face and r[3] is None) or r[3] == "@" + face)]
            allowed = {("fresh",), ("none",)}
            for kind, row_face, name, _ in mine:
                used.add((entry, param, kind, row_face, name))
                if kind == "ARG":
                    if ("check", name) not in got:
                        bad.append(f"{where}: `{name}` does not reach the library through the shared check: {sorted(got)}")
                    allowed |= {("check", name), ("param", name)}          # (the parameter as it came: None, where None is allowed)
                else:
                    allowed |= {("param", name)}
            if not mine and INTERNAL not in rows:
                bad.append(f"{where}: no row of BINDING covers this call site")
            for o in sorted(got - allowed):
                bad.append(f"{where}: {o[0]}: {o[1] if len(o) > 1 else ''}")
    return seen, bad, used


# ------------------------------------------------------------------------------------------------------------------ the table
BINDING = {
    ("vbq_solve_grid", "h_grid"): [HOST],
    ("vbq_device_name", "buf"): [HOST],
    ("vbq_check_inputs_f32", "d_bad"): [INTERNAL],
    ("vbq_quantize_f32", "d_out_idx"): [ARG("ops.quantize", "out_idx")],
    ("vbq_quantize_f32", "d_out_zhat"): [ARG("ops.quantize", "out_zhat")],
    ("vbq_quantize_f32", "d_out_bits"): [ARG("ops.quantize", "out_bits")],
    ("vbq_quantize_f32", "d_workspace"): [ARG("ops.quantize", "workspace")],
    ("vbq_n_bit_intervals_f32", "d_left"): [INTERNAL],
    ("vbq_n_bit_intervals_f32", "d_right"): [INTERNAL],
    ("vbq_quantize_rows_f32", "d_out_idx"): [ARG("ops.quantize", "out_idx")],
    ("vbq_quantize_rows_f32", "d_out_zhat"): [ARG("ops.quantize", "out_zhat")],
    ("vbq_quantize_rows_f32", "d_out_bits"): [ARG("ops.quantize", "out_bits")],
    ("vbq_quantize_rows_f32", "d_workspace"): [ARG("ops.quantize", "workspace")],
    ("vbq_level_counts_f32", "d_level_counts"): [ARG("ops.level_counts", "out")],
    ("vbq_level_counts_f32", "d_workspace"): [ARG("ops.level_counts", "workspace")],
    ("vbq_code_lengths_from_counts", "d_out_len"): [ARG("ops.code_lengths_from_counts", "out_len")],
    ("vbq_code_lengths_from_counts", "d_out_model"): [ARG("ops.code_lengths_from_counts", "out_model")],
    ("vbq_host_neg_log2_freq_f32", "log2_data"): [HOST],
    ("vbq_host_neg_log2_freq_f32", "h_out_model"): [HOST],
    ("vbq_host_neg_log2_freq_f32", "h_out_len"): [HOST],
    ("vbq_host_stage_run", "stage"): [HOST],
    ("vbq_argmax_candidates_f32", "d_out_j"): [INTERNAL],
    ("vbq_argmax_candidates_f32", "d_out_zhat"): [INTERNAL],
    ("vbq_argmax_candidates_f32", "d_out_bits"): [INTERNAL],
    ("vbq_xi_intervals_f64", "d_left"): [INTERNAL],
    ("vbq_xi_intervals_f64", "d_right"): [INTERNAL],
    ("vbq_xi_select_f64", "d_z_hat"): [INTERNAL],
    ("vbq_xi_select_f64", "d_num_bits"): [INTERNAL],
    ("vbq_xi_select_f64", "d_xi_hat"): [INTERNAL],
    ("vbq_xi_select_f64", "d_f_z_hat"): [INTERNAL],
    ("vbq_quantize_notebook_f64", "d_out_idx"): [ARG("ops.quantize_notebook", "out_idx")],
    ("vbq_quantize_notebook_f64", "d_out_val"): [INTERNAL],
    ("vbq_histogram_u16", "d_counts"): [ARG("ops.histogram", "out")],
    ("vbq_histogram_u16_i32", "d_counts"): [ARG("ops.histogram", "out")],
    ("vbq_histogram_rows_u16", "d_counts"): [ARG("ops.histogram", "out")],
    ("vbq_histogram_models_u16", "d_counts"): [ARG("ops.histogram_models", "counts")],
    ("vbq_histogram_models_u16", "d_models"): [ARG("ops.histogram_models", "models")],
    ("vbq_index_max_u16", "d_max"): [INTERNAL],
    ("vbq_moments_f32", "d_out"): [ARG("ops.moments", "out")],
    ("vbq_numpy_sum_sq_f32", "d_out"): [INTERNAL],
    ("vbq_numpy_sum_sq_f32", "d_workspace"): [INTERNAL],
    ("vbq_numpy_row_sums_f32", "d_out"): [INTERNAL],
    ("vbq_numpy_row_sums_f32", "d_workspace"): [ARG("ops.numpy_row_sums", "workspace")],
    ("vbq_gather_f32", "d_out"): [INTERNAL],
    ("vbq_rd_sums_u16", "d_out"): [ARG("ops.rd_sums", "out")],
    ("vbq_transpose_f32", "d_out"): [ARG("ops.transpose", "out")],
    ("vbq_transpose_planes", "d_out"): [ARG("ops.transpose_planes", "out")],
    ("vbq_prep_planes_f32", "d_mu_cb"): [ARG("ops.prep_planes", "out_mu")],
    ("vbq_prep_planes_f32", "d_sigma_cb"): [ARG("ops.prep_planes", "out_sigma")],
    ("vbq_gather_latents_u16", "d_out_zhat"): [INTERNAL],
    ("vbq_gather_latents_u16", "d_out_raw_bits"): [INTERNAL],
    ("vbq_gather_latents_u16", "d_out_num_bits"): [INTERNAL],
    ("vbq_gather_latents_u16", "d_out_idx"): [INTERNAL],
    ("vbq_compress_latents_f32", "d_out_zhat"): [INTERNAL],
    ("vbq_compress_latents_f32", "d_out_raw_bits"): [INTERNAL],
    ("vbq_compress_latents_f32", "d_out_num_bits"): [INTERNAL],
    ("vbq_compress_latents_f32", "d_workspace"): [ARG("ops.compress_latents", "workspace")],
    ("vbq_build_entropy_models_f32", "d_level_counts"): [INTERNAL],
    ("vbq_build_entropy_models_f32", "d_level_len"): [INTERNAL],
    ("vbq_build_entropy_models_f32", "d_raw_models"): [INTERNAL],
    ("vbq_build_entropy_models_f32", "d_counts"): [INTERNAL],
    ("vbq_build_entropy_models_f32", "d_models"): [INTERNAL],
    ("vbq_build_entropy_models_f32", "d_workspace"): [INTERNAL],
    ("vbq_bmshj_cdf_pdf_f32", "d_cdf"): [INTERNAL],
    ("vbq_bmshj_cdf_pdf_f32", "d_pdf"): [INTERNAL],
    ("vbq_bmshj_cdf_pdf_f32", "d_logpdf"): [INTERNAL],
    ("vbq_bmshj_icdf_step_f32", "d_left"): [ARG("ops.bmshj_icdf_step", "left")],
    ("vbq_bmshj_icdf_step_f32", "d_right"): [ARG("ops.bmshj_icdf_step", "right")],
    ("vbq_bmshj_icdf_step_f32", "d_mid"): [ARG("ops.bmshj_icdf_step", "mid")],
    ("vbq_bmshj_icdf_step_f32", "d_flags"): [ARG("ops.bmshj_icdf_step", "flags")],
    ("vbq_bmshj_icdf_chain_f32", "d_left"): [ARG("ops.bmshj_icdf_chain", "left")],
    ("vbq_bmshj_icdf_chain_f32", "d_right"): [ARG("ops.bmshj_icdf_chain", "right")],
    ("vbq_bmshj_icdf_chain_f32", "d_mid"): [ARG("ops.bmshj_icdf_chain", "mid")],
    ("vbq_bmshj_icdf_chain_f32", "d_flags"): [ARG("ops.bmshj_icdf_chain", "flags")],
    ("vbq_bmshj_nll_grad_f32", "d_out"): [ARG("ops.bmshj_nll_grad", "out")],
    ("vbq_rans_encode_u16", "d_words"): [HANDED("coder.RansCodec._encode", "words")],
    ("vbq_rans_encode_u16", "d_sizes"): [HANDED("coder.RansCodec._encode", "sizes")],
    ("vbq_rans_sizes_u16", "d_sizes"): [HANDED("coder.RansCodec._sizes", "sizes")],
    ("vbq_rans_decode_u16", "d_idx"): [HANDED("coder.RansCodec._decode", "idx")],
    ("vbq_rans_decode_u16", "d_status"): [HANDED("coder.RansCodec._decode", "status")],
    ("vbq_rans_pack_u16", "d_payload"): [HANDED("coder.RansCodec._pack", "payload"), INTERNAL],
    ("vbq_rans_pack_u16", "d_offsets"): [HANDED("coder.RansCodec._pack", "offsets"), INTERNAL],
    ("vbq_rans_pack_u16", "d_total"): [HANDED("coder.RansCodec._pack", "total"),
        HANDED("quantizer.ChannelwisePriorCDFQuantizer._encode_batch_run", "d_host"),
        HANDED("quantizer.ChannelwisePriorCDFQuantizer._mapped_batch_run", "d_host")],
    ("vbq_rans_unpack_u16", "d_words"): [INTERNAL],
    ("vbq_rans_unpack_u16", "d_sizes"): [INTERNAL],
    ("vbq_rans_unpack_u16", "d_offsets"): [INTERNAL],
    ("vbq_rans_unpack_u16", "d_status"): [ARG("coder.RansCodec.unpack_device", "status")],
    ("vbq_rans_segment_offsets_u16", "d_offsets"): [INTERNAL],
    ("vbq_rans_segment_offsets_u16", "d_status"): [INTERNAL],
    ("vbq_rans_decode_values_f32", "d_out"): [HANDED("embeddings.CompressedEmbeddings._decode", "out")],
    ("vbq_rans_decode_values_f32", "d_status"): [INTERNAL],
    ("vbq_rans_il_sizes_u16", "d_sizes"): [INTERNAL],
    ("vbq_rans_il_encode_u16", "d_payload"): [INTERNAL],
    ("vbq_rans_il_decode_u16", "d_idx"): [HANDED("coder.RansCodec._decode_interleaved", "idx")],
    ("vbq_rans_il_decode_u16", "d_status"): [HANDED("coder.RansCodec._decode_interleaved", "status")],
    ("vbq_rans_map_encode_u16", "d_words"): [HANDED("coder.MappedRansCodec._encode", "words")],
    ("vbq_rans_map_encode_u16", "d_sizes"): [HANDED("coder.MappedRansCodec._encode", "sizes")],
    ("vbq_rans_map_sizes_u16", "d_sizes"): [HANDED("coder.MappedRansCodec._sizes", "sizes")],
    ("vbq_rans_map_decode_u16", "d_idx"): [HANDED("coder.MappedRansCodec._decode", "idx")],
    ("vbq_rans_map_decode_u16", "d_status"): [HANDED("coder.MappedRansCodec._decode", "status")],
    ("vbq_pack_counts_3x21", "d_words"): [INTERNAL],
    ("vbq_pack_counts_3x21", "d_overflow"): [INTERNAL],
    ("vbq_unpack_counts_3x21", "d_counts"): [ARG("dist.CountsAllReduce.start", "counts", via="@dist.CountsAllReduce.wait")],
    ("vbq_comm_unique_id", "h_id"): [COMM],
    ("vbq_comm_init", "comm"): [COMM],
    ("vbq_allreduce_hist", "comm"): [COMM],
    ("vbq_allreduce_hist", "d_counts"): [COMM],
    ("vbq_comm_destroy", "comm"): [COMM],
    ("vbq_uniform_quantize_f32", "d_out_index"): [INTERNAL],
    ("vbq_uniform_quantize_f32", "d_out_value"): [INTERNAL],
    ("vbq_uniform_quantize_f32", "d_counts"): [INTERNAL],
    ("vbq_nearest_code_f64", "d_out_index"): [INTERNAL],
    ("vbq_nearest_code_f64", "d_out_value"): [INTERNAL],
    ("vbq_nearest_code_f64", "d_counts"): [INTERNAL],
    ("vbq_analogy_ranks_f32", "d_out_ranks"): [INTERNAL],
    ("vbq_analogy_ranks_f32", "d_workspace"): [INTERNAL],
    ("vbq_image_sqerr_u8", "d_out_sum"): [INTERNAL],
    ("vbq_u8_to_f64", "d_out"): [INTERNAL],
    ("vbq_unit_to_u8_f32", "d_out"): [INTERNAL],
    ("vbq_ssim_scale_f64", "d_out_ssim"): [INTERNAL],
    ("vbq_ssim_scale_f64", "d_out_cs"): [INTERNAL],
    ("vbq_ssim_scale_f64", "d_workspace"): [INTERNAL],
    ("vbq_downsample2_f64", "d_out"): [INTERNAL],
    ("vbq_budget_dp_f64", "d_out_bits"): [INTERNAL],
    ("vbq_budget_dp_f64", "d_out_obj"): [INTERNAL],
    ("vbq_budget_dp_f64", "d_status"): [ARG("ops.budget_dp", "status")],
    ("vbq_budget_dp_f64", "d_workspace"): [ARG("ops.budget_dp", "workspace")],
    ("vbq_budget_patience_f64", "d_out_bits"): [INTERNAL],
    ("vbq_budget_patience_f64", "d_out_g"): [INTERNAL],
    ("vbq_records_pack_u16", "d_words"): [ARG("ops.records_pack", "out")],
    ("vbq_records_pack_u16", "d_status"): [ARG("ops.records_pack", "status")],
    ("vbq_records_unpack_f32", "d_out_values"): [INTERNAL],
    ("vbq_records_unpack_f32", "d_out_idx"): [INTERNAL],
    ("vbq_records_unpack_f32", "d_status"): [ARG("ops.records_unpack", "status")],
    ("vbq_records_topk_f32", "d_out_ids"): [INTERNAL],
    ("vbq_records_topk_f32", "d_out_scores"): [INTERNAL],
    ("vbq_records_topk_f32", "d_status"): [ARG("ops.records_topk", "status")],
    ("vbq_records_topk_f32", "d_workspace"): [ARG("ops.records_topk", "workspace")],
    ("vbq_topk_f32", "d_out_ids"): [INTERNAL],
    ("vbq_topk_f32", "d_out_scores"): [INTERNAL],
    ("vbq_topk_f32", "d_workspace"): [ARG("ops.topk", "workspace")],
    ("vbq_records_bag_f32", "d_out"): [ARG("ops.records_bag", "out")],
    ("vbq_records_bag_f32", "d_status"): [ARG("ops.records_bag", "status")],
    ("vbq_bag_f32", "d_out"): [ARG("ops.bag", "out")],
    ("vbq_bag_f32", "d_status"): [ARG("ops.bag", "status")],
    ("vbq_rans_decode_window_f32", "d_out"): [ARG("ops.rans_decode_window", "out"),
        ARG("store.LatentStore.crops", "out", via="ops.rans_decode_window:out")],
    ("vbq_rans_decode_window_f32", "d_status"): [ARG("ops.rans_decode_window", "status"),
        ARG("store.LatentStore.crops", "status", via="ops.rans_decode_window:status")],
    ("vbq_rans_map_decode_window_f32", "d_out"): [ARG("ops.rans_map_decode_window", "out"),
        ARG("store.LatentStore.crops", "out", via="ops.rans_map_decode_window:out")],
    ("vbq_rans_map_decode_window_f32", "d_status"): [ARG("ops.rans_map_decode_window", "status"),
        ARG("store.LatentStore.crops", "status", via="ops.rans_map_decode_window:status")],
    ("vbq_rans_encode_files_u16", "d_words"): [ARG("ops.rans_encode_files", "words")],
    ("vbq_rans_encode_files_u16", "d_sizes"): [ARG("ops.rans_encode_files", "sizes")],
    ("vbq_rans_encode_files_u16", "d_status"): [ARG("ops.rans_encode_files", "status")],
    ("vbq_rans_sizes_files_u16", "d_totals"): [ARG("ops.rans_sizes_files", "totals")],
    ("vbq_rans_sizes_files_u16", "d_status"): [ARG("ops.rans_sizes_files", "status")],
    ("vbq_rans_map_encode_files_u16", "d_words"): [ARG("ops.rans_map_encode_files", "words")],
    ("vbq_rans_map_encode_files_u16", "d_sizes"): [ARG("ops.rans_map_encode_files", "sizes")],
    ("vbq_rans_map_encode_files_u16", "d_status"): [ARG("ops.rans_map_encode_files", "status")],
    ("vbq_rans_map_sizes_files_u16", "d_sizes"): [ARG("ops.rans_map_sizes_files", "sizes")],
    ("vbq_rans_map_sizes_files_u16", "d_status"): [ARG("ops.rans_map_sizes_files", "status")],
    ("vbq_rans_map_rates_files_u16", "d_totals"): [ARG("ops.rans_map_rates_files", "totals")],
    ("vbq_rans_map_rates_files_u16", "d_status"): [ARG("ops.rans_map_rates_files", "status")],
    ("vbq_rans_il_sizes_files_u16", "d_sizes"): [ARG("ops.rans_il_sizes_files", "sizes")],
    ("vbq_rans_il_sizes_files_u16", "d_status"): [ARG("ops.rans_il_sizes_files", "status")],
    ("vbq_rans_il_encode_files_u16", "d_payload"): [ARG("ops.rans_il_encode_files", "payload")],
    ("vbq_rans_il_encode_files_u16", "d_status"): [ARG("ops.rans_il_encode_files", "status")],
    ("vbq_rans_il_decode_files_u16", "d_idx"): [ARG("ops.rans_il_decode_files", "idx")],
    ("vbq_rans_il_decode_files_u16", "d_status"): [ARG("ops.rans_il_decode_files", "status")],
    ("vbq_rans_il_rates_files_u16", "d_sizes"): [ARG("ops.rans_il_rates_files", "sizes")],
    ("vbq_rans_il_rates_files_u16", "d_status"): [ARG("ops.rans_il_rates_files", "status")],
    ("vbqx_records_scores_f32", "d_out"): [ARG("ops.records_scores", "out")],
    ("vbqx_records_scores_f32", "d_status"): [ARG("ops.records_scores", "status")],
    ("vbqx_scores_f32", "d_out"): [ARG("ops.scores", "out")],
    ("vbqx_scores_f32", "d_status"): [ARG("ops.scores", "status")],
    ("vbqb_budget_sweep_f64", "d_out_bits"): [INTERNAL],
    ("vbqb_budget_sweep_f64", "d_out_obj"): [INTERNAL],
    ("vbqb_budget_sweep_f64", "d_curve"): [INTERNAL],
    ("vbqb_budget_sweep_f64", "d_status"): [ARG("ops.budget_dp_sweep", "status")],
    ("vbqb_budget_sweep_f64", "d_workspace"): [ARG("ops.budget_dp_sweep", "workspace")],
    ("vbqk_kmeans1d_f64", "d_out_starts"): [INTERNAL],
    ("vbqk_kmeans1d_f64", "d_out_codes"): [INTERNAL],
    ("vbqk_kmeans1d_f64", "d_out_counts"): [INTERNAL],
    ("vbqk_kmeans1d_f64", "d_out_sse"): [INTERNAL],
    ("vbqk_kmeans1d_f64", "d_status"): [ARG("kmeans1d.kmeans1d_dp", "status")],
    ("vbqk_kmeans1d_f64", "d_workspace"): [ARG("kmeans1d.kmeans1d_dp", "workspace")],
    ("vbqk_nearest_code_channels_f64", "d_out_index"): [INTERNAL],
    ("vbqk_nearest_code_channels_f64", "d_out_value"): [INTERNAL],
    ("vbqk_nearest_code_channels_f64", "d_counts"): [ARG("kmeans1d.nearest_code_channels", "counts")],
    ("vbqs_plan_boxes", "d_desc"): [ARG("store.plan_boxes", "desc")],
    ("vbqs_plan_boxes", "d_segs"): [ARG("store.plan_boxes", "segs")],
    ("vbqs_plan_boxes", "d_status"): [ARG("store.plan_boxes", "status"),
        ARG("store.LatentStore.crops", "status", via="store.plan_boxes:status")],
}
"""(entry point, parameter) -> its rows."""

_OR = ("or", "OR-ed into")
_ADD = ("add", "ADDED to")
_KEEP = ("keep", "left untouched")
IN_PLACE = {
    # the bisection state: brackets that are read and narrowed where they lie, flags that a step accumulates into
    **{("vbq_bmshj_icdf_step_f32", p): ("state", "one masked bisection update") for p in ("d_left", "d_right", "d_mid")},
    ("vbq_bmshj_icdf_step_f32", "d_flags"): ("state", "writes mid points and accumulates"),
    **{("vbq_bmshj_icdf_chain_f32", p): ("state", "n_steps of those updates enqueued at once") for p in ("d_left", "d_right", "d_mid")},
    ("vbq_bmshj_icdf_chain_f32", "d_flags"): ("state", "continues the chain from flags[n_steps]"),
    # sums, counts and totals
    ("vbq_level_counts_f32", "d_level_counts"): _ADD,
    ("vbq_histogram_u16", "d_counts"): ("add", "Counts are ADDED to d_counts"),
    ("vbq_histogram_u16_i32", "d_counts"): ("add", "Counts are ADDED to d_counts"),
    ("vbq_histogram_rows_u16", "d_counts"): ("add", "Counts are ADDED to d_counts"),
    ("vbq_moments_f32", "d_out"): ("add", "(ADDED to d_out)"),
    ("vbq_rd_sums_u16", "d_out"): ("add", "d_out[2l]     +="),
    ("vbq_bmshj_nll_grad_f32", "d_out"): ("add", "ADDS to d_out[c][0..42]"),
    ("vbq_rans_sizes_files_u16", "d_totals"): _ADD,
    ("vbq_rans_map_rates_files_u16", "d_totals"): _ADD,
    ("vbqk_nearest_code_channels_f64", "d_counts"): ("add", "is ADDED to d_counts[c][j]"),
    # slots that keep what they held
    **{(e, p): _KEEP for e in ("vbq_rans_encode_files_u16", "vbq_rans_map_encode_files_u16") for p in ("d_words", "d_sizes")},
    ("vbq_rans_map_sizes_files_u16", "d_sizes"): _KEEP,
    ("vbq_rans_il_sizes_files_u16", "d_sizes"): _KEEP,
    ("vbq_rans_il_rates_files_u16", "d_sizes"): _KEEP,
    ("vbq_rans_il_encode_files_u16", "d_payload"): _KEEP,
    ("vbq_rans_il_decode_files_u16", "d_idx"): _KEEP,
    ("vbq_rans_decode_window_f32", "d_out"): _KEEP,
    ("vbq_rans_map_decode_window_f32", "d_out"): _KEEP,
    # status words
    **{(e, "d_status"): _OR for e in (
        "vbq_budget_dp_f64", "vbqb_budget_sweep_f64", "vbqk_kmeans1d_f64", "vbq_records_pack_u16", "vbq_records_unpack_f32",
        "vbq_records_topk_f32", "vbq_records_bag_f32", "vbq_bag_f32", "vbqx_records_scores_f32", "vbqx_scores_f32",
        "vbq_rans_unpack_u16", "vbq_rans_decode_window_f32", "vbq_rans_map_decode_window_f32", "vbq_rans_encode_files_u16",
        "vbq_rans_sizes_files_u16", "vbq_rans_map_encode_files_u16", "vbq_rans_map_sizes_files_u16",
        "vbq_rans_map_rates_files_u16", "vbq_rans_il_sizes_files_u16", "vbq_rans_il_rates_files_u16",
        "vbq_rans_il_encode_files_u16", "vbq_rans_il_decode_files_u16", "vbqs_plan_boxes")},
}
"""(entry point, parameter) of an ARG row -> (what the call does with the earlier content: "state" it updates, "add", "or",
"keep" for the slots it does not name; words of the declaring header that say so).  Everything else is assigned."""


def arg_rows():
    """[(entry point, parameter, face, python parameter, via)] of every ARG row, in the table's order."""
    return [(e, p, r[1], r[2], r[3]) for (e, p), rows in BINDING.items() for r in rows if isinstance(r, tuple) and r[0] == "ARG"]


def handed_violations(modules, binding):
    """Every HANDED row names a private helper, and every call of that helper in its module hands it, at that parameter, a new
    tensor (or None) -> (calls seen, [text])."""
    origins, bad, seen = Origins(modules), [], 0
    rows = sorted({(r[1], r[2]) for rs in binding.values() for r in rs if isinstance(r, tuple) and r[0] == "HANDED"})
    for face, param in rows:
        mod_name, _, qual = face.partition(".")
        mod, helper = modules[mod_name], qual.split(".")[-1]
        fdef = mod.functions.get(qual)
        if fdef is None or not helper.startswith("_") or param not in _params(fdef):
            bad.append(f"{face}({param}): no such private helper or parameter")
            continue
        calls = [n for n in ast.walk(mod.tree) if isinstance(n, ast.Call) and _callee(n) == helper]
        if not calls:
            bad.append(f"{face}: never called in vbq_amd/{mod_name}")
        for call in calls:
            seen += 1
            arg = Origins.argument(call, fdef, param)
            got = {("none",)} if arg is None else origins.of(mod, arg, 0, call)
            for o in sorted(got - {("fresh",), ("none",)}):
                bad.append(f"{mod_name}.{mod.owner(call)[0]} hands {face}({param}) {ast.unparse(arg)}: {o[0]}: {o[1] if len(o) > 1 else ''}")
    return seen, bad


def via_violations(modules, binding):
    """Every ARG row with a `via`: the face checks its parameter with the shared check and hands it -- or a slice or view of it
    -- to the named function under the named keyword -> (rows seen, [text])."""
    origins, bad, seen = Origins(modules), [], 0
    for (entry, p), rows in binding.items():
        for r in rows:
            if not (isinstance(r, tuple) and r[0] == "ARG" and r[3]) or r[3].startswith("@"):
                continue
            seen += 1
            _, face, param, via = r
            target, keyword = via.split(":")
            mod_name, _, qual = face.partition(".")
            mod, fdef = modules[mod_name], modules[mod_name].functions.get(qual)
            inner = [x for x in binding[(entry, p)] if isinstance(x, tuple) and x[0] == "ARG" and x[1] == target and x[2] == keyword]
            if fdef is None or not inner:
                bad.append(f"{face}({param}) via {via}: no such function, or {target}({keyword}) is no ARG row of {entry}({p})")
                continue
            found = False
            for call in (n for n in ast.walk(fdef) if isinstance(n, ast.Call) and _callee(n) == target.split(".")[-1]):
                for kw in call.keywords:
                    if kw.arg == keyword:
                        found = True
                        got = origins.of(mod, kw.value, 0, call)
                        if ("check", param) not in got or got - {("check", param), ("param", param), ("fresh",)}:
                            bad.append(f"{face}: {target}({keyword}={ast.unparse(kw.value)}): {sorted(got)}")
            if not found:
                bad.append(f"{face} never calls {target}({keyword}=...)")
    return seen, bad
