"""Every call answers for its inputs' VALUES, in any form, and for their CONTENT at the time of the call (tests/input_forms.py
has the forms, the edit routes and the catalogue).

ANSWERS UNDER EVERY FORM.  For every catalogued call, every array parameter and every form that applies: the answer with that one
argument in the form (all others plain), and once with every argument in it, equals the answer under the plain form of
form.values(a) -- read into plain host values (stream_order.plain) and compared by dtype, shape and every bit
(quantizer_histories.same).  The plain answer must be a result, not an error; the kind of what comes back (NumPy, CPU tensor,
device tensor) is that of the plain form of the same family, never a matter of layout or dtype; and after the call every
argument still holds its bits, its layout, its dtype and its flags.  A failure names the call, the parameter, the form and the
first differing leaf (dirty_memory.first_difference).  Where a call documents a narrower contract, input_forms.REFUSED has the
(call, parameter, form) with the exception and the sentence, and that refusal is what is asserted.

  a. every probe of quantizer_histories.PROBES on ONE quantizer in state A, through Inputs.in_form: the latents (host forms; device
     forms for the file probes), the class maps of the mapped probes, the image of the WITH_VAE probes;
  b. every case of test_gpu_stream_order.CASES as call(make(7)) against call([form(t) for t in make(7)]), under the three device
     layout forms (the ops level takes the exact dtype);
  c. input_forms.ENTRIES: the public calls outside the quantizer.

ANSWERS FOLLOW CONTENT, NOT IDENTITY.  For every entry of a. and c. and every edit route that applies (input_forms.EDIT_ROUTES: an
assignment into a NumPy array, the array behind torch.from_numpy, t.data.copy_, a torch.from_dlpack alias, the library's own
ops.transpose(..., out=t)): call with values A, overwrite every array argument in place with values B, call again with the same
objects -- the second answer equals a fresh call on B and differs from the first.  This probes api._CHECKED, compress_replay's
fast path, lazy.common_stack and whatever else a call keeps between calls.

THE CONTROLS.  A fake call that reads a strided tensor's storage as if it were dense is reported under dev_strided; with
ops._dev made to skip .contiguous() the strided form of quantize_planes differs.  If a control does not fire the module tests
nothing, and says so.

WHAT THE MODULE FOUND when it was written (each fixed with it; EXPERIMENTS.md has the fix-by-fix record):
  * api._device_table served a STALE torch table: it keyed the rank-order copy by (id, data_ptr, _version), and the version
    counter does not move for an edit through .data, a DLPack alias, the NumPy array behind torch.from_numpy or a kernel's out=
    write.  quantize() and quantize_rows_to_budget() then answered for the old table.  It also raised on an inference tensor
    (no version counter).  Now a device table's rank-order copy is gathered on every call (one launch, no synchronisation) and
    a CPU tensor takes the NumPy content path.
  * every quantizer method that takes latents refused a reversed array (torch.from_numpy: negative strides) and warned about a
    read-only one, where vbq_amd.quantize accepted both: all conversions now go through ops.host_tensor.
  * embeddings._bag_args / _listed_ids cast ids to int64 before the range check: a uint64 id >= 2**63 became padding.
  * rows_budget.level_candidates handed the raw pointer of its table to the kernel unchecked: a strided, transposed, f64 or f16
    table was read as dense f32 (180 of 225 scores wrong).  It checks its three tensors as every ops call does now.
  * compress_replay raised on a CPU image tensor that requires grad; the frequency table of a rANS codec aliased the caller's
    array; the baseline fits refused a nested list as "float64" (k-means) or binned it with f64 edges (uniform); the code book
    of the embedding files could not be a device tensor.  Everything else -- every probe, every ops-level case -- answered the
    same under every form from the first run on.

MEASURED on an MI355X (325 tests): the module takes 9.7 s after set-up, 20 s in all -- 5886 calls, 4437 (parameter, form) pairs,
1662 in-place edits, 44 refusals asserted, 44 exemptions (the fixture prints these figures on every run);
tests/test_gpu_dirty_memory.py reports 5.5 .. 6.0 s for itself.  Both controls fire."""
import collections
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dirty_memory as DM  # noqa: E402
import input_forms as IF  # noqa: E402
import quantizer_histories as QH  # noqa: E402
import stream_order as SO  # noqa: E402
import test_gpu_stream_order as TSO  # noqa: E402

pytestmark = pytest.mark.gpu

A = QH.STATES["A"]
COUNTS = collections.Counter()
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    t0 = time.perf_counter()
    yield
    print(f"\n[test_gpu_input_forms] {time.perf_counter() - t0:.1f} s; {COUNTS['calls']} calls, {COUNTS['pairs']} (parameter, form) "
          f"pairs, {COUNTS['edits']} in-place edits, {COUNTS['refusals']} refusals asserted, {len(IF.EXEMPT)} exemptions")


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """A device error is not a wrong answer: after one, nothing more of this module is launched."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"device error, the rest of the module is not run: {e}", returncode=3)


# ====================================================================================================== the harness
_DEVICE_ERRORS = ("HIP error", "hipError", "illegal memory", "CUDA error", "device-side assert", "unspecified launch failure")


def answer(fn):
    """("ok", the plain answer, the kinds of its leaves) or ("raised", the error's type name, its message).  A device error ends
    the session: nothing more is launched after one."""
    COUNTS["calls"] += 1
    try:
        out = fn()
        got = ("ok", _signed(SO.plain(out)), IF.kinds(out))
        torch.cuda.synchronize()
        return got
    except Exception as e:                                                        # noqa: BLE001 -- every error is an outcome here
        if any(s in str(e) for s in _DEVICE_ERRORS):
            pytest.exit(f"device error, the rest of the module is not run: {type(e).__name__}: {e}", returncode=3)
        return ("raised", type(e).__name__, str(e).splitlines()[0][:300] if str(e) else "")


def _signed(v):
    """quantizer_histories._plain reads an unsigned TENSOR as the signed view of its bits and leaves an unsigned NumPy array as
    it is: here every unsigned array becomes that signed view, so that a result compares by its bits whichever kind it is."""
    if isinstance(v, tuple):
        return tuple(_signed(x) for x in v)
    if isinstance(v, np.ndarray) and v.dtype.kind == "u" and v.dtype.itemsize > 1:
        return v.view({2: np.int16, 4: np.int32, 8: np.int64}[v.dtype.itemsize])
    return v


def same(a, b):
    return a[0] == b[0] and QH.same(a[:2] if a[0] == "ok" else a, b[:2] if b[0] == "ok" else b)


def why(got, want):
    if got[0] != want[0] or got[0] == "raised":
        return f"{got[:3] if got[0] == 'raised' else 'a result'} against {want[:3] if want[0] == 'raised' else 'a result'}"
    return DM.first_difference(got[1], want[1])


def check_entry(name, base, params, call, ref, refused=None, only=None):
    """Every parameter x every form that applies (of the names in `only`, when given), and every form on all parameters together
    -> the lines of what failed."""
    refused = IF.REFUSED if refused is None else refused
    plain = IF.plain_of(base)
    lines, expected, kinds_of = [], {}, {}

    def run(args):
        return answer(lambda: call(**args))

    def plain_args(values):
        return {p: plain.make(values[p]) for p in params}

    want = run(plain_args(ref))
    assert want[0] == "ok", f"{name}: the plain call is no result but {want}"
    for target in tuple(params) + ("all",):
        group = params if target == "all" else (target,)
        forms = {f.name: f for p in group for f in IF.forms_for(base, ref[p]) if only is None or f.name in only}
        for form in forms.values():
            hit = [p for p in group if form.applies(ref[p])]
            key = next(((name, p, form.name) for p in hit if (name, p, form.name) in refused), None)
            COUNTS["pairs"] += 1
            args = plain_args(ref)
            for p in hit:
                args[p] = form.make(ref[p])
            before = {p: IF.snapshot(a) for p, a in args.items()}
            got = run(args)
            where = f"{name}, {target} as {form.name}"
            if key is not None:
                exc, fragment, _ = refused[key]
                COUNTS["refusals"] += 1
                if not (got[0] == "raised" and got[1] == exc.__name__ and fragment in got[2]):
                    lines.append(f"{where}: the documented refusal is {exc.__name__}({fragment!r}), got {got[:3] if got[0] == 'raised' else 'a result'}")
                continue
            values = {p: (form.values(ref[p]) if p in hit else ref[p]) for p in params}
            changed = tuple(p for p in hit if values[p] is not ref[p])
            if changed not in expected:
                expected[changed] = want if not changed else run(plain_args(values))
            if not same(got, expected[changed]):
                lines.append(f"{where}: {why(got, expected[changed])} (the form against the plain form of its values)")
                continue
            base_form = IF.BASELINE[form.family]
            if base_form is not plain:                                            # the kind of the result follows the family's plain form
                k = (target, form.family)
                if k not in kinds_of:
                    a2 = plain_args(ref)
                    for p in hit:
                        a2[p] = base_form.make(ref[p])
                    kinds_of[k] = run(a2)
                want_kinds = kinds_of[k][2] if kinds_of[k][0] == "ok" else None
            else:
                want_kinds = want[2]
            if got[2] != want_kinds:
                lines.append(f"{where}: returns {got[2]}, the {base_form.name} form returns {want_kinds}")
            after = {p: IF.snapshot(a) for p, a in args.items()}
            for p in params:
                if after[p] != before[p]:
                    what = [k for k, (x, y) in enumerate(zip(before[p], after[p])) if x != y]
                    lines.append(f"{where}: the call changed its argument {p} (fields {what} of input_forms.snapshot)")
    return lines


def check_edits(name, base, params, call, ref_a, ref_b):
    """Call on A, overwrite every argument in place with B by each route, call again with the same objects."""
    lines = []
    plain = IF.plain_of(base)
    fresh_b = answer(lambda: call(**{p: plain.make(ref_b[p]) for p in params}))
    for route in IF.routes_for(base):
        args = {p: route.form.make(ref_a[p]) for p in params}
        first = answer(lambda: call(**args))
        versions = {p: a._version for p, a in args.items() if hasattr(a, "_version")}
        for p in params:
            route.edit(args[p], ref_b[p])
            COUNTS["edits"] += 1
        torch.cuda.synchronize()
        if route.name in IF.SILENT_ROUTES:
            assert versions == {p: a._version for p, a in args.items() if hasattr(a, "_version")}, \
                f"{route.name} moved a version counter: it is no silent edit (any more)"
        second = answer(lambda: call(**args))
        where = f"{name}, edited through {route.name}"
        if first[0] != "ok":
            lines.append(f"{where}: the first call is no result but {first[:3]}")
        elif same(second, first):
            lines.append(f"{where}: the second call answers as the first -- for the OLD content")
        elif not same(second, fresh_b):
            lines.append(f"{where}: {why(second, fresh_b)} (the second call against a fresh call on the new content)")
    return lines


# ====================================================================================================== c. the catalogue
@pytest.mark.parametrize("name", list(IF.ENTRIES))
def test_entry_under_every_form(name):
    e = IF.ENTRIES[name]
    call, make = e.build()
    lines = check_entry(name, e.base, e.params, call, make("A"))
    assert not lines, f"{len(lines)} of the forms of {name}:\n" + "\n".join(lines)


@pytest.mark.parametrize("name", [n for n in IF.ENTRIES if n not in IF.NOT_EDITABLE])
def test_entry_follows_the_content_of_its_arguments(name):
    e = IF.ENTRIES[name]
    call, make = e.build()
    a, b = make("A"), make("B")
    assert all(a[p].shape == b[p].shape and a[p].dtype == b[p].dtype and not np.array_equal(a[p], b[p]) for p in e.params), name
    lines = check_edits(name, e.base, e.params, call, a, b)
    assert not lines, "\n".join(lines)


# ====================================================================================================== b. the ops-level cases
@pytest.mark.parametrize("name", list(TSO.CASES))
def test_case_under_the_device_layout_forms(name):
    fn, _ = TSO.CASES[name]
    call, make = fn()
    ref = [t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t for t in make(7)]
    params = tuple(f"b[{k}]" for k, t in enumerate(ref) if isinstance(t, np.ndarray))
    assert params, name
    by_name = {f"b[{k}]": t for k, t in enumerate(ref)}

    def run(**kw):
        return call([kw.get(f"b[{k}]", t) for k, t in enumerate(ref)])
    lines = check_entry(name, "device", params, run, by_name, refused={}, only=IF.DEVICE_LAYOUT_FORMS)
    assert not lines, f"{len(lines)} of the forms of {name}:\n" + "\n".join(lines)


# ====================================================================================================== a. the probes
def quantizer(role):
    """One quantizer in state A for the answers under the forms and the edits ("subject"), one for what they are held against."""
    if role not in _CACHE:
        _CACHE[role] = QH.fresh(A)
    return _CACHE[role]


def _groups(name):
    """The groups of arrays of Inputs a probe reads (see Inputs.in_form)."""
    if name in QH.WITH_VAE:
        return ["X"]                                        # (their latents are the VAE's own)
    groups = ["files"]
    if "mapped" in name or "palettes" in name or name in ("r_decompress_m", "r_mapped_window", "r_mapped_batch"):
        groups += ["cls2"] + (["cls3"] if name in ("latents_mapped", "to_bytes_mapped", "coded_nbytes_mapped", "b_mapped") else [])
    return groups + ["all"]


def _arrays(inp, which):
    host = lambda a: np.asarray(a.detach().cpu() if hasattr(a, "detach") else a)
    out = []
    if which in ("files", "all"):
        out += [host(a) for pair in inp.files for a in pair]
    for g in ("cls2", "cls3"):
        if which in (g, "all"):
            out += [host(a) for a in getattr(inp, g)]
    if which in ("X", "all"):
        out.append(QH.image(QH.IMAGE_SHAPES[0]))
    return out


def _live(inp, which):
    """The arguments themselves (for the snapshot before and after)."""
    out = []
    if which in ("files", "all"):
        out += [a for pair in inp.files for a in pair]
    for g in ("cls2", "cls3"):
        if which in (g, "all"):
            out += list(getattr(inp, g))
    return out


PROBE_RUNS = list(QH.PROBES) + [n + "[device]" for n in {**QH.ONE_FILE, **QH.BATCHES}]


@pytest.mark.parametrize("name", PROBE_RUNS)
def test_probe_under_every_form(name):
    inp, dinp = TSO.inputs_A()
    on_device = name.endswith("[device]")
    probe, base = QH.PROBES[name.replace("[device]", "")], (dinp if on_device else inp)
    q, oracle = quantizer("subject"), quantizer("oracle")
    want = answer(lambda: probe(oracle, base))
    assert want[0] == "ok", f"{name}: the plain call is no result but {want}"
    lines = []
    for which in (["files"] if on_device else _groups(name.replace("[device]", ""))):
        arrays = _arrays(base, which)
        names = sorted({f.name for a in arrays for f in IF.forms_for("device" if on_device else "numpy", a)})
        for form in (IF.FORMS[n] for n in names):
            if which == "X" and form.family == "device":
                continue
            COUNTS["pairs"] += 1
            i = base.in_form(form, which)
            before = [IF.snapshot(a) for a in _live(i, which)]
            got = answer(lambda: probe(q, i))
            if any(form.values(a) is not a for a in arrays if form.applies(a)):
                expected = answer(lambda: probe(oracle, base.in_form(form, which, values_only=True)))
            else:
                expected = want
            where = f"probe {name}, {which} as {form.name}"
            if not same(got, expected):
                lines.append(f"{where}: {why(got, expected)} (the form against the plain form of its values)")
            elif [IF.snapshot(a) for a in _live(i, which)] != before:
                lines.append(f"{where}: the call changed its arguments")
    assert not lines, f"{len(lines)} of the forms of {name}:\n" + "\n".join(lines)


FILES_B = QH.latents(QH.FILE_SHAPES, seed=8)


@pytest.mark.parametrize("name", [n for n in PROBE_RUNS if n not in QH.WITH_VAE])
def test_probe_follows_the_content_of_its_latents(name):
    """The latents of Inputs are overwritten in place (the class maps, budgets and palettes stay): the same quantizer, asked again
    with the same objects, answers as the oracle does on fresh inputs of the new content."""
    inp, dinp = TSO.inputs_A()
    on_device = name.endswith("[device]")
    probe, base = QH.PROBES[name.replace("[device]", "")], (dinp if on_device else inp)
    q, oracle = quantizer("subject"), quantizer("oracle")
    plain = IF.DEV_PLAIN if on_device else IF.NP_PLAIN
    fresh = TSO.with_files(base, [(plain.make(m), plain.make(lv)) for m, lv in FILES_B])
    fresh_b = answer(lambda: probe(oracle, fresh))
    lines = []
    for route in IF.routes_for("device" if on_device else "numpy"):
        if route.form.family == "cpu":
            continue                                        # (the probes take NumPy arrays or device tensors: Inputs.on_device)
        i = base.in_form(route.form, "files")
        first = answer(lambda: probe(q, i))
        for (m, lv), (mb, lvb) in zip(i.files, FILES_B):
            route.edit(m, mb)
            route.edit(lv, lvb)
            COUNTS["edits"] += 2
        torch.cuda.synchronize()
        second = answer(lambda: probe(q, i))
        where = f"probe {name}, latents edited through {route.name}"
        if first[0] != "ok":
            lines.append(f"{where}: the first call is no result but {first[:3]}")
        elif same(second, first):
            lines.append(f"{where}: the second call answers as the first -- for the OLD content")
        elif not same(second, fresh_b):
            lines.append(f"{where}: {why(second, fresh_b)} (the second call against the oracle on the new content)")
    assert not lines, "\n".join(lines)


@pytest.mark.parametrize("name", list(QH.WITH_VAE))
def test_image_probe_follows_the_content_of_its_image(name):
    """ONE image buffer, refilled in place between two runs of the probe (compress_replay keeps a capture per VAE and image shape
    and a fast path for the image it saw last): the second run answers for what the buffer holds then."""
    inp, _ = TSO.inputs_A()
    probe, q, oracle = QH.PROBES[name], quantizer("subject"), quantizer("oracle")
    X0 = QH.image(QH.IMAGE_SHAPES[0])
    new = (0.7 * X0).astype(np.float32)
    buf = X0.copy()
    held, fresh = inp._copy(), inp._copy()
    held.image_form = lambda a: buf                          # the same object for every image the probe asks with
    fresh.image_form = lambda a: new.copy()
    first = answer(lambda: probe(q, held))
    buf[...] = new
    COUNTS["edits"] += 1
    second, want = answer(lambda: probe(q, held)), answer(lambda: probe(oracle, fresh))
    assert first[0] == "ok", first[:3]
    assert not same(second, first), f"probe {name}: the second run answers as the first -- for the OLD image"
    assert same(second, want), f"probe {name}, the image refilled in place: {why(second, want)}"


# ====================================================================================================== the premise, on the device
@pytest.mark.parametrize("route", [r for r in IF.SILENT_ROUTES if r.startswith("device")])
def test_a_silent_edit_of_a_device_tensor_leaves_the_version_counter_where_it_was(route):
    r = IF.EDIT_ROUTES[route]
    a = np.random.default_rng(1).normal(0, 1, (6, 5)).astype(np.float32)
    t = r.form.make(a)
    before = t._version
    r.edit(t, a + 1)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), a + 1) and t._version == before
    t.add_(1)
    assert t._version == before + 1


def test_every_device_form_is_what_it_says():
    a = np.random.default_rng(1).normal(0, 1, (6, 5)).astype(np.float32)
    ids = np.random.default_rng(2).integers(0, 200, (6, 5)).astype(np.int64)
    for ref in (a, ids):
        for form in IF.forms_for("device", ref):
            t = form.make(ref)
            assert t.is_cuda and tuple(t.shape) == ref.shape, form.name
            assert np.array_equal(t.detach().cpu().numpy().astype(ref.dtype), form.values(ref)), form.name
            if form.name in ("dev_strided", "dev_transposed"):
                assert not t.is_contiguous(), form.name
            if form.name == "dev_offset":
                assert t.storage_offset() == 1 and t.data_ptr() % 16 == ref.itemsize % 16 and t.is_contiguous()
            if form.name == "dev_inference":
                assert t.is_inference()
            if form.name == "dev_requires_grad":
                assert t.requires_grad
            if form.name in ("dev_float64", "dev_float16"):
                assert str(t.dtype) == "torch." + form.name[4:]


# ====================================================================================================== the controls
def test_control_a_call_that_reads_a_strided_tensor_as_dense_is_reported():
    def fake(x):
        dense = tuple(int(np.prod(x.shape[k + 1:])) for k in range(x.dim()))
        return torch.as_strided(x, tuple(x.shape), dense) * 1               # what a kernel given x.data_ptr() alone would read

    ref = {"x": np.random.default_rng(1).normal(0, 1, (6, 5)).astype(np.float32)}
    lines = check_entry("fake", "device", ("x",), fake, ref, refused={})
    named = [l for l in lines if "x as dev_strided" in l or "x as dev_transposed" in l]
    assert len(named) == 2 and all("answer" in l for l in named) and not [l for l in lines if "dev_offset" in l or "dev_inference" in l], \
        f"THE CONTROL DID NOT FIRE: a call that reads a strided tensor as if it were dense was not reported ({lines}) -- this " \
        f"module is testing nothing"
    assert any(l.startswith("fake, all as dev_strided") for l in lines)


def test_control_b_without_contiguous_the_strided_form_of_quantize_planes_differs(monkeypatch):
    """ops._dev made to skip .contiguous(): the kernels get the pointer of a strided tensor and read it as dense -- inside the
    tensor's own, twice as large storage."""
    from vbq_amd import ops
    call, make = TSO.CASES["quantize_planes"][0]()
    ref = {f"b[{k}]": t.cpu().numpy() for k, t in enumerate(make(7))}

    def run(**kw):
        return call([kw[f"b[{k}]"] for k in range(len(ref))])

    def no_copy(t, dtype, name):
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype, name
        return t
    assert not check_entry("quantize_planes", "device", tuple(ref), run, ref, refused={}, only=("dev_strided",))
    monkeypatch.setattr(ops, "_dev", no_copy)
    lines = check_entry("quantize_planes", "device", tuple(ref), run, ref, refused={}, only=("dev_strided",))
    assert any("as dev_strided" in l and "answer" in l for l in lines), \
        f"THE CONTROL DID NOT FIRE: without .contiguous() in ops._dev the strided form of quantize_planes answered as the plain " \
        f"one ({lines}) -- this module is testing nothing"
