"""tests/input_forms.py on the host: the forms are what they say, the coverage tables account for every public callable, and the
conversions that need no device answer for their inputs' values.

1. every form holds values(a) bit for bit and has the property it is named after (a form must not quietly become the plain one
   after a torch or NumPy upgrade); torch.from_numpy still refuses a negative stride and still warns about a read-only array --
   the reasons vbq_amd.ops.host_tensor exists;
2. the silent edit routes -- through the NumPy array a tensor shares its memory with, through .data -- leave the tensor's
   _version where it was (the premise of the stale-table test), and reading _version on an inference tensor raises;
3. coverage: every public callable of input_forms.MODULES, of store.LatentStore and (through quantizer_histories.PROBED) of the
   quantizer is in COVERED or EXEMPT, with an entry that exists, parameters its signature has and a reason of the closed list;
4. embeddings._bag_args, _listed_ids, _pair_ids and _row_ids under every integer form against the plain form, and the unsigned
   ids that used to wrap: a uint64 id of 2**63 + 5 and a uint32 id >= V raise IndexError;
5. api._device_table on dev = "cpu": after every silent edit of a torch table the pair is that of the new content; an
   inference tensor is accepted;
6. the calls that are host-only arithmetic (EXEMPT with HOST_ONLY) under the NumPy layout forms.

WHAT FAILS ON THE PARENT COMMIT: with the parent's vbq_amd/api.py the cases of 5 fail (the torch table was keyed by
(id, data_ptr, _version): the second call returned the pair of the OLD content; the inference tensor raised "Inference tensors do
not track version counter"); with the parent's vbq_amd/embeddings.py the uint64 cases of 4 fail for _bag_args and _listed_ids
(2**63 + 5 became a negative id, which means padding); _row_ids raised already, naming the wrapped value."""
import inspect
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import input_forms as IF  # noqa: E402
import quantizer_histories as QH  # noqa: E402

HOST_FORMS = [f for f in IF.FORMS.values() if f.family != "device"]
SAMPLES = {"f32_2d": np.random.default_rng(1).normal(0, 1, (6, 5)).astype(np.float32),
           "i64_2d": np.random.default_rng(2).integers(0, 200, (6, 5)).astype(np.int64),
           "f32_1d": np.random.default_rng(3).normal(0, 1, 9).astype(np.float32)}


def _bytes(arg):
    """The values an argument holds, as a C-contiguous NumPy array."""
    if isinstance(arg, torch.Tensor):
        return arg.detach().cpu().numpy().copy()
    return np.array(arg)


# ====================================================================================================== 1. the forms
@pytest.mark.parametrize("sample", list(SAMPLES))
@pytest.mark.parametrize("form", HOST_FORMS, ids=lambda f: f.name)
def test_a_form_holds_its_values_and_is_what_it_says(form, sample):
    a = SAMPLES[sample]
    if not form.applies(a):
        return                                                   # (the applicability rules have a test of their own)
    arg, want = form.make(a), form.values(a)
    got = _bytes(arg)
    assert got.shape == a.shape
    if form.family == "python":
        assert isinstance(arg, list) and np.array_equal(np.asarray(got, a.dtype), want)
    else:
        assert np.array_equal(got.astype(a.dtype), want) and got.astype(a.dtype).tobytes() == np.ascontiguousarray(want).tobytes()
        assert got.dtype == a.dtype or form.name.split("_")[-1] in ("float64", "float16", "int32", "uint8")
    assert not np.shares_memory(got, a)
    name = form.name
    if name in ("np_every_second", "np_fortran"):
        assert not arg.flags.c_contiguous
    if name in ("cpu_strided",):
        assert not arg.is_contiguous()
    if name == "np_reversed":
        assert arg.strides[0] < 0
    if name == "np_offset":
        assert arg.ctypes.data % 16 == a.itemsize % 16 and arg.flags.c_contiguous
    if name == "np_readonly":
        assert arg.flags.writeable is False
    if name == "cpu_shared":
        assert np.shares_memory(arg.numpy(), arg.shared_array)
    if name == "cpu_requires_grad":
        assert arg.requires_grad
    if name == "cpu_inference":
        assert arg.is_inference()
    if name in ("np_float64", "cpu_float64"):
        assert got.dtype == np.float64
    if name == "np_float16":
        assert got.dtype == np.float16 and not np.array_equal(want, a)          # the rounding is real on these samples
    if name == "np_int32":
        assert got.dtype == np.int32
    if name == "np_uint8":
        assert got.dtype == np.uint8


def test_the_plain_forms_and_the_applicability_rules():
    a = SAMPLES["f32_2d"]
    assert IF.NP_PLAIN.make(a).flags.c_contiguous and IF.NP_PLAIN.make(a) is not a
    assert IF.CPU_PLAIN.make(a).is_contiguous() and not np.shares_memory(IF.CPU_PLAIN.make(a).numpy(), a)
    names = lambda base, arr: {f.name for f in IF.forms_for(base, arr)}
    assert "np_uint8" not in names("numpy", np.array([0, 300])) and "np_uint8" in names("numpy", np.array([0, 255]))
    assert "np_float16" not in names("numpy", SAMPLES["i64_2d"]) and "np_int32" not in names("numpy", a)
    assert "np_fortran" not in names("numpy", SAMPLES["f32_1d"]) and "np_every_second" in names("numpy", SAMPLES["f32_1d"])
    assert names("device", a) == {"dev_strided", "dev_transposed", "dev_offset", "dev_float64", "dev_float16", "dev_requires_grad",
                                  "dev_inference"}
    assert not names("numpy", a) & names("device", a) and "cpu_plain" not in names("numpy", a)
    assert set(IF.DEVICE_LAYOUT_FORMS) <= set(IF.FORMS)


def test_torch_from_numpy_refuses_and_warns_where_the_library_must_not():
    a = SAMPLES["f32_2d"]
    with pytest.raises(ValueError, match="negative"):
        torch.from_numpy(IF.FORMS["np_reversed"].make(a))
    from vbq_amd import ops
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for form in HOST_FORMS:
            if form.family == "numpy" and form.applies(a):
                t = ops.host_tensor(form.make(a))
                assert t.is_contiguous() and np.array_equal(t.numpy().astype(np.float32), form.values(a)), form.name
        assert np.array_equal(ops.host_tensor(a.tolist()).numpy(), a.astype(np.float64))
        plain = a.copy()
        assert np.shares_memory(ops.host_tensor(plain).numpy(), plain)            # the plain form is not copied
    # (torch warns about a read-only array once per process; whether it still does is only visible where nobody asked before)
    ro = IF.FORMS["np_readonly"].make(a)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.from_numpy(ro)
    assert all("writable" in str(w.message) for w in seen)


# ====================================================================================================== 2. the silent edits
@pytest.mark.parametrize("route", [r for r in IF.SILENT_ROUTES if not r.startswith("device")])
def test_a_silent_edit_leaves_the_version_counter_where_it_was(route):
    r = IF.EDIT_ROUTES[route]
    a, b = SAMPLES["f32_2d"], SAMPLES["f32_2d"] + 1
    t = r.form.make(a)
    before = t._version
    r.edit(t, b)
    assert np.array_equal(t.numpy(), b) and t._version == before
    t.add_(1)
    assert t._version == before + 1                                               # (an edit torch sees does move it)


def test_an_inference_tensor_has_no_version_counter():
    t = IF.FORMS["cpu_inference"].make(SAMPLES["f32_2d"])
    with pytest.raises(RuntimeError, match="version counter"):
        t._version


# ====================================================================================================== 3. coverage
def test_every_public_callable_is_covered_or_exempt():
    import test_gpu_stream_order as TSO
    public = IF.public_callables()
    assert len(public) > 100
    both = set(IF.COVERED) & set(IF.EXEMPT)
    assert not both, sorted(both)
    missing = sorted(set(public) - set(IF.COVERED) - set(IF.EXEMPT))
    assert not missing, "public callables in neither COVERED nor EXEMPT of tests/input_forms.py: " + ", ".join(missing)
    gone = sorted((set(IF.COVERED) | set(IF.EXEMPT)) - set(public))
    assert not gone, "names of COVERED / EXEMPT that are no public callables (any more): " + ", ".join(gone)
    for name, (where, params) in IF.COVERED.items():
        assert where in IF.ENTRIES or where in TSO.CASES, (name, where)
        have = inspect.signature(public[name]).parameters
        assert all(p in have for p in params), (name, params, list(have))
    reasons = IF.exempt_reasons()
    for name, reason in IF.EXEMPT.items():
        assert any(reason == r or (r.endswith("::") and reason.startswith(r)) for r in reasons), (name, reason)
        if reason == IF.TAKES_NO_ARRAY:
            hints = ("means", "stds", "mu", "sigma", "ids", "samples", "emb", "queries", "table", "freq", "idx", "words")
            assert not [p for p in inspect.signature(public[name]).parameters if p in hints], name
        if reason == IF.HOST_ONLY:
            assert name in HOST_ONLY_CALLS, name
    assert set(HOST_ONLY_CALLS) == {n for n, r in IF.EXEMPT.items() if r == IF.HOST_ONLY}


def test_every_entry_is_well_formed():
    for name, e in IF.ENTRIES.items():
        assert e.base in ("numpy", "device") and name.endswith(f"[{e.base}]") and e.params, name
    for (ent, param, form), (exc, fragment, (path, sentence)) in IF.REFUSED.items():
        assert ent in IF.ENTRIES and param in IF.ENTRIES[ent].params and form in IF.FORMS, (ent, param, form)
        assert issubclass(exc, Exception) and fragment
        import os
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        text = " ".join(" ".join(open(os.path.join(root, p.strip()), encoding="utf-8").read().split()) for p in path.split("/ ")
                        if os.path.exists(os.path.join(root, p.strip())))
        assert " ".join(sentence.split()) in text, f"REFUSED {ent}/{param}/{form}: {path} does not say {sentence!r}"


def test_the_quantizer_is_covered_through_its_probes():
    from vbq_amd import ChannelwisePriorCDFQuantizer
    public = QH.public_methods(ChannelwisePriorCDFQuantizer)
    assert sorted(set(QH.PROBED) | set(QH.EXEMPT)) == public
    assert all(p in QH.PROBES for ps in QH.PROBED.values() for p in ps)


def test_inputs_in_form_transforms_what_it_names():
    files, cls2, cls3 = QH.latents(QH.FILE_SHAPES), QH.class_maps(QH.FILE_SHAPES, 2), QH.class_maps(QH.FILE_SHAPES, 3)
    inp = QH.Inputs(sorted(QH.LAMBS_A), files, cls2, cls3, {"one": 5}, "t")
    rev, f16 = IF.FORMS["np_reversed"], IF.FORMS["np_float16"]
    new = inp.in_form(rev, "files")
    assert new.files[0][0].strides[0] < 0 and np.array_equal(new.files[0][0], files[0][0])
    assert new.cls2[0] is cls2[0] and new.budgets == inp.budgets and new.lambs == inp.lambs and inp.files[0][0] is files[0][0]
    assert inp.in_form(rev, "cls3").cls3[0].strides[0] < 0 and inp.in_form(rev, "cls3").files[0][0] is files[0][0]
    half = inp.in_form(f16, "all")
    assert half.files[1][1].dtype == np.float16 and half.cls2[1].dtype == np.int64            # float16 does not apply to a class map
    vals = inp.in_form(f16, "files", values_only=True)
    assert vals.files[1][1].dtype == np.float32 and np.array_equal(vals.files[1][1], f16.values(files[1][1]))
    X = QH.image(QH.IMAGE_SHAPES[0])
    assert inp.image(X) is X and not inp.in_form(IF.FORMS["np_every_second"], "X").image(X).flags.c_contiguous
    assert inp.in_form(f16, "X").image(X).dtype == np.float16
    assert inp.in_form(f16, "X", values_only=True).image(X).dtype == np.float32


# ====================================================================================================== 4. the id conversions
V = 301
INT_FORMS = [f for f in HOST_FORMS if f.applies(SAMPLES["i64_2d"])]


def _same(a, b):
    return QH.same(QH._plain(a), QH._plain(b))


def _id_calls():
    from vbq_amd import embeddings as E
    rng = np.random.default_rng(5)
    ids2, ids1 = rng.integers(0, 200, (3, 4)).astype(np.int64), rng.integers(0, 200, 8).astype(np.int64)
    offsets = np.array([0, 3, 3], np.int64)
    q = np.zeros((3, 7), np.float32)
    return {
        "_bag_args[2d]": (lambda ids: E._bag_args(ids, None, None, "sum", V), ids2),
        "_bag_args[ids]": (lambda ids: E._bag_args(ids, offsets, None, "mean", V), ids1),
        "_bag_args[offsets]": (lambda off: E._bag_args(ids1, off, None, "max", V), offsets),
        "_listed_ids": (lambda ids: E._listed_ids(q, ids, V), ids2),
        "_pair_ids[a]": (lambda a: E._pair_ids(a, ids2[::-1].copy(), V), ids2),
        "_pair_ids[b]": (lambda b: E._pair_ids(ids2, b, V), ids2),
        "_row_ids": (lambda ids: E._row_ids(ids, V), ids1),
    }


@pytest.mark.parametrize("call", ["_bag_args[2d]", "_bag_args[ids]", "_bag_args[offsets]", "_listed_ids", "_pair_ids[a]", "_pair_ids[b]",
                                  "_row_ids"])
def test_the_id_conversions_under_every_integer_form(call):
    fn, a = _id_calls()[call]
    want = fn(IF.NP_PLAIN.make(a))
    ran = 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for form in INT_FORMS:
            if form.applies(a):
                arg = form.make(a)
                before = IF.snapshot(arg)
                got = fn(arg)
                assert _same(got, want), f"{call} under {form.name}"
                assert IF.snapshot(arg) == before, f"{call} changed its argument under {form.name}"
                ran += 1
    assert ran >= 10


@pytest.mark.parametrize("call", ["_bag_args[2d]", "_bag_args[ids]", "_listed_ids", "_pair_ids[a]", "_row_ids"])
@pytest.mark.parametrize("dtype,bad", [(np.uint64, 2 ** 63 + 5), (np.uint32, V), (np.uint32, 2 ** 32 - 1), (np.uint64, 2 ** 64 - 1),
                                       (np.int64, V), (np.uint8, 255)])
def test_an_unsigned_id_outside_the_matrix_raises_and_never_wraps_into_padding(call, dtype, bad):
    fn, a = _id_calls()[call]
    v = 200 if dtype == np.uint8 else V                  # (a uint8 id cannot reach 301: a smaller matrix)
    from vbq_amd import embeddings as E
    if dtype == np.uint8:
        fn = {"_bag_args[2d]": lambda ids: E._bag_args(ids, None, None, "sum", v),
              "_bag_args[ids]": lambda ids: E._bag_args(ids, np.array([0, 3, 3]), None, "mean", v),
              "_listed_ids": lambda ids: E._listed_ids(np.zeros((3, 7), np.float32), ids, v),
              "_pair_ids[a]": lambda x: E._pair_ids(x, np.zeros((3, 4), np.int64), v),
              "_row_ids": lambda ids: E._row_ids(ids, v)}[call]
    ids = (a % 100).astype(dtype)
    fn(ids)                                              # in range: answered
    ids.reshape(-1)[3] = bad
    with pytest.raises(IndexError, match=rf"row {bad} outside \[0, {v}\)"):
        fn(ids)


# ====================================================================================================== 5. the facade's table
def _pair_of(tab, N=4):
    from vbq_amd import tables as TB
    return np.asarray(tab, np.float32), TB.level_major_to_sorted(np.asarray(tab, np.float32))


@pytest.mark.parametrize("route", ["cpu_shared_array", "cpu_data", "numpy_assign"])
@pytest.mark.parametrize("validate", [True, False])
def test_device_table_follows_the_content_of_a_host_table(route, validate):
    from vbq_amd import api
    api._CHECKED.clear()
    C, N = 3, 4
    A, B = IF._table("A", C, N), IF._table("B", C, N)
    r = IF.EDIT_ROUTES[route]
    table = r.form.make(A)
    lm, srt = api._device_table(table, C, N, "cpu", validate)
    first = (lm.numpy().copy(), srt.numpy().copy())
    assert all(np.array_equal(x, y) for x, y in zip(first, _pair_of(A)))
    again = api._device_table(table, C, N, "cpu", validate)
    assert again[0] is lm and again[1] is srt                                  # the same content: the pair that was prepared
    r.edit(table, B)
    lm2, srt2 = api._device_table(table, C, N, "cpu", validate)
    assert all(np.array_equal(x.numpy(), y) for x, y in zip((lm2, srt2), _pair_of(B))), f"{route}: the pair of the OLD content"
    assert not np.array_equal(srt2.numpy(), first[1])
    bad = B.copy()
    bad[1, 5] = 1e9
    r.edit(table, bad)
    if validate:
        with pytest.raises(ValueError, match="not monotone"):
            api._device_table(table, C, N, "cpu", validate)
    else:
        assert np.array_equal(api._device_table(table, C, N, "cpu", validate)[0].numpy(), bad)


@pytest.mark.parametrize("form", ["cpu_inference", "cpu_requires_grad", "cpu_float64", "cpu_strided", "np_reversed", "np_readonly",
                                  "np_fortran", "py_lists"])
def test_device_table_accepts_a_table_in_any_form(form):
    from vbq_amd import api
    api._CHECKED.clear()
    C, N = 3, 4
    A = IF._table("A", C, N)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        lm, srt = api._device_table(IF.FORMS[form].make(A), C, N, "cpu", True)
    assert all(np.array_equal(x.numpy(), y) for x, y in zip((lm, srt), _pair_of(A)))


# ====================================================================================================== 6. host-only calls
def _prior_arrays():
    from vbq_amd import priors
    return priors.BMSHJ2018Prior(3, seed=0).effective_parameters()


def _host_only_calls():
    """name of EXEMPT -> (call(array), the reference array).  Where a call takes several arrays the first is transformed."""
    from vbq_amd import api, coder, embeddings as E, metrics, priors
    from vbq_amd.baselines import KmeansQuantizer
    rng = np.random.default_rng(6)
    f = lambda shape: rng.uniform(0.1, 0.9, shape).astype(np.float32)
    counts = rng.integers(0, 50, (3, 31)).astype(np.int64)
    mats, biases, factors = _prior_arrays()
    fg = lambda mean: priors.FactoredGaussianPrior(mean, np.array([0.5, 1.0, 2.0], np.float32))

    def km_fit(samples):
        np.random.seed(0)                                      # (scikit-learn draws its initial centres from NumPy's global state)
        k = KmeansQuantizer(4)
        k.fit(samples)
        return k.code_points, k.code_lengths

    def set_weights(w0):
        p = priors.BMSHJ2018Prior(3, seed=0)
        p.set_weights([w0] + p.get_weights()[1:])
        return tuple(p.get_weights())
    return {
        "api.gaussian_table": (lambda s: api.gaussian_table(s, 4), f((2, 3))[0] + 0.5),
        "embeddings.analogy_metrics": (E.analogy_metrics, rng.integers(0, 50, 40).astype(np.int64)),
        "embeddings.entropy_from_counts": (E.entropy_from_counts, counts),
        "metrics.convert_to_db": (metrics.convert_to_db, f((2, 5))),
        "baselines.KmeansQuantizer.fit": (km_fit, rng.normal(0, 1, (50, 2)).astype(np.float32)),
        "priors.BMSHJ2018Prior.set_weights": (set_weights, mats[0] + 0.25),
        "priors.FactoredGaussianPrior.__init__": (lambda m: (fg(m).mean, fg(m).std, fg(m).logvar), f((2, 3))[0]),
        "priors.FactoredGaussianPrior.inverse_cdf": (lambda xi: fg(np.zeros(3, np.float32)).inverse_cdf(xi), f((5, 3))),
        "priors.FactoredGaussianPrior.logpdf": (lambda z: fg(np.zeros(3, np.float32)).logpdf(z), f((5, 3))),
        "priors.FactoredGaussianPrior.pdf": (lambda z: fg(np.zeros(3, np.float32)).pdf(z), f((5, 3))),
        "priors.StandardGaussianPrior.inverse_cdf": (priors.StandardGaussianPrior.inverse_cdf, f((5, 3))),
        "priors.StandardGaussianPrior.logpdf": (priors.StandardGaussianPrior.logpdf, f((5, 3))),
        "priors.StandardGaussianPrior.pdf": (priors.StandardGaussianPrior.pdf, f((5, 3))),
        "priors.log_normal_pdf": (lambda s: priors.log_normal_pdf(s, np.float32(0.5), np.float32(-1.0)), f((5, 3))),
        "priors.pack_bmshj_params": (lambda m0: priors.pack_bmshj_params([m0] + list(mats[1:]), biases, factors), mats[0]),
        "coder.exact_frequencies": (coder.exact_frequencies, counts),
        "coder.ideal_bits": (lambda c: coder.ideal_bits(c, coder.quantize_frequencies(counts)), counts),
        "coder.quantize_frequencies": (coder.quantize_frequencies, counts),
    }


HOST_ONLY_CALLS = tuple(n for n, r in IF.EXEMPT.items() if r == IF.HOST_ONLY)
LAYOUT_FORMS = ("np_every_second", "np_fortran", "np_reversed", "np_offset", "np_readonly")
"""These calls are the reference's own NumPy arithmetic: their result dtype follows the dtype they are given, so only the layout
is varied."""


@pytest.mark.parametrize("name", HOST_ONLY_CALLS)
def test_host_only_calls_under_the_layout_forms(name):
    fn, a = _host_only_calls()[name]
    want = fn(IF.NP_PLAIN.make(a))
    ran = 0
    for form in (IF.FORMS[n] for n in LAYOUT_FORMS):
        if form.applies(a):
            arg = form.make(a)
            before = IF.snapshot(arg)
            assert _same(fn(arg), want), f"{name} under {form.name}"
            assert IF.snapshot(arg) == before, f"{name} changed its argument under {form.name}"
            ran += 1
    assert ran >= 3, name
