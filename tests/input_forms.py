"""Every call answers for its inputs' VALUES, in whatever form they arrive: the forms, the edit routes and the catalogue.

The other suites hand the library one form of input: a fresh, C-contiguous float32 / int64 NumPy array or its .cuda() copy.
Callers pass slices, transposes, reversed and read-only arrays, float64 and float16 latents, nested lists, CPU tensors, tensors
that require grad or were made under torch.inference_mode() -- and buffers they refill in place between calls.

A FORM turns a plain reference array `a` into an argument: `form.make(a)`.  `form.values(a)` are the values that argument holds:
`a` itself except where the form's dtype cannot hold it (float16: `a` rounded to f16 and widened back).  THE EXPECTED ANSWER OF A
CALL UNDER A FORM IS ITS ANSWER UNDER THE PLAIN FORM OF values(a), bit for bit.  The plain form is the C-contiguous NumPy array
for host callers (NP_PLAIN) and its .cuda() copy where the contract is device tensors (DEV_PLAIN).  Forms are applied to one
argument at a time (all others stay plain), and once to every array argument together.  The slots a strided or offset form
leaves out hold other values OF THE SAME ARRAY (rolled by one): a call that reads them answers wrongly, never wildly.

An EDIT ROUTE overwrites an argument in place with other values, in a way torch's version counter does not see (EDIT_ROUTES):
the answer of the next call with the same object must follow the content.

The CATALOGUE (section c; a. and b. are quantizer_histories.PROBES and test_gpu_stream_order.CASES) names the public calls
outside the quantizer: ENTRIES[name] = Entry(base, params, build), build() -> (call, make) with make(which) the plain reference
arrays {parameter: array} of value set "A" or "B" and call(**arguments) the answer; every run of an entry gets objects of its
own.  `base` is "numpy" (NumPy, Python and CPU-tensor forms apply) or "device" (device forms apply).
COVERED maps every public callable with an array parameter to (entry, its array parameters); EXEMPT the others to one of
EXEMPT_REASONS; REFUSED the (entry, parameter, form) triples whose narrower contract the docstring or a header states, with the
exception type, a fragment of its message and the sentence.  A NEW PUBLIC CALL WITH AN ARRAY PARAMETER GOES INTO COVERED OR
EXEMPT; tests/test_input_forms_host.py enforces it.  Importable without a GPU (the builders import the library when called)."""
import collections

import numpy as np

F32, I64 = np.float32, np.int64


# ====================================================================================================== the forms
def _torch():
    import torch
    return torch


def _roll(a):
    return np.roll(a, 1, axis=-1) if a.ndim else a


def _wide(a):
    """A buffer of twice the last axis: `a` in the even slots, `a` rolled by one in the odd ones."""
    w = np.empty(a.shape[:-1] + (2 * a.shape[-1],), a.dtype)
    w[..., 0::2], w[..., 1::2] = a, _roll(a)
    return w


def _offset_buffer(a):
    """A flat buffer one element longer than `a`, 16-byte aligned, with `a` from element 1 on (element 0: the last of `a`)."""
    raw = np.empty((a.size + 1) * a.itemsize + 16, np.uint8)
    start = -raw.ctypes.data % 16
    buf = raw[start:start + (a.size + 1) * a.itemsize].view(a.dtype)
    buf[1:], buf[0] = a.reshape(-1), a.reshape(-1)[-1]
    return buf


def _np_second(a):
    return _wide(a)[..., 0::2]


def _np_fortran(a):
    return np.ascontiguousarray(a.T).T


def _np_reversed(a):
    return np.ascontiguousarray(a[::-1])[::-1]


def _np_offset(a):
    return _offset_buffer(a)[1:].reshape(a.shape)


def _np_readonly(a):
    b = a.copy()
    b.setflags(write=False)
    return b


def _f16(a):
    return a.astype(np.float16).astype(a.dtype)


def _cpu(a):
    return _torch().from_numpy(np.array(a, order="C"))


def _cpu_shared(a):
    """The tensor shares the memory of a NumPy array kept as `t.shared_array`: an edit of the array is an edit of the tensor."""
    arr = np.array(a, order="C")
    t = _torch().from_numpy(arr)
    t.shared_array = arr
    return t


def _cpu_inference(a):
    torch = _torch()
    with torch.inference_mode():
        return torch.from_numpy(np.array(a, order="C")).clone()


def _cpu_grad(a):
    return _cpu(a).requires_grad_(True)


def _dev(a):
    return _cpu(a).cuda()


def _dev_strided(a):
    return _cpu(_wide(a)).cuda()[..., 0::2]


def _dev_transposed(a):
    return _cpu(a.T).cuda().permute(*reversed(range(a.ndim)))


def _dev_offset(a):
    return _cpu(_offset_buffer(a)).cuda()[1:].view(a.shape)


def _dev_inference(a):
    torch = _torch()
    with torch.inference_mode():
        return _cpu(a).cuda().clone()


def _is(a, kinds):
    return a.dtype.kind in kinds


_ANY = lambda a: a.size > 0
_FLOAT = lambda a: a.size > 0 and _is(a, "f")
_INT = lambda a: a.size > 0 and _is(a, "iu")
_2D = lambda a: a.size > 0 and a.ndim >= 2 and min(a.shape) > 1

Form = collections.namedtuple("Form", "name family make applies values")
"""family: "numpy", "python", "cpu" or "device"; applies(a): whether the form can hold / differs from the plain form for `a`."""


def _form(name, family, make, applies=_ANY, values=None):
    return Form(name, family, make, applies, values or (lambda a: a))


NP_PLAIN = _form("np_plain", "numpy", lambda a: np.array(a, order="C"))
CPU_PLAIN = _form("cpu_plain", "cpu", _cpu)
DEV_PLAIN = _form("dev_plain", "device", _dev)

FORMS = {f.name: f for f in (
    # NumPy, layout
    _form("np_every_second", "numpy", _np_second, lambda a: a.size > 1 and a.shape[-1] > 1),
    _form("np_fortran", "numpy", _np_fortran, _2D),
    _form("np_reversed", "numpy", _np_reversed, lambda a: a.size > 1 and a.shape[0] > 1),
    _form("np_offset", "numpy", _np_offset),
    _form("np_readonly", "numpy", _np_readonly),
    # NumPy / Python, type
    _form("np_float64", "numpy", lambda a: a.astype(np.float64), _FLOAT),
    _form("np_float16", "numpy", lambda a: a.astype(np.float16), _FLOAT, _f16),
    _form("py_lists", "python", lambda a: a.tolist()),
    _form("np_int32", "numpy", lambda a: a.astype(np.int32), _INT),
    _form("np_uint8", "numpy", lambda a: a.astype(np.uint8), lambda a: _INT(a) and int(a.min()) >= 0 and int(a.max()) <= 255),
    # CPU torch
    CPU_PLAIN,
    _form("cpu_shared", "cpu", _cpu_shared),
    _form("cpu_strided", "cpu", lambda a: _cpu(_wide(a))[..., 0::2], lambda a: a.size > 1 and a.shape[-1] > 1),
    _form("cpu_float64", "cpu", lambda a: _cpu(a.astype(np.float64)), _FLOAT),
    _form("cpu_requires_grad", "cpu", _cpu_grad, _FLOAT),
    _form("cpu_inference", "cpu", _cpu_inference),
    # device torch
    _form("dev_strided", "device", _dev_strided, lambda a: a.size > 1 and a.shape[-1] > 1),
    _form("dev_transposed", "device", _dev_transposed, _2D),
    _form("dev_offset", "device", _dev_offset),
    _form("dev_float64", "device", lambda a: _dev(a.astype(np.float64)), _FLOAT),
    _form("dev_float16", "device", lambda a: _dev(a.astype(np.float16)), _FLOAT, _f16),
    _form("dev_requires_grad", "device", lambda a: _dev(a).requires_grad_(True), _FLOAT),
    _form("dev_inference", "device", _dev_inference),
)}

HOST_FAMILIES, DEVICE_FAMILIES = ("numpy", "python", "cpu"), ("device",)
DEVICE_LAYOUT_FORMS = ("dev_strided", "dev_transposed", "dev_offset")
"""What applies at the ops level, whose contract is the exact dtype."""

BASELINE = {"numpy": NP_PLAIN, "python": NP_PLAIN, "cpu": CPU_PLAIN, "device": DEV_PLAIN}
"""The form whose RETURN KIND a form of each family shares: the kind of the result (NumPy, CPU or device tensor) follows the kind
of the input, never its layout or dtype."""


def forms_for(base, a):
    """The forms that apply to the reference array `a` of an entry of `base`."""
    families = HOST_FAMILIES if base == "numpy" else DEVICE_FAMILIES
    return [f for f in FORMS.values() if f.family in families and f.applies(a) and f is not CPU_PLAIN]


def plain_of(base):
    return NP_PLAIN if base == "numpy" else DEV_PLAIN


# ---- what an argument is, for the check that a call left it alone
def snapshot(arg):
    """Type, dtype, shape, strides, flags and every byte of one argument."""
    if isinstance(arg, np.ndarray):
        return ("ndarray", arg.dtype.str, arg.shape, arg.strides, bool(arg.flags.writeable), arg.tobytes())
    if hasattr(arg, "data_ptr"):
        host = arg.detach().cpu()
        return ("tensor", str(arg.dtype), tuple(arg.shape), tuple(arg.stride()), str(arg.device), bool(arg.requires_grad),
                bool(arg.is_inference()), arg.data_ptr(), host.contiguous().reshape(-1).view(_torch().uint8).numpy().tobytes())
    return ("python", repr(arg))


def kinds(v):
    """The kind of every leaf of an answer: "ndarray", "tensor:cpu", "tensor:cuda" or the type's name."""
    if isinstance(v, dict):
        return tuple((k, kinds(x)) for k, x in v.items())
    if isinstance(v, (list, tuple)):
        return tuple(kinds(x) for x in v)
    if hasattr(v, "data_ptr"):
        return "tensor:" + v.device.type
    return "ndarray" if isinstance(v, np.ndarray) else type(v).__name__


# ====================================================================================================== the edit routes
def _as_dtype(t, b):
    return _torch().from_numpy(np.array(b, order="C")).to(t.dtype)


def _edit_numpy(arg, b):
    arg[...] = b


def _edit_shared(arg, b):
    arg.shared_array[...] = b


def _edit_data(arg, b):
    arg.data.copy_(_as_dtype(arg, b))


def _edit_dlpack(arg, b):
    _torch().from_dlpack(arg).copy_(_as_dtype(arg, b))


def _edit_out(arg, b):
    """One of the library's own out= writes: ops.transpose of the transposed values INTO the argument (f32 matrices); every other
    argument is written through .data."""
    torch = _torch()
    if arg.dtype == torch.float32 and arg.dim() == 2 and arg.is_contiguous():
        from vbq_amd import ops
        ops.transpose(_dev(np.ascontiguousarray(np.asarray(b, F32).T)), out=arg)
    else:
        _edit_data(arg, b)


Route = collections.namedtuple("Route", "name form edit")
EDIT_ROUTES = {r.name: r for r in (
    Route("numpy_assign", NP_PLAIN, _edit_numpy),                       # arg[...] = b
    Route("cpu_shared_array", FORMS["cpu_shared"], _edit_shared),      # the array behind torch.from_numpy(array)
    Route("cpu_data", CPU_PLAIN, _edit_data),                           # t.data.copy_(b)
    Route("device_data", DEV_PLAIN, _edit_data),
    Route("device_dlpack", DEV_PLAIN, _edit_dlpack),                    # torch.from_dlpack(t).copy_(b)
    Route("device_out_write", DEV_PLAIN, _edit_out),                    # ops.transpose(..., out=t)
)}
SILENT_ROUTES = ("cpu_shared_array", "cpu_data", "device_data", "device_dlpack", "device_out_write")
"""The routes that leave a tensor's _version where it was (tests/test_input_forms_host.py holds the CPU ones to it, the GPU module
the device ones)."""


def routes_for(base):
    return [r for r in EDIT_ROUTES.values() if (r.form.family == "device") == (base == "device")]


# ====================================================================================================== c. the catalogue
Entry = collections.namedtuple("Entry", "base params build")
ENTRIES = {}


def entry(name, base, params):
    def deco(fn):
        assert name not in ENTRIES, name
        ENTRIES[name] = Entry(base, tuple(params), fn)
        return fn
    return deco


N4, T4, K_ROW, BITS = 4, 31, 5, 11
SEED = {"A": 7, "B": 8}


def _book4(scale=1.0):
    from scipy.stats import norm
    from vbq_amd import tables as TB
    return (norm.ppf(TB.dyadic_xi(N4)) * scale).astype(F32)


def _table(which, C, N=N4):
    """gaussian_table at one scale per value set: B is another valid monotone table."""
    from vbq_amd import gaussian_table
    return gaussian_table(np.linspace(0.5, 2.0, C) * {"A": 1.0, "B": 1.7}[which], N)


def _mu_sigma(which, shape):
    rng = np.random.default_rng(SEED[which])
    return rng.normal(0, 1.2, shape).astype(F32), np.clip(np.exp(rng.normal(-2, 0.7, shape)), 1e-3, 10).astype(F32)


def _quantize_entry(name, base, shape, layout, C):
    @entry(name, base, ("mu", "sigma", "table", "lengths"))
    def _():
        import vbq_amd
        lam = [0.02, 0.7, 9.0]

        def make(which):
            mu, sigma = _mu_sigma(which, shape)
            rng = np.random.default_rng(SEED[which] + 17)
            lengths = (np.arange(N4 + 1, dtype=F32)[None, None] + rng.uniform(0, 3, (3, C, N4 + 1))).astype(F32)
            return dict(mu=mu, sigma=sigma, table=_table(which, C), lengths=lengths)

        def call(mu, sigma, table, lengths):
            return (vbq_amd.quantize(mu, sigma, lam, table=table, N=N4, lengths=lengths, layout=layout, return_values=True,
                                     return_bits=True),
                    vbq_amd.quantize(mu, sigma, lam[1], table=table, N=N4, layout=layout, out_layout="planes"))
        return call, make


for _base in ("numpy", "device"):
    _quantize_entry(f"quantize_bc[{_base}]", _base, (7, 3), "bc", 3)           # channel-last, C > 1: the plane kernels
    _quantize_entry(f"quantize_cb[{_base}]", _base, (3, 7), "cb", 3)
    _quantize_entry(f"quantize_one_channel[{_base}]", _base, (9,), "bc", 1)     # [n]: C = 1


def _rows_entry(name, base, fn_name, with_bits):
    @entry(name, base, ("mu", "sigma", "table") + (("total_bits",) if with_bits else ()))
    def _():
        import vbq_amd
        from vbq_amd import rows_budget

        def make(which):
            rng = np.random.default_rng(SEED[which])
            out = dict(mu=rng.normal(0, 1, (9, K_ROW)).astype(F32), sigma=rng.uniform(0.05, 1.0, (9, K_ROW)).astype(F32),
                       table=np.stack([_book4(s * {"A": 1.0, "B": 1.3}[which]) for s in (0.5, 1.0, 1.5, 2.0, 3.0)]))
            if with_bits:
                out["total_bits"] = np.array([BITS, 0, 3, K_ROW * N4, 7, BITS, 1, 12, 5], I64) if which == "A" else \
                    np.array([2, BITS, 4, 0, 9, 1, K_ROW * N4, 3, 6], I64)
            return out

        def call(mu, sigma, table, total_bits=None):
            if fn_name == "budget":
                return vbq_amd.quantize_rows_to_budget(mu, sigma, total_bits, table=table, N=N4)
            if fn_name == "budgets":
                return rows_budget.quantize_rows_to_budgets(mu, sigma, [BITS, 0, 20, BITS], table=table, N=N4)
            return rows_budget.budget_curve(mu, sigma, table=table, N=N4, max_bits=7)
        return call, make


for _base in ("numpy", "device"):
    _rows_entry(f"quantize_rows_to_budget[{_base}]", _base, "budget", True)
    _rows_entry(f"quantize_rows_to_budgets[{_base}]", _base, "budgets", False)
    _rows_entry(f"budget_curve[{_base}]", _base, "curve", False)


# ---- embeddings: dense matrices and record files
V_DENSE, K_DENSE, V_REC = 301, 7, 40


def _ids(which, shape, V, padding=True):
    ids = np.random.default_rng(SEED[which] + 3).integers(0, V, shape).astype(I64)
    if padding:
        ids.reshape(-1)[-1] = -1
    return ids


def _emb(which, V=V_DENSE, K=K_DENSE):
    return np.random.default_rng(SEED[which]).normal(0, 1, (V, K)).astype(F32)


def _queries(which, Q, K):
    return np.random.default_rng(SEED[which] + 1).normal(0, 1, (Q, K)).astype(F32)


def _record_file(which, rows=V_REC):
    from vbq_amd import embeddings as E
    rng = np.random.default_rng(SEED[which] + 5)
    m, s = rng.normal(0, 1, (rows, K_ROW)).astype(F32), rng.uniform(0.05, 1.0, (rows, K_ROW)).astype(F32)
    return E.compress_to_records(m, s, BITS, _book4(), N4)


def _search_entries(kind, base):
    """bag, scores, similarity, rerank, most_similar on a dense matrix (`emb` is a parameter) or a record file (the file of the
    value set is the object's state; its array parameters are the same without `emb`)."""
    from_file = kind == "records"
    V, K = (V_REC, K_ROW) if from_file else (V_DENSE, K_DENSE)
    head = () if from_file else ("emb",)

    def target(emb, which_file):
        from vbq_amd import embeddings as E
        if not from_file:
            return lambda name: (lambda *a, **kw: getattr(E, name)(emb, *a, **kw))
        re = E.RecordEmbeddings(_record_file(which_file))
        return lambda name: getattr(re, name)

    def with_emb(d, which):
        return d if from_file else dict(emb=_emb(which), **d)

    def reg(name, params, make, call):
        @entry(f"{kind}_{name}[{base}]", base, head + params)
        def _():
            def run(emb=None, **kw):
                return call(target(emb, "A"), **kw)
            return run, (lambda which: with_emb(make(which), which))

    offsets = {"A": np.array([0, 3, 3], I64), "B": np.array([0, 1, 6], I64)}
    reg("bag", ("ids", "offsets", "weights"),
        lambda w: dict(ids=_ids(w, (8,), V), offsets=offsets[w],
                       weights=np.random.default_rng(SEED[w]).uniform(0.5, 2, 8).astype(F32)),
        lambda t, ids, offsets, weights: (t("bag")(ids, offsets, weights=weights), t("bag")(ids, offsets, mode="max")))
    reg("bag_2d", ("ids",), lambda w: dict(ids=_ids(w, (3, 4), V)), lambda t, ids: t("bag")(ids, mode="mean"))
    reg("scores", ("queries", "ids"), lambda w: dict(queries=_queries(w, 3, K), ids=_ids(w, (3, 6), V)),
        lambda t, queries, ids: (t("scores")(queries, ids), t("scores")(queries, ids, metric="dot")))
    reg("similarity", ("a", "b"), lambda w: dict(a=_ids(w, (6,), V, False), b=_ids(w, (6,), V, False)[::-1].copy()),
        lambda t, a, b: t("similarity")(a, b))
    reg("rerank", ("queries", "ids"), lambda w: dict(queries=_queries(w, 3, K), ids=_ids(w, (3, 6), V)),
        lambda t, queries, ids: t("rerank")(queries, ids, k=4))
    reg("most_similar", ("queries", "exclude"),
        lambda w: dict(queries=_queries(w, 3, K), exclude=np.array([[1, -1], [7, 8], [0, 0]], I64) + (w == "B")),
        lambda t, queries, exclude: t("most_similar")(queries, k=3, exclude=exclude))
    if from_file:
        reg("most_similar_ids", ("ids",), lambda w: dict(ids=_ids(w, (2,), V, False)),
            lambda t, ids: t("most_similar")(ids=ids, k=3, metric="dot"))
        reg("rows", ("ids",), lambda w: dict(ids=_ids(w, (5,), V, False)), lambda t, ids: t("rows")(ids))


_search_entries("dense", "numpy")
_search_entries("dense", "device")
_search_entries("records", "numpy")


@entry("compressed_embeddings_rows[numpy]", "numpy", ("ids",))
def _():
    from vbq_amd import embeddings as E
    rng = np.random.default_rng(4)
    m, s = rng.normal(0, 1, (60, 6)).astype(F32), rng.uniform(0.05, 1.0, (60, 6)).astype(F32)
    cp = E.make_code_book(1.0, N4)[0]
    data = E.compress_to_bytes(m, s, 17.0, cp, segment=5)
    return (lambda ids: E.CompressedEmbeddings(data).rows(ids)), (lambda w: dict(ids=_ids(w, (6,), 60, False)))


def _records_entry(name, base, run):
    @entry(f"{name}[{base}]", base, ("means", "stds", "codepoints"))
    def _():
        from vbq_amd import embeddings as E

        def make(which):
            rng = np.random.default_rng(SEED[which] + 5)
            return dict(means=rng.normal(0, 1, (V_REC, K_ROW)).astype(F32), stds=rng.uniform(0.05, 1.0, (V_REC, K_ROW)).astype(F32),
                        codepoints=_book4({"A": 1.0, "B": 1.3}[which]))
        return (lambda means, stds, codepoints: run(E, means, stds, codepoints)), make


def _quality(E, m, s, cp):
    curve = E.records_distortion_curve(m, s, cp, N4)
    return E.compress_to_records_quality(m, s, cp, float(np.sort(curve)[len(curve) // 3]), N4)


for _base in ("numpy", "device"):
    _records_entry("compress_to_records", _base, lambda E, m, s, cp: E.compress_to_records(m, s, BITS, cp, N4))
    _records_entry("compress_to_records_sweep", _base, lambda E, m, s, cp: E.compress_to_records_sweep(m, s, [BITS, 0, 20], cp, N4))
    _records_entry("compress_to_records_budget", _base, lambda E, m, s, cp: E.compress_to_records_budget(m, s, cp, 400, N4))
    _records_entry("compress_to_records_quality", _base, _quality)
    _records_entry("records_distortion_curve", _base, lambda E, m, s, cp: E.records_distortion_curve(m, s, cp, N4))


for _base in ("numpy", "device"):
    @entry(f"prediction_ranks[{_base}]", _base, ("emb", "analogies_id"))
    def _():
        from vbq_amd import embeddings as E
        return (lambda emb, analogies_id: E.prediction_ranks(emb, analogies_id),
                lambda w: dict(emb=_emb(w, V_DENSE, 50), analogies_id=_ids(w, (37, 4), V_DENSE, False)))


# ---- k-means and the baseline quantizers
def _samples(which, B, C):
    return np.random.default_rng(SEED[which] + 2).normal(0, 1, (B, C)).astype(F32)


for _base in ("numpy", "device"):
    @entry(f"kmeans1d[{_base}]", _base, ("samples",))
    def _():
        from vbq_amd import kmeans1d
        return (lambda samples: (kmeans1d.prefix_sums(samples), kmeans1d.fit_channels(samples, [6, 2, 17, 2, 1]),
                                 kmeans1d.sse_curve(samples, 17)),
                lambda w: dict(samples=_samples(w, 257, 3)))


@entry("uniform_quantizer[numpy]", "numpy", ("fit_samples", "samples"))
def _():
    from vbq_amd import baselines

    def call(fit_samples, samples):
        u = baselines.UniformQuantizer(16)
        u.fit(fit_samples)
        return u.code_points, u.code_lengths, u.quantize(samples)
    return call, lambda w: dict(fit_samples=_samples(w, 1031, 1)[:, 0].copy(), samples=_samples(w, 77, 2))


@entry("optimal_kmeans_quantizer[numpy]", "numpy", ("fit_samples", "samples"))
def _():
    from vbq_amd import baselines

    def call(fit_samples, samples):
        k = baselines.OptimalKmeansQuantizer(4)
        k.fit(fit_samples)
        return k.code_points, k.code_lengths, k.quantize(samples)
    return call, lambda w: dict(fit_samples=_samples(w, 300, 1)[:, 0].copy(), samples=_samples(w, 77, 2))


class ArrayVAE:
    """encode hands back the means it was built on, in the very form they were given in (NumPy or tensor, any layout); decode
    is a fixed map of the latents."""

    def __init__(self, means):
        self.means = means

    def encode(self, X):
        return self.means, None

    def decode(self, Z):
        Z = Z.detach().cpu().numpy() if hasattr(Z, "detach") else np.asarray(Z)
        return (0.1 * Z.mean(axis=-1, keepdims=True) + 0.5).repeat(3, axis=-1)


@entry("optimal_kmeans_wrapper[numpy]", "numpy", ("fit_means", "means"))
def _():
    """ChannelwiseOptimalKmeansWrapper.fit / .compress: the arrays are the posterior means the VAE's encoder returns."""
    import vbq_amd
    levels = [2, 4, 6]
    X = np.random.default_rng(9).random((2, 8, 8, 3)).astype(F32)

    def make(which):
        rng = np.random.default_rng(SEED[which] + 9)
        return dict(fit_means=rng.normal(0, 1, (2, 8, 8, 3)).astype(F32), means=rng.normal(0, 1, (2, 8, 8, 3)).astype(F32))

    def call(fit_means, means):
        w = vbq_amd.ChannelwiseOptimalKmeansWrapper(3, levels)
        w.fit(X, ArrayVAE(fit_means), 1.0)
        return w.code_points, w.code_lengths, w.compress(X, ArrayVAE(means), levels, clip=True)
    return call, make


@entry("simple_quantizer_wrappers[numpy]", "numpy", ("fit_means", "means"))
def _():
    """ChannelwiseSimpleQuantizer and ChannelwiseSimpleQuantizerWrapper over UniformQuantizer: every channel's column (a strided
    view of the means) goes to the scalar quantizer."""
    from vbq_amd import baselines
    levels = [4, 8]
    X = np.random.default_rng(9).random((2, 8, 8, 3)).astype(F32)

    def make(which):
        rng = np.random.default_rng(SEED[which] + 9)
        return dict(fit_means=rng.normal(0, 1, (2, 8, 8, 3)).astype(F32), means=rng.normal(0, 1, (2, 8, 8, 3)).astype(F32))

    def call(fit_means, means):
        w = baselines.ChannelwiseSimpleQuantizerWrapper(baselines.UniformQuantizer, 3, levels)
        w.fit(X, ArrayVAE(fit_means), 1.0)
        one = baselines.ChannelwiseSimpleQuantizer(baselines.UniformQuantizer, 3, 8)
        one.fit(X, ArrayVAE(fit_means), 1.0)
        return (w.compress(X, ArrayVAE(means), levels, clip=True), one.code_points, one.code_lengths,
                one.compress(X, ArrayVAE(means), clip=False))
    return call, make


# ---- metrics, priors, the latent store, the coder
def _image_pair(which, dtype):
    rng = np.random.default_rng(SEED[which])
    a = rng.integers(0, 256, (2, 24, 20, 3))
    b = np.clip(a + rng.integers(-9, 10, a.shape), 0, 255)
    return (a.astype(np.uint8), b.astype(np.uint8)) if dtype == np.uint8 else ((a / 255).astype(F32), (b / 255).astype(F32))


for _base in ("numpy", "device"):
    for _dt, _tag in ((np.uint8, "u8"), (F32, "f32")):
        @entry(f"metrics_{_tag}[{_base}]", _base, ("img1", "img2"))
        def _(_dt=_dt):
            from vbq_amd import metrics
            mx = 255 if _dt == np.uint8 else 1.0
            return (lambda img1, img2: (metrics.mse(img1, img2), metrics.psnr(img1, img2, max_val=mx),
                                        metrics.ms_ssim(img1, img2, max_val=mx, weights=[0.3, 0.7])),
                    lambda w: dict(zip(("img1", "img2"), _image_pair(w, _dt))))


def _bmshj():
    from vbq_amd import priors
    p = priors.BMSHJ2018Prior(3, init_scale=10.0, seed=0)
    rng = np.random.default_rng(1000)
    p.set_weights([w + rng.normal(0, 0.3, w.shape).astype(F32) for w in p.get_weights()])
    return p


for _base in ("numpy", "device"):
    @entry(f"bmshj_prior[{_base}]", _base, ("inputs", "xi", "data"))
    def _():
        def make(which):
            rng = np.random.default_rng(SEED[which])
            return dict(inputs=rng.normal(0, 3, (37, 3)).astype(F32), xi=rng.uniform(0.02, 0.98, (37, 3)).astype(F32),
                        data=rng.normal(0, 2, (41, 3)).astype(F32))

        def call(inputs, xi, data):
            p = _bmshj()
            out = (p.cdf(inputs), p.pdf(inputs), p.logpdf(inputs), p.cdf_pdf(inputs), p.inverse_cdf(xi))
            record = p.fit(data, its=2, logging_freq=1)
            return out + (tuple((r["it"], r["loss"]) for r in record), tuple(p.get_weights()))
        return call, make


BOX = (1, 2, 3)


for _base in ("numpy", "device"):
    @entry(f"latent_store[{_base}]", _base, ("ids", "origins"))
    def _(_base_of_store=_base):
        import quantizer_histories as QH
        from vbq_amd.store import LatentStore
        q = QH.fresh(QH.STATES["A"])
        inp = QH.Inputs(sorted(QH.LAMBS_A), QH.latents(QH.FILE_SHAPES), QH.class_maps(QH.FILE_SHAPES, 2),
                        QH.class_maps(QH.FILE_SHAPES, 3), {}, "store")
        files = [QH.written(q, inp, "b", f) for f in (0, 2)]                   # 24 x 24 and 3 x 5 positions

        def make(which):
            return dict(ids=np.array([0, 1, 0, 0, 1], I64) if which == "A" else np.array([1, 0, 0, 1, 0], I64),
                        origins=np.array([[0, 3, 5], [0, 0, 1], [0, 20, 21], [0, 0, 0], [0, 1, 2]], I64) if which == "A"
                        else np.array([[0, 1, 0], [0, 7, 9], [0, 11, 2], [0, 0, 2], [0, 21, 20]], I64))
        device = _base_of_store == "device"

        def call(ids, origins):
            from vbq_amd import store
            st = LatentStore(q, files)
            out, status = st.crops(ids, origins, BOX, channels=[2, 0])
            st.check(status, ids)
            plan = store.plan_boxes(st._table, ids, origins, BOX, seg=st.segment, n_sel=st._n_sel(BOX)) if device else ()
            return (out, status, st.read(ids, origins, BOX), st.read(ids, origins, BOX, return_np=True)) + tuple(plan)
        return call, make


@entry("rans_codec_tables[numpy]", "numpy", ("freq",))
def _():
    from vbq_amd import coder
    idx = np.random.default_rng(7).integers(0, T4, (3, 75)).astype(np.uint16)

    def call(freq):
        codec = coder.RansCodec(freq, N=N4, segment=32)
        words, sizes = codec.encode(_dev(idx))
        return words, sizes, codec.decode(words, sizes, 75), codec.freq_host
    return call, lambda w: dict(freq=coder.quantize_frequencies(np.random.default_rng(SEED[w]).integers(0, 50, (3, T4))))


@entry("mapped_codec_tables[numpy]", "numpy", ("freq", "cls"))
def _():
    from vbq_amd import coder
    idx = np.random.default_rng(7).integers(0, T4, (2, 3, 75)).astype(np.uint16)

    def make(w):
        rng = np.random.default_rng(SEED[w])
        return dict(freq=coder.quantize_frequencies(rng.integers(0, 50, (2, 3, T4))), cls=rng.integers(0, 2, 75).astype(I64))

    def call(freq, cls):
        codec = coder.MappedRansCodec(freq, N=N4, segment=32)
        words, sizes = codec.encode(_dev(idx), cls)
        sz, payload = codec.encode_packed(_dev(idx), cls)
        return (words, sizes, codec.sizes(_dev(idx), cls), codec.decode(words, sizes, cls, 75), sz, payload,
                codec.decode_packed(_dev(payload), _dev(sz.astype(np.uint16)), cls, 75))
    return call, make


@entry("rans_packed_forms[device]", "device", ("words", "sizes", "payload", "packed_sizes"))
def _():
    """RansCodec.pack / pack_device / compressed_bits / decode on the words and sizes an encoder wrote, unpack_device /
    decode_packed on its packed payload (ops level: exact dtype).  Of the payload only the first `total` words are valid (vbq_amd/coder.py), and of a segment's words the first
    sizes[g]: both are cut to that."""
    from vbq_amd import coder

    def codec():
        return coder.RansCodec(coder.quantize_frequencies(np.random.default_rng(1).integers(0, 50, (3, T4))), N=N4, segment=32)

    def make(w):
        idx = np.random.default_rng(SEED[w]).integers(0, T4, (3, 75)).astype(np.uint16)
        words, sizes = codec().encode(_dev(idx))
        words, sizes = words.cpu().numpy(), sizes.cpu().numpy()
        sz, packed = codec().encode_packed(_dev(idx))
        return dict(words=valid(words, sizes), sizes=sizes, payload=np.asarray(packed), packed_sizes=np.asarray(sz).astype(np.uint16))

    def valid(words, sizes):
        keep = np.arange(words.shape[-1])[None, :] < sizes.reshape(-1).astype(I64)[:, None]
        return np.where(keep.reshape(words.shape), words, 0).astype(words.dtype)

    def call(words, sizes, payload, packed_sizes):
        c = codec()
        w2, s2, status = c.unpack_device(payload, packed_sizes, 75)
        unpacked = (valid(w2.cpu().numpy(), s2.cpu().numpy()), s2, status, c.decode_packed(payload, packed_sizes, 75))
        return unpacked + packed_forms(c, words, sizes)

    def packed_forms(c, words, sizes):
        payload, total, offsets = c.pack_device(words, sizes)
        n = int(total.cpu().to(_torch().int64).reshape(-1)[0])
        return (payload[:n], total, offsets, coder.RansCodec.pack(words, sizes), coder.RansCodec.compressed_bits(sizes),
                c.decode(words, sizes, 75))
    return call, make


@entry("entropy_from_indices[device]", "device", ("idx",))
def _():
    from vbq_amd import embeddings as E
    return (lambda idx: E.entropy_from_indices(idx, N4),
            lambda w: dict(idx=np.random.default_rng(SEED[w]).integers(0, T4, (60, 6)).astype(np.uint16)))


@entry("kmeans1d_ops[device]", "device", ("S1", "S2", "shift", "x", "codes"))
def _():
    """kmeans1d_dp and nearest_code_channels (ops level: exact dtype)."""
    from vbq_amd import kmeans1d

    def make(w):
        x = _samples(w, 257, 3)
        _, shift, S1, S2 = kmeans1d.prefix_sums(x)
        codes = np.sort(np.random.default_rng(SEED[w]).normal(0, 1, (3, 5)), axis=1)
        return dict(S1=S1.cpu().numpy(), S2=S2.cpu().numpy(), shift=shift.cpu().numpy(), x=x[:65].copy(), codes=codes)

    def call(S1, S2, shift, x, codes):
        return kmeans1d.kmeans1d_dp(S1, S2, shift, [1, 5, 16]) + kmeans1d.nearest_code_channels(x, codes)
    return call, make


@entry("level_candidates[device]", "device", ("mu_t", "sg_t", "tab_lm"))
def _():
    from vbq_amd import rows_budget

    def make(w):
        rng = np.random.default_rng(SEED[w])
        return dict(mu_t=rng.normal(0, 1, (9, K_ROW)).astype(F32), sg_t=rng.uniform(0.05, 1.0, (9, K_ROW)).astype(F32),
                    tab_lm=np.stack([_book4(s * {"A": 1.0, "B": 1.3}[w]) for s in (0.5, 1.0, 1.5, 2.0, 3.0)]))
    return (lambda mu_t, sg_t, tab_lm: rows_budget.level_candidates(mu_t, sg_t, tab_lm, N4)), make


def _vbqe_entry(name, base, run):
    @entry(f"{name}[{base}]", base, ("means", "stds", "codepoints"))
    def _():
        from vbq_amd import embeddings as E

        def make(which):
            rng = np.random.default_rng(SEED[which] + 4)
            return dict(means=rng.normal(0, 1, (60, 6)).astype(F32), stds=rng.uniform(0.05, 1.0, (60, 6)).astype(F32),
                        codepoints=E.make_code_book({"A": 1.0, "B": 1.3}[which], N4)[0])
        return (lambda means, stds, codepoints: run(E, means, stds, codepoints)), make


_BETAS = [0.6, 17.0, 1e3]
for _base in ("numpy", "device"):
    _vbqe_entry("compress_to_bytes", _base, lambda E, m, s, cp: E.compress_to_bytes(m, s, 17.0, cp, segment=5))
    _vbqe_entry("coded_nbytes", _base, lambda E, m, s, cp: E.coded_nbytes(m, s, _BETAS, cp, segment=5))
    _vbqe_entry("compress_to_budget", _base, lambda E, m, s, cp: E.compress_to_budget(m, s, cp, 10 ** 6, betas=_BETAS, segment=5))
    _vbqe_entry("compress_coordinates", _base, lambda E, m, s, cp: E.compress_coordinates(m, s, 17.0, codepoints=cp))
    _vbqe_entry("compress_coordinates_sweep", _base, lambda E, m, s, cp: E.compress_coordinates_sweep(m, s, _BETAS, cp))


for _base in ("numpy", "device"):
    @entry(f"embedding_statistics[{_base}]", _base, ("vecs", "means"))
    def _():
        """empirical_std, empirical_entropy and quantize_coordinates: reductions of one matrix."""
        from vbq_amd import embeddings as E

        def make(w):
            rng = np.random.default_rng(SEED[w])
            return dict(vecs=rng.normal(0, 1, (60, 6)).astype(F32), means=np.round(rng.normal(0, 2, (60, 6))).astype(F32))
        return (lambda vecs, means: (E.empirical_std(vecs), E.empirical_entropy(means), E.quantize_coordinates(vecs, 4))), make


# ====================================================================================================== the tables
_DTYPE = "expected dtype"
_OPS_F64 = ("include/vbq_kmeans.h / vbq_amd/kmeans1d.py", "S1, S2 (f64 [C, n + 1]) and shift (f64 [C])")
REFUSED = {
    # (entry, parameter, form) -> (exception type, a fragment of its message, (file, the sentence that states the contract))
    **{(f"kmeans1d[{base}]", "samples", form): (ValueError, "float64 samples are not supported",
                                                ("vbq_amd/kmeans1d.py", "(host or device, float32)"))
       for base, form in (("numpy", "np_float64"), ("numpy", "cpu_float64"), ("device", "dev_float64"))},
    **{(e, p, form): (ValueError, "float64 samples are not supported",
                      ("vbq_amd/baselines.py", "float64 samples are not supported: the comparison quantizers run in float32"))
       for e in ("uniform_quantizer[numpy]", "optimal_kmeans_quantizer[numpy]") for p in ("fit_samples", "samples")
       for form in ("np_float64", "cpu_float64")},
    **{("optimal_kmeans_wrapper[numpy]", "fit_means", form): (
        ValueError, "float64 samples are not supported", ("vbq_amd/kmeans1d.py", "(host or device, float32)"))
       for form in ("np_float64", "cpu_float64")},
    **{("simple_quantizer_wrappers[numpy]", p, form): (
        ValueError, "float64 samples are not supported",
        ("vbq_amd/baselines.py", "float64 samples are not supported: the comparison quantizers run in float32"))
       for p in ("fit_means", "means") for form in ("np_float64", "cpu_float64")},
    **{("level_candidates[device]", p, form): (ValueError, _DTYPE, ("vbq_amd/rows_budget.py", "are f32 device tensors (ValueError for another dtype)"))
       for p in ("mu_t", "sg_t", "tab_lm") for form in ("dev_float64", "dev_float16")},
    **{("kmeans1d_ops[device]", p, "dev_float16"): (ValueError, _DTYPE, _OPS_F64) for p in ("S1", "S2", "shift")},
    **{("kmeans1d_ops[device]", "x", form): (ValueError, _DTYPE, ("vbq_amd/kmeans1d.py", "x f32 [B, C] channel-last, codes f64 [C, k]"))
       for form in ("dev_float16", "dev_float64")},
    ("kmeans1d_ops[device]", "codes", "dev_float16"): (ValueError, _DTYPE, ("vbq_amd/kmeans1d.py", "codes f64 [C, k]")),
}

NOT_EDITABLE = {"rans_packed_forms[device]": "the length of a packed payload follows its content: values B do not fit the buffers of A"}
"""Entries left out of the in-place edits, each with its reason."""

TAKES_NO_ARRAY, MULTI_GPU = "takes no array", "multi-GPU only"
HOST_ONLY = "host-only, covered in test_input_forms_host.py::test_host_only_calls_under_the_layout_forms"
"""dirty_memory.HOST_ONLY, naming this suite's host test."""


def exempt_reasons():
    import dirty_memory as DM
    return (TAKES_NO_ARRAY, MULTI_GPU, HOST_ONLY) + tuple(r for r in DM.EXEMPT_REASONS if r != DM.HOST_ONLY)


MODULES = ("api", "rows_budget", "embeddings", "kmeans1d", "baselines", "metrics", "priors", "coder")
"""The modules whose public callables COVERED and EXEMPT account for, with store.LatentStore and the quantizer (through
quantizer_histories.PROBED: every probe is run under the forms, section a)."""

_LAT = ("means", "stds", "codepoints")
COVERED = {
    # public callable -> (the catalogue entry that calls it -- of section c, or a case of test_gpu_stream_order.CASES --, the
    # array parameters of the callable that the entry transforms)
    "api.quantize": ("quantize_bc[numpy]", ("mu", "sigma", "table", "lengths")),
    "rows_budget.quantize_rows_to_budget": ("quantize_rows_to_budget[numpy]", ("mu", "sigma", "total_bits", "table")),
    "rows_budget.quantize_rows_to_budgets": ("quantize_rows_to_budgets[numpy]", ("mu", "sigma", "table")),
    "rows_budget.budget_curve": ("budget_curve[numpy]", ("mu", "sigma", "table")),
    "rows_budget.level_candidates": ("level_candidates[device]", ("mu_t", "sg_t", "tab_lm")),
    "embeddings.bag": ("dense_bag[numpy]", ("emb", "ids", "offsets", "weights")),
    "embeddings.scores": ("dense_scores[numpy]", ("emb", "queries", "ids")),
    "embeddings.similarity": ("dense_similarity[numpy]", ("emb", "a", "b")),
    "embeddings.rerank": ("dense_rerank[numpy]", ("emb", "queries", "ids")),
    "embeddings.most_similar": ("dense_most_similar[numpy]", ("emb", "queries", "exclude")),
    "embeddings.RecordEmbeddings.bag": ("records_bag[numpy]", ("ids", "offsets", "weights")),
    "embeddings.RecordEmbeddings.scores": ("records_scores[numpy]", ("queries", "ids")),
    "embeddings.RecordEmbeddings.similarity": ("records_similarity[numpy]", ("a", "b")),
    "embeddings.RecordEmbeddings.rerank": ("records_rerank[numpy]", ("queries", "ids")),
    "embeddings.RecordEmbeddings.most_similar": ("records_most_similar[numpy]", ("queries", "ids", "exclude")),
    "embeddings.RecordEmbeddings.rows": ("records_rows[numpy]", ("ids",)),
    "embeddings.CompressedEmbeddings.rows": ("compressed_embeddings_rows[numpy]", ("ids",)),
    "embeddings.compress_to_records": ("compress_to_records[numpy]", _LAT),
    "embeddings.compress_to_records_sweep": ("compress_to_records_sweep[numpy]", _LAT),
    "embeddings.compress_to_records_budget": ("compress_to_records_budget[numpy]", _LAT),
    "embeddings.compress_to_records_quality": ("compress_to_records_quality[numpy]", _LAT),
    "embeddings.records_distortion_curve": ("records_distortion_curve[numpy]", _LAT),
    "embeddings.compress_to_bytes": ("compress_to_bytes[numpy]", _LAT),
    "embeddings.coded_nbytes": ("coded_nbytes[numpy]", _LAT),
    "embeddings.compress_to_budget": ("compress_to_budget[numpy]", _LAT),
    "embeddings.compress_coordinates": ("compress_coordinates[numpy]", _LAT),
    "embeddings.compress_coordinates_sweep": ("compress_coordinates_sweep[numpy]", _LAT),
    "embeddings.prediction_ranks": ("prediction_ranks[numpy]", ("emb", "analogies_id")),
    "embeddings.empirical_std": ("embedding_statistics[numpy]", ("vecs",)),
    "embeddings.empirical_entropy": ("embedding_statistics[numpy]", ("values",)),
    "embeddings.quantize_coordinates": ("embedding_statistics[numpy]", ("means",)),
    "embeddings.entropy_from_indices": ("entropy_from_indices[device]", ("idx",)),
    "kmeans1d.prefix_sums": ("kmeans1d[numpy]", ("samples",)),
    "kmeans1d.fit_channels": ("kmeans1d[numpy]", ("samples",)),
    "kmeans1d.sse_curve": ("kmeans1d[numpy]", ("samples",)),
    "kmeans1d.kmeans1d_dp": ("kmeans1d_ops[device]", ("S1", "S2", "shift")),
    "kmeans1d.nearest_code_channels": ("kmeans1d_ops[device]", ("x", "codes")),
    "baselines.UniformQuantizer.fit": ("uniform_quantizer[numpy]", ("samples",)),
    "baselines.UniformQuantizer.quantize": ("uniform_quantizer[numpy]", ("samples",)),
    "baselines.OptimalKmeansQuantizer.fit": ("optimal_kmeans_quantizer[numpy]", ("samples",)),
    "baselines.KmeansQuantizer.quantize": ("optimal_kmeans_quantizer[numpy]", ("samples",)),
    # (fit / compress hand X to vae.encode and take its means: the arrays are those of fit_latents / compress_latents)
    "baselines.ChannelwiseOptimalKmeansWrapper.fit": ("optimal_kmeans_wrapper[numpy]", ()),
    "baselines.ChannelwiseOptimalKmeansWrapper.compress": ("optimal_kmeans_wrapper[numpy]", ()),
    "baselines.ChannelwiseSimpleQuantizer.fit": ("simple_quantizer_wrappers[numpy]", ()),
    "baselines.ChannelwiseSimpleQuantizer.compress": ("simple_quantizer_wrappers[numpy]", ()),
    "baselines.ChannelwiseSimpleQuantizer.fit_latents": ("simple_quantizer_wrappers[numpy]", ("posterior_means",)),
    "baselines.ChannelwiseSimpleQuantizer.compress_latents": ("simple_quantizer_wrappers[numpy]", ("posterior_means",)),
    "baselines.ChannelwiseSimpleQuantizerWrapper.fit": ("simple_quantizer_wrappers[numpy]", ()),
    "baselines.ChannelwiseSimpleQuantizerWrapper.compress": ("simple_quantizer_wrappers[numpy]", ()),
    "baselines.ChannelwiseOptimalKmeansWrapper.fit_latents": ("optimal_kmeans_wrapper[numpy]", ("posterior_means",)),
    "baselines.ChannelwiseOptimalKmeansWrapper.compress_latents": ("optimal_kmeans_wrapper[numpy]", ("posterior_means",)),
    "metrics.mse": ("metrics_u8[numpy]", ("img1", "img2")),
    "metrics.psnr": ("metrics_u8[numpy]", ("img1", "img2")),
    "metrics.ms_ssim": ("metrics_u8[numpy]", ("img1", "img2")),
    "priors.BMSHJ2018Prior.cdf": ("bmshj_prior[numpy]", ("inputs",)),
    "priors.BMSHJ2018Prior.pdf": ("bmshj_prior[numpy]", ("inputs",)),
    "priors.BMSHJ2018Prior.logpdf": ("bmshj_prior[numpy]", ("inputs",)),
    "priors.BMSHJ2018Prior.cdf_pdf": ("bmshj_prior[numpy]", ("inputs",)),
    "priors.BMSHJ2018Prior.inverse_cdf": ("bmshj_prior[numpy]", ("xi",)),
    "priors.BMSHJ2018Prior.fit": ("bmshj_prior[numpy]", ("data",)),
    "priors.BMSHJ2018Prior.loss_and_grads": ("bmshj_loss_and_grads", ("x_cb",)),
    "coder.RansCodec.__init__": ("rans_codec_tables[numpy]", ("freq",)),
    "coder.RansCodec.encode": ("rans_encode", ("idx",)),
    "coder.RansCodec.sizes": ("rans_encode", ("idx",)),
    "coder.RansCodec.decode": ("rans_packed_forms[device]", ("words", "sizes")),
    "coder.RansCodec.encode_packed": ("rans_codec", ("idx",)),
    "coder.RansCodec.decode_packed": ("rans_packed_forms[device]", ("payload", "sizes")),
    "coder.RansCodec.unpack_device": ("rans_packed_forms[device]", ("payload", "sizes")),
    "coder.RansCodec.sizes_interleaved": ("interleaved_sizes", ("idx",)),
    "coder.RansCodec.encode_interleaved": ("interleaved_codec", ("idx",)),
    "coder.RansCodec.decode_interleaved": ("interleaved_codec", ("payload", "sizes")),
    "coder.RansCodec.pack": ("rans_packed_forms[device]", ("words", "sizes")),
    "coder.RansCodec.pack_device": ("rans_packed_forms[device]", ("words", "sizes")),
    "coder.RansCodec.compressed_bits": ("rans_packed_forms[device]", ("sizes",)),
    "coder.MappedRansCodec.__init__": ("mapped_codec_tables[numpy]", ("freq",)),
    "coder.MappedRansCodec.encode": ("mapped_codec_tables[numpy]", ("cls",)),
    "coder.MappedRansCodec.sizes": ("mapped_codec_tables[numpy]", ("cls",)),
    "coder.MappedRansCodec.decode": ("mapped_codec_tables[numpy]", ("cls",)),
    "coder.MappedRansCodec.encode_packed": ("mapped_codec_tables[numpy]", ("cls",)),
    "coder.MappedRansCodec.decode_packed": ("mapped_codec_tables[numpy]", ("cls",)),
    "store.LatentStore.crops": ("latent_store[numpy]", ("ids", "origins")),
    "store.LatentStore.read": ("latent_store[numpy]", ("ids", "origins")),
    "store.LatentStore.check": ("latent_store[numpy]", ("ids",)),
    "store.plan_boxes": ("latent_store[device]", ("ids", "origins")),
}

_EVAL = "evaluation harness (utils.evaluate_*), frozen"
EXEMPT = {
    **{name: TAKES_NO_ARRAY for name in (
        "embeddings.CompressedEmbeddings.__init__", "embeddings.CompressedEmbeddings.tensor", "embeddings.RecordEmbeddings.__init__",
        "embeddings.RecordEmbeddings.tensor", "embeddings.decompress", "embeddings.default_segment", "embeddings.make_code_book",
        "baselines.ChannelwiseOptimalKmeansWrapper.__init__", "baselines.ChannelwiseSimpleQuantizer.__init__",
        "baselines.ChannelwiseSimpleQuantizerWrapper.__init__", "baselines.KmeansQuantizer.__init__",
        "baselines.UniformQuantizer.__init__", "priors.BMSHJ2018Prior.__init__", "priors.BMSHJ2018Prior.effective_parameters",
        "priors.BMSHJ2018Prior.get_weights", "priors.BMSHJ2018Prior.load_weights", "priors.BMSHJ2018Prior.save_weights",
        "store.LatentStore.__init__", "store.LatentStore.sample", "store.LatentStore.verify", "store.file_dims",
        "store.max_listed_segments")},
    # the notebook's evaluation loops (each a chain of covered calls around prediction_ranks)
    **{name: _EVAL for name in (
        "embeddings.test_beta", "embeddings.test_betas", "embeddings.test_quantization", "embeddings.test_total_bits")},
    **{name: HOST_ONLY for name in (
        "api.gaussian_table", "embeddings.analogy_metrics", "embeddings.entropy_from_counts", "metrics.convert_to_db",
        "baselines.KmeansQuantizer.fit", "priors.BMSHJ2018Prior.set_weights", "priors.FactoredGaussianPrior.__init__",
        "priors.FactoredGaussianPrior.inverse_cdf", "priors.FactoredGaussianPrior.logpdf", "priors.FactoredGaussianPrior.pdf",
        "priors.StandardGaussianPrior.inverse_cdf", "priors.StandardGaussianPrior.logpdf", "priors.StandardGaussianPrior.pdf",
        "priors.log_normal_pdf", "priors.pack_bmshj_params", "coder.exact_frequencies", "coder.ideal_bits",
        "coder.quantize_frequencies")},
}


def public_callables():
    """'<module>.<function>' / '<module>.<class>.<method>' -> function, for the public callables of MODULES and of
    store.LatentStore (with the module's functions); __init__ counts as public."""
    import importlib
    import inspect
    out = {}
    for mn in MODULES + ("store",):
        m = importlib.import_module("vbq_amd." + mn)
        for n, o in sorted(vars(m).items()):
            if n.startswith("_") or getattr(o, "__module__", None) != m.__name__:
                continue
            if inspect.isfunction(o):
                out[f"{mn}.{n}"] = o
            elif inspect.isclass(o) and (mn != "store" or n == "LatentStore"):
                for k, v in sorted(vars(o).items()):
                    f = v.__func__ if isinstance(v, (staticmethod, classmethod)) else v
                    if (not k.startswith("_") or k == "__init__") and inspect.isfunction(f):
                        out[f"{mn}.{n}.{k}"] = f
    return out
