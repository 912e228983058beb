"""What the Python binding refuses, and with which exception: one defect at a time against a valid argument set, for every
`ops` function that validates through the shared helpers (_pair, _table, _per_lambda, _workspace, _out), plus the pieces
RansCodec's five methods and EntropyModelBuild's two length-table calls are assembled from.

Every refusal must come from Python: the library is replaced by a guard while a defective call runs, so a check that lets
a bad pointer or size through fails the test instead of reaching a kernel."""
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
ROWS, C, N, L = 8, 2, 4, 2
T = 2 ** (N + 1) - 1
LAMBDAS = [0.5, 2.0]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _empty(shape, dtype, device="cuda"):
    return torch.empty(shape, dtype=dtype, device=device)


def _strided(shape, dtype):
    """The right shape and dtype on the device, but every second element of a wider buffer."""
    return torch.empty(tuple(shape[:-1]) + (2 * shape[-1],), dtype=dtype, device="cuda")[..., ::2]


@pytest.fixture(scope="module")
def V():
    """The valid arguments every case starts from (never written to by a refused call)."""
    from scipy.stats import norm
    from vbq_amd import _lib, tables
    rng = np.random.default_rng(0)
    tab = np.ascontiguousarray(np.broadcast_to(norm.ppf(tables.dyadic_xi(N)), (C, T)), dtype=np.float32)
    h = _lib.lib()
    mu, sigma = _f32(rng.standard_normal((ROWS, C))), _f32(rng.uniform(0.1, 1.0, (ROWS, C)))
    return dict(mu=mu, sigma=sigma, mu_cb=mu.t().contiguous(), sigma_cb=sigma.t().contiguous(),
                table_lm=_f32(tab), table_sorted=_f32(tables.level_major_to_sorted(tab)),
                level_len=_f32(rng.uniform(1, 8, (L, C, N + 1))), models=_f32(rng.uniform(1, 12, (L, C, T))),
                idx=torch.from_numpy(rng.integers(0, T, (L, C, ROWS)).astype(np.uint16)).cuda(),
                codebook=torch.from_numpy(norm.ppf(tables.dyadic_xi(N))).cuda(),
                level_counts=torch.from_numpy(rng.integers(0, ROWS + 1, (L, C, N + 1))).cuda(),
                lut=_f32(-np.log2((np.arange(ROWS + 1) + 1.0) / (ROWS + T))),
                wsb=h.vbq_quantize_workspace_bytes(C, L, N), wsb_latents=h.vbq_compress_latents_workspace_bytes(ROWS, C, L, N))


def _solve(V):
    return dict(mu=V["mu"], sigma=V["sigma"], table_lm=V["table_lm"], lambdas=LAMBDAS, N=N, level_len=V["level_len"])


BASE = {
    "quantize": _solve,
    # the histogram-only solve takes channel-major planes [C, rows] (or channel-last through 'bc->cb'), never plain 'bc'
    "level_counts": lambda V: dict(_solve(V), mu=V["mu_cb"], sigma=V["sigma_cb"], layout="cb"),
    "compress_latents": lambda V: dict(means_bc=V["mu"], spread_bc=V["sigma"], table_lm=V["table_lm"], table_sorted=V["table_sorted"],
                                       lambdas=LAMBDAS, N=N, level_len=V["level_len"], models=V["models"]),
    "gather_latents": lambda V: dict(idx_planes=V["idx"], N=N, table_sorted=V["table_sorted"], level_len=V["level_len"],
                                     models=V["models"], want_num_bits=True),
    "histogram": lambda V: dict(idx=V["idx"], n_ch=C, N=N, layout="cb"),
    "histogram_models": lambda V: dict(idx=V["idx"], n_ch=C, counts=_empty((L, C, T), torch.int32), N=N, lut=V["lut"],
                                       models=_empty((L, C, T), torch.float32)),
    "prep_planes": lambda V: dict(means_bc=V["mu"], spread_bc=V["sigma"]),
    "transpose": lambda V: dict(x=V["mu"]),
    "transpose_planes": lambda V: dict(x=V["idx"]),
    "quantize_notebook": lambda V: dict(means=V["mu"], stds=V["sigma"], codebook_lm=V["codebook"], betas=LAMBDAS, N=N),
    "code_lengths_from_counts": lambda V: dict(counts=V["level_counts"], lut=V["lut"], level_period=N + 1, want_model=True),
}


def test_the_valid_set_runs_and_returns_the_documented_tensors(V):
    from vbq_amd import ops

    def is_(t, shape, dtype):
        return isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == shape and t.dtype == dtype

    call = lambda name, **more: getattr(ops, name)(**BASE[name](V), **more)
    assert is_(call("quantize"), (L, ROWS, C), torch.uint16)
    idx, zhat, bits = call("quantize", want_zhat=True, want_bits=True, workspace=_empty(V["wsb"], torch.uint8))
    assert is_(idx, (L, ROWS, C), torch.uint16) and is_(zhat, (L, ROWS, C), torch.float32) and is_(bits, (L, ROWS, C), torch.float32)
    given = _empty((L, ROWS, C), torch.uint16)
    assert call("quantize", out_idx=given) is given
    assert is_(call("level_counts"), (L, C, N + 1), torch.int64)
    given = torch.zeros((L, C, N + 1), dtype=torch.int64, device="cuda")
    assert call("level_counts", out=given, workspace=_empty(V["wsb"], torch.uint8)) is given
    assert int(given.sum()) == L * C * ROWS
    z, raw, nb = call("compress_latents", workspace=_empty(V["wsb_latents"], torch.uint8))
    assert is_(z, (L, ROWS, C), torch.float32) and is_(raw, (L, ROWS, C), torch.float32) and is_(nb, (L, ROWS, C), torch.float32)
    z, raw, nb, qi = call("gather_latents")
    assert is_(z, (L, ROWS, C), torch.float32) and is_(raw, (L, ROWS, C), torch.float32) and is_(nb, (L, ROWS, C), torch.float32)
    assert qi is None
    assert is_(call("histogram"), (L, C, T), torch.int64)
    given = torch.zeros((L, C, T), dtype=torch.int32, device="cuda")
    assert call("histogram", out=given) is given and int(given.sum()) == L * C * ROWS
    kw = BASE["histogram_models"](V)
    counts, models = ops.histogram_models(**kw)
    assert counts is kw["counts"] and models is kw["models"] and int(counts.sum()) == L * C * ROWS
    pm, ps = call("prep_planes")
    assert is_(pm, (C, ROWS), torch.float32) and is_(ps, (C, ROWS), torch.float32)
    given = _empty((C, ROWS), torch.float32)
    assert call("prep_planes", out_sigma=given)[1] is given
    assert is_(call("transpose"), (C, ROWS), torch.float32)
    assert call("transpose", out=given) is given and torch.equal(given, V["mu"].t())
    assert is_(call("transpose_planes"), (L, ROWS, C), torch.uint16)
    given = _empty((L, ROWS, C), torch.uint16)
    assert call("transpose_planes", out=given) is given
    idx, val = call("quantize_notebook")
    assert is_(idx, (L, ROWS, C), torch.uint16) and is_(val, (L, ROWS, C), torch.float32)
    idx, val = call("quantize_notebook", out_idx=given, want_values=False)
    assert idx is given and val is None
    ln, md = call("code_lengths_from_counts")
    assert is_(ln, (L, C, N + 1), torch.float32) and is_(md, (L, C, N + 1), torch.float32)


OUT_IDX = r"out_idx: expected a contiguous torch\.uint16 device tensor of shape \(2, 8, 2\)"
LC_OUT = r"out: expected a contiguous (torch\.)?int64 device tensor of shape \(2, 2, 5\)"
LEVEL_LEN = r"level_len shape \(2, 2, 4\) != \(2, 2, 5\)"
MODELS = r"models shape \(2, 2, 30\) != \(2, 2, 31\)"


def _out_msg(name, dtype, shape, before):
    """The one wording of the shared output check, in full -- or, word for word, what this function said before it shared it."""
    return "(%s|%s)" % (re.escape(f"{name}: expected a contiguous {dtype} device tensor of shape {shape}"), re.escape(before))


H_OUT = _out_msg("out", torch.int64, (L, C, T), "out shape (2, 2, 30) != (2, 2, 31)")
HM_BEFORE = "counts: expected a contiguous int32 / int64 device tensor of shape (2, 2, 31)"
HM_MODELS = _out_msg("models", torch.float32, (L, C, T), "models: expected a contiguous f32 device tensor of shape (2, 2, 31)")
PLANES = {n: _out_msg(n, torch.float32, (C, ROWS), n + " must be a contiguous f32 device tensor of shape (2, 8)") for n in ("out_mu", "out_sigma")}
TR_OUT = _out_msg("out", torch.float32, (C, ROWS), "out must be a contiguous f32 tensor of shape (2, 8)")
TP_OUT = _out_msg("out", torch.uint16, (L, ROWS, C), "out must be a contiguous torch.uint16 device tensor of shape (2, 8, 2)")
NB_OUT = _out_msg("out_idx", torch.uint16, (L, ROWS, C), "out_idx: expected a contiguous uint16 tensor of shape (2, 8, 2)")
V_ERR, X_ERR = "ValueError", "VBQError"


def _ws_short(key):
    return lambda V: _empty(V[key] - 1, torch.uint8)


def _ws_text(key):
    return lambda V: "workspace must be a device tensor of at least %d bytes" % V[key]


# (function, case, {argument: lambda V: defective value}, exception, pattern or lambda V: pattern)
CASES = []
for fn, mu_shape in (("quantize", r"\(8, 2\)"), ("level_counts", r"\(2, 8\)")):
    CASES += [
        (fn, "sigma_shape", {"sigma": lambda V: V["sigma"][:4]}, V_ERR, r"mu %s and sigma \(4, 2\) differ in shape" % mu_shape),
        (fn, "mu_dtype", {"mu": lambda V: V["mu"].double()}, V_ERR, r"mu: expected dtype torch\.float32"),
        (fn, "mu_not_a_tensor", {"mu": lambda V: V["mu"].cpu().numpy()}, V_ERR, "mu: expected a torch tensor"),
        (fn, "sigma_cpu", {"sigma": lambda V: V["sigma"].cpu()}, X_ERR, "sigma: tensor is on cpu"),
        (fn, "table_short", {"table_lm": lambda V: V["table_lm"].reshape(-1)[:-1]}, V_ERR, r"table_lm has 61 entries, expected C\*T = 2\*31"),
        (fn, "table_cpu", {"table_lm": lambda V: V["table_lm"].cpu()}, X_ERR, "table_lm: tensor is on cpu"),
        (fn, "no_lambdas", {"lambdas": lambda V: []}, V_ERR, "need at least one lambda"),
        (fn, "level_len_shape", {"level_len": lambda V: V["level_len"][:, :, :N]}, V_ERR, LEVEL_LEN),
        (fn, "level_len_dtype", {"level_len": lambda V: V["level_len"].double()}, V_ERR, r"level_len: expected dtype torch\.float32"),
        (fn, "workspace_short", {"workspace": _ws_short("wsb")}, V_ERR, _ws_text("wsb")),
        (fn, "workspace_cpu", {"workspace": lambda V: _empty(V["wsb"], torch.uint8, "cpu")}, V_ERR, _ws_text("wsb")),
    ]
CASES += [
    ("quantize", "out_idx_shape", {"out_idx": lambda V: _empty((L, ROWS, C + 1), torch.uint16)}, V_ERR, OUT_IDX),
    ("quantize", "out_idx_dtype", {"out_idx": lambda V: _empty((L, ROWS, C), torch.int16)}, V_ERR, OUT_IDX),
    ("quantize", "out_idx_strided", {"out_idx": lambda V: _strided((L, ROWS, C), torch.uint16)}, V_ERR, OUT_IDX),
    ("quantize", "out_idx_cpu", {"out_idx": lambda V: _empty((L, ROWS, C), torch.uint16, "cpu")}, V_ERR, OUT_IDX),
    ("quantize", "out_zhat_dtype", {"out_zhat": lambda V: _empty((L, ROWS, C), torch.float64)}, V_ERR,
     r"out_zhat: expected a contiguous torch\.float32 device tensor of shape \(2, 8, 2\)"),
    ("quantize", "out_bits_shape", {"out_bits": lambda V: _empty((L, C, ROWS), torch.float32)}, V_ERR,
     r"out_bits: expected a contiguous torch\.float32 device tensor of shape \(2, 8, 2\)"),
    ("level_counts", "out_shape", {"out": lambda V: _empty((L, C, N), torch.int64)}, V_ERR, LC_OUT),
    ("level_counts", "out_dtype", {"out": lambda V: _empty((L, C, N + 1), torch.int32)}, V_ERR, LC_OUT),
    ("level_counts", "out_strided", {"out": lambda V: _strided((L, C, N + 1), torch.int64)}, V_ERR, LC_OUT),
    ("level_counts", "out_cpu", {"out": lambda V: _empty((L, C, N + 1), torch.int64, "cpu")}, V_ERR, LC_OUT),

    ("compress_latents", "spread_shape", {"spread_bc": lambda V: V["sigma"][:4]}, V_ERR,
     r"expected two \[rows, C\] tensors, got \(8, 2\) / \(4, 2\)"),
    ("compress_latents", "means_1d", {"means_bc": lambda V: V["mu"].reshape(-1), "spread_bc": lambda V: V["sigma"].reshape(-1)}, V_ERR,
     r"expected two \[rows, C\] tensors, got \(16,\) / \(16,\)"),
    ("compress_latents", "means_dtype", {"means_bc": lambda V: V["mu"].double()}, V_ERR, r"means: expected dtype torch\.float32"),
    ("compress_latents", "spread_cpu", {"spread_bc": lambda V: V["sigma"].cpu()}, X_ERR, "spread: tensor is on cpu"),
    ("compress_latents", "no_lambdas", {"lambdas": lambda V: []}, V_ERR, "need at least one lambda"),
    ("compress_latents", "table_lm_short", {"table_lm": lambda V: V["table_lm"].reshape(-1)[:-1]}, V_ERR, r"tables must hold C\*T = 2\*31 entries"),
    ("compress_latents", "table_sorted_short", {"table_sorted": lambda V: V["table_sorted"].reshape(-1)[:-1]}, V_ERR,
     r"tables must hold C\*T = 2\*31 entries"),
    ("compress_latents", "table_sorted_cpu", {"table_sorted": lambda V: V["table_sorted"].cpu()}, X_ERR, "table_sorted: tensor is on cpu"),
    ("compress_latents", "level_len_shape", {"level_len": lambda V: V["level_len"][:, :, :N]}, V_ERR, LEVEL_LEN),
    ("compress_latents", "models_shape", {"models": lambda V: V["models"][:, :, :T - 1]}, V_ERR, MODELS),
    ("compress_latents", "models_cpu", {"models": lambda V: V["models"].cpu()}, X_ERR, "models: tensor is on cpu"),
    ("compress_latents", "workspace_short", {"workspace": _ws_short("wsb_latents")}, V_ERR, _ws_text("wsb_latents")),
    ("compress_latents", "workspace_cpu", {"workspace": lambda V: _empty(V["wsb_latents"], torch.uint8, "cpu")}, V_ERR, _ws_text("wsb_latents")),
    ("compress_latents", "spread_kind", {"spread": lambda V: "stddev"}, V_ERR, "spread must be one of"),

    ("gather_latents", "idx_2d", {"idx_planes": lambda V: V["idx"][0]}, V_ERR, r"idx_planes must be \[L, C, B\], got \(2, 8\)"),
    ("gather_latents", "idx_dtype", {"idx_planes": lambda V: V["idx"].view(torch.int16)}, V_ERR, r"idx_planes: expected dtype torch\.uint16"),
    ("gather_latents", "idx_cpu", {"idx_planes": lambda V: V["idx"].cpu()}, X_ERR, "idx_planes: tensor is on cpu"),
    ("gather_latents", "table_short", {"table_sorted": lambda V: V["table_sorted"].reshape(-1)[:-1]}, V_ERR,
     r"table_sorted has 61 entries, expected (C\*T = )?2\*31"),
    ("gather_latents", "table_missing", {"table_sorted": lambda V: None}, V_ERR, "table_sorted: expected a torch tensor"),
    ("gather_latents", "level_len_shape", {"level_len": lambda V: V["level_len"][:, :, :N]}, V_ERR, LEVEL_LEN),
    ("gather_latents", "models_shape", {"models": lambda V: V["models"][:, :, :T - 1]}, V_ERR, MODELS),
    ("gather_latents", "models_dtype", {"models": lambda V: V["models"].double()}, V_ERR, r"models: expected dtype torch\.float32"),

    ("histogram", "idx_dtype", {"idx": lambda V: V["idx"].view(torch.int16)}, V_ERR, r"idx: expected dtype torch\.uint16"),
    ("histogram", "idx_cpu", {"idx": lambda V: V["idx"].cpu()}, X_ERR, "idx: tensor is on cpu"),
    ("histogram", "channels", {"n_ch": lambda V: 3}, V_ERR, "16 indices per lambda is not a multiple of n_ch=3"),
    ("histogram", "out_dtype", {"out": lambda V: _empty((L, C, T), torch.float32)}, V_ERR, "out must be int64 or int32"),
    ("histogram", "out_shape", {"out": lambda V: _empty((L, C, T - 1), torch.int64)}, V_ERR, H_OUT),
    ("histogram", "out_strided", {"out": lambda V: _strided((L, C, T), torch.int32)}, V_ERR, r"out must be contiguous \(counts are accumulated in place\)"),
    ("histogram", "out_cpu", {"out": lambda V: _empty((L, C, T), torch.int64, "cpu")}, X_ERR, "out: tensor is on cpu"),

    ("histogram_models", "idx_channels", {"n_ch": lambda V: 1}, V_ERR, r"idx must be planes \[L, 1, rows\], got \(2, 2, 8\)"),
    ("histogram_models", "idx_cpu", {"idx": lambda V: V["idx"].cpu()}, X_ERR, "idx: tensor is on cpu"),
    ("histogram_models", "counts_shape", {"counts": lambda V: _empty((L, C, T - 1), torch.int32)}, V_ERR,
     _out_msg("counts", torch.int32, (L, C, T), HM_BEFORE)),
    ("histogram_models", "counts_dtype", {"counts": lambda V: _empty((L, C, T), torch.float32)}, V_ERR, re.escape(HM_BEFORE)),
    ("histogram_models", "counts_strided", {"counts": lambda V: _strided((L, C, T), torch.int64)}, V_ERR,
     _out_msg("counts", torch.int64, (L, C, T), HM_BEFORE)),
    ("histogram_models", "counts_cpu", {"counts": lambda V: _empty((L, C, T), torch.int32, "cpu")}, V_ERR,
     _out_msg("counts", torch.int32, (L, C, T), HM_BEFORE)),
    ("histogram_models", "lut_alone", {"models": lambda V: None}, V_ERR, "lut and models go together"),
    ("histogram_models", "models_alone", {"lut": lambda V: None}, V_ERR, "lut and models go together"),
    ("histogram_models", "lut_cpu", {"lut": lambda V: V["lut"].cpu()}, X_ERR, "lut: tensor is on cpu"),
    ("histogram_models", "models_shape", {"models": lambda V: _empty((L, C, T - 1), torch.float32)}, V_ERR, HM_MODELS),
    ("histogram_models", "models_dtype", {"models": lambda V: _empty((L, C, T), torch.float64)}, V_ERR, HM_MODELS),
    ("histogram_models", "models_strided", {"models": lambda V: _strided((L, C, T), torch.float32)}, V_ERR, HM_MODELS),
    ("histogram_models", "models_cpu", {"models": lambda V: _empty((L, C, T), torch.float32, "cpu")}, V_ERR, HM_MODELS),

    ("prep_planes", "spread_shape", {"spread_bc": lambda V: V["sigma"][:4]}, V_ERR, r"expected two \[rows, C\] tensors, got \(8, 2\) / \(4, 2\)"),
    ("prep_planes", "means_dtype", {"means_bc": lambda V: V["mu"].double()}, V_ERR, r"means: expected dtype torch\.float32"),
    ("prep_planes", "means_cpu", {"means_bc": lambda V: V["mu"].cpu()}, X_ERR, "means: tensor is on cpu"),
    ("prep_planes", "out_mu_shape", {"out_mu": lambda V: _empty((ROWS, C), torch.float32)}, V_ERR, PLANES["out_mu"]),
    ("prep_planes", "out_sigma_dtype", {"out_sigma": lambda V: _empty((C, ROWS), torch.float64)}, V_ERR, PLANES["out_sigma"]),
    ("prep_planes", "out_mu_strided", {"out_mu": lambda V: _strided((C, ROWS), torch.float32)}, V_ERR, PLANES["out_mu"]),
    ("prep_planes", "out_sigma_cpu", {"out_sigma": lambda V: _empty((C, ROWS), torch.float32, "cpu")}, V_ERR, PLANES["out_sigma"]),
    ("prep_planes", "spread_kind", {"spread": lambda V: "stddev"}, V_ERR, "spread must be one of"),

    ("transpose", "x_3d", {"x": lambda V: V["models"]}, V_ERR, "transpose expects a 2-D tensor"),
    ("transpose", "x_dtype", {"x": lambda V: V["mu"].double()}, V_ERR, r"x: expected dtype torch\.float32"),
    ("transpose", "x_cpu", {"x": lambda V: V["mu"].cpu()}, X_ERR, "x: tensor is on cpu"),
    ("transpose", "out_shape", {"out": lambda V: _empty((ROWS, C), torch.float32)}, V_ERR, TR_OUT),
    ("transpose", "out_dtype", {"out": lambda V: _empty((C, ROWS), torch.float64)}, V_ERR, TR_OUT),
    ("transpose", "out_strided", {"out": lambda V: _strided((C, ROWS), torch.float32)}, V_ERR, TR_OUT),

    ("transpose_planes", "x_2d", {"x": lambda V: V["idx"][0]}, V_ERR, "transpose_planes expects a 3-D tensor"),
    ("transpose_planes", "x_width", {"x": lambda V: V["models"].double()}, V_ERR, "2- or 4-byte elements"),
    ("transpose_planes", "x_cpu", {"x": lambda V: V["idx"].cpu()}, X_ERR, "transpose_planes: expected a tensor on a ROCm device"),
    ("transpose_planes", "out_shape", {"out": lambda V: _empty((L, C, ROWS), torch.uint16)}, V_ERR, TP_OUT),
    ("transpose_planes", "out_dtype", {"out": lambda V: _empty((L, ROWS, C), torch.int16)}, V_ERR, TP_OUT),
    ("transpose_planes", "out_strided", {"out": lambda V: _strided((L, ROWS, C), torch.uint16)}, V_ERR, TP_OUT),
    ("transpose_planes", "out_cpu", {"out": lambda V: _empty((L, ROWS, C), torch.uint16, "cpu")}, V_ERR, TP_OUT),

    ("quantize_notebook", "stds_shape", {"stds": lambda V: V["sigma"][:4]}, V_ERR, "means and stds differ in shape"),
    ("quantize_notebook", "means_dtype", {"means": lambda V: V["mu"].double()}, V_ERR, r"means: expected dtype torch\.float32"),
    ("quantize_notebook", "stds_cpu", {"stds": lambda V: V["sigma"].cpu()}, X_ERR, "stds: tensor is on cpu"),
    ("quantize_notebook", "codebook_short", {"codebook_lm": lambda V: V["codebook"][:-1]}, V_ERR, "codebook has 30 entries, expected 31"),
    ("quantize_notebook", "codebook_dtype", {"codebook_lm": lambda V: V["codebook"].float()}, V_ERR, r"codebook_lm: expected dtype torch\.float64"),
    ("quantize_notebook", "out_idx_shape", {"out_idx": lambda V: _empty((L, C, ROWS), torch.uint16)}, V_ERR, NB_OUT),
    ("quantize_notebook", "out_idx_dtype", {"out_idx": lambda V: _empty((L, ROWS, C), torch.int16)}, V_ERR, NB_OUT),
    ("quantize_notebook", "out_idx_strided", {"out_idx": lambda V: _strided((L, ROWS, C), torch.uint16)}, V_ERR, NB_OUT),

    ("code_lengths_from_counts", "counts_dtype", {"counts": lambda V: V["level_counts"].float()}, V_ERR, "counts must be int64 or int32"),
    ("code_lengths_from_counts", "counts_cpu", {"counts": lambda V: V["level_counts"].cpu()}, X_ERR, "counts: tensor is on cpu"),
    ("code_lengths_from_counts", "lut_dtype", {"lut": lambda V: V["lut"].double()}, V_ERR, r"lut: expected dtype torch\.float32"),
    ("code_lengths_from_counts", "lut_cpu", {"lut": lambda V: V["lut"].cpu()}, X_ERR, "lut: tensor is on cpu"),

    # The two output checks that did not look at the device before the validators were shared: a host tensor used to pass
    # them (its pointer went to the library).  These two cases, and no others in this file, are refused only since then.
    ("transpose", "out_cpu_tightened", {"out": lambda V: _empty((C, ROWS), torch.float32, "cpu")}, V_ERR, TR_OUT),
    ("quantize_notebook", "out_idx_cpu_tightened", {"out_idx": lambda V: _empty((L, ROWS, C), torch.uint16, "cpu")}, V_ERR, NB_OUT),
]


class _NoKernels:
    """Stands in for the library while a defective call runs: only the workspace-size queries answer."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name.endswith("_workspace_bytes"):
            return getattr(self._real, name)

        def reached(*args):
            raise AssertionError(f"{name} was reached with a defective argument")
        return reached


def _refused(monkeypatch, V, fn, defects, exc, pattern):
    from vbq_amd import _lib, ops
    kw = BASE[fn](V)
    kw.update({k: make(V) for k, make in defects.items()})
    real = _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: _NoKernels(real))
    with pytest.raises(ValueError if exc == V_ERR else _lib.VBQError, match=pattern(V) if callable(pattern) else pattern) as e:
        getattr(ops, fn)(**kw)
    assert type(e.value) is (ValueError if exc == V_ERR else _lib.VBQError)


@pytest.mark.parametrize("fn,defects,exc,pattern", [pytest.param(f, d, e, p, id=f"{f}-{c}") for f, c, d, e, p in CASES])
def test_one_defect_is_refused_before_the_library(monkeypatch, V, fn, defects, exc, pattern):
    _refused(monkeypatch, V, fn, defects, exc, pattern)


@pytest.mark.parametrize("arg", ["out_len", "out_model"])
@pytest.mark.parametrize("defect", ["shape", "dtype", "strided", "cpu"])
def test_code_lengths_checks_the_outputs_it_is_given(monkeypatch, V, arg, defect):
    """out_len= / out_model= (what pipeline.lengths and pipeline._models_from hand over) go through the shared output check."""
    shape = (L, C, N + 1)
    bad = {"shape": lambda V: _empty((L, C, N), torch.float32), "dtype": lambda V: _empty(shape, torch.float64),
           "strided": lambda V: _strided(shape, torch.float32), "cpu": lambda V: _empty(shape, torch.float32, "cpu")}[defect]
    _refused(monkeypatch, V, "code_lengths_from_counts", {arg: bad}, V_ERR,
             arg + r": expected a contiguous torch\.float32 device tensor of shape \(2, 2, 5\)")


def test_code_lengths_writes_into_the_outputs_it_is_given(V):
    from vbq_amd import ops
    ln, md = ops.code_lengths_from_counts(V["level_counts"], V["lut"], level_period=N + 1, want_model=True)
    out_len, out_model = _empty((L, C, N + 1), torch.float32), _empty((L, C, N + 1), torch.float32)
    got = ops.code_lengths_from_counts(V["level_counts"], V["lut"], level_period=N + 1, out_len=out_len, out_model=out_model)
    assert got[0] is out_len and got[1] is out_model and torch.equal(out_len, ln) and torch.equal(out_model, md)
    only = ops.code_lengths_from_counts(V["level_counts"], V["lut"], want_len=False, out_model=out_model)
    assert only is out_model and torch.equal(only, md)


# ------------------------------------------------------------------------------------------------------------ RansCodec
def _codec(S=2, n=70, seg=32):
    from vbq_amd.coder import RansCodec, quantize_frequencies
    rng = np.random.default_rng(70)
    idx = np.clip(np.rint(rng.normal(T // 2, 3.0, (S, n))), 0, T - 1).astype(np.uint16)
    freq = quantize_frequencies(np.stack([np.bincount(r, minlength=T) for r in idx]))
    return RansCodec(freq, N=N, segment=seg), idx


@pytest.mark.parametrize("method", ["encode", "sizes", "encode_packed"])
def test_codec_checks_the_stream_count(monkeypatch, method):
    from vbq_amd import _lib
    codec, _ = _codec()
    real = _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: _NoKernels(real))
    with pytest.raises(ValueError, match="3 index streams but 2 frequency rows"):
        getattr(codec, method)(torch.zeros((3, 70), dtype=torch.uint16, device="cuda"))
    with pytest.raises(_lib.VBQError, match="idx: tensor is on cpu"):
        getattr(codec, method)(torch.zeros((2, 70), dtype=torch.uint16))


def test_codec_padded_and_packed_forms_agree():
    codec, idx = _codec()
    d_idx = torch.from_numpy(idx).cuda()
    words, sizes = codec.encode(d_idx)
    assert tuple(words.shape) == (2, 3, 34) and words.dtype == torch.uint16
    assert tuple(sizes.shape) == (2, 3) and sizes.dtype == torch.uint32
    assert np.array_equal(codec.sizes(d_idx).cpu().numpy(), sizes.cpu().numpy())
    sz_h, pay_h = codec.encode_packed(d_idx)
    assert sz_h.dtype == np.uint32 and np.array_equal(sz_h, sizes.cpu().numpy())
    assert pay_h.dtype == np.uint16 and pay_h.tobytes() == codec.pack(words, sizes)
    back = codec.decode(words, sizes, 70)
    assert back.dtype == torch.uint16 and np.array_equal(back.cpu().numpy(), idx)
    back = codec.decode_packed(torch.from_numpy(pay_h).cuda(), torch.from_numpy(sz_h.astype(np.uint16).reshape(-1)).cuda(), 70)
    assert back.dtype == torch.uint16 and np.array_equal(back.cpu().numpy(), idx)


def test_codec_decode_names_what_is_wrong_with_a_stream():
    from vbq_amd import _lib
    codec, idx = _codec()
    words, sizes = codec.encode(torch.from_numpy(idx).cuda())
    big = sizes.cpu().numpy().copy()
    big[1, 2] = 35                                                        # more words than a segment of 32 symbols can hold
    with pytest.raises(_lib.VBQError, match=re.escape("rANS bitstream rejected: segment size out of range")):
        codec.decode(words, torch.from_numpy(big).cuda(), 70)


# --------------------------------------------------------------------------------------------------- EntropyModelBuild
@pytest.mark.parametrize("rows,n_chunks", [(2048, None), (4096, 2)])      # K2 writes the models itself / chunked: looked up afterwards
def test_build_tables_equal_the_code_length_op(V, rows, n_chunks):
    from vbq_amd import ops
    from vbq_amd.pipeline import EntropyModelBuild
    rng = np.random.default_rng(rows)
    mu_cb, sg_cb = _f32(rng.standard_normal((C, rows))), _f32(rng.uniform(0.05, 1.0, (C, rows)))
    build = EntropyModelBuild(rows, C, LAMBDAS, V["table_lm"], N=N, n_chunks=n_chunks).run(mu_cb, sg_cb)
    assert (build.side is not None) == (n_chunks == 2) and build.lut1 is not None and build.lut2 is not None
    build.check()
    ln, raw = ops.code_lengths_from_counts(build.level_counts, build.lut1, level_period=N + 1, want_model=True)
    assert torch.equal(build.level_len, ln) and torch.equal(build.raw_models, raw)
    assert torch.equal(build.models, ops.code_lengths_from_counts(build.counts, build.lut2, want_len=False, want_model=True))
    assert int(build.counts.sum()) == L * C * rows and build.models.dtype == torch.float32 and tuple(build.models.shape) == (L, C, T)
