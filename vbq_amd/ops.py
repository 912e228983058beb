"""Torch-tensor front end of the C-ABI (include/vbq.h).  PyTorch supplies device memory and
the current HIP stream; all arithmetic happens in libvbq_hip.so.  Every function raises
(VBQError / ValueError) instead of falling back to anything slower."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import LAYOUT_BC, LAYOUT_BC_TO_CB, LAYOUT_CB, MODE_F32, MODE_F64_SCORE, VBQError, check
from .tables import table_size

_LAYOUTS = {"bc": LAYOUT_BC, "cb": LAYOUT_CB, LAYOUT_BC: LAYOUT_BC, LAYOUT_CB: LAYOUT_CB}
_MODES = {"f32": MODE_F32, "f64": MODE_F64_SCORE, MODE_F32: MODE_F32, MODE_F64_SCORE: MODE_F64_SCORE}


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def raw_stream(device: torch.device) -> int:
    """Handle of the current HIP stream of `device` (an integer; 0 = the default stream) without building a torch.cuda.Stream
    object: torch.cuda.current_stream costs 4 us of Python per call, and every op asks once."""
    if _raw_stream is not None:
        return _raw_stream(device.index if device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(device).cuda_stream


def current_device(who: str) -> torch.device:
    """The current ROCm device; VBQError in the name of `who` (a module or class that computes nowhere else) without one."""
    if not torch.cuda.is_available():
        raise VBQError(f"no ROCm device visible: {who} has no CPU implementation")
    return torch.device("cuda", torch.cuda.current_device())


def host_tensor(a) -> torch.Tensor:
    """A NumPy array or sequence -> CPU tensor of the same values and dtype, whatever the array's layout: a C-contiguous
    writable array is shared, every other one (a slice, a transpose, a reversed or a read-only array -- torch.from_numpy refuses
    negative strides and warns about memory it may not write) is copied.  The tensor is only ever read."""
    a = np.asarray(a)
    if not (a.flags.c_contiguous and a.flags.writeable):
        a = np.array(a, order="C")
    return torch.from_numpy(a)


def upload(a, device, dtype) -> torch.Tensor:
    """A tensor, NumPy array or sequence -> contiguous tensor of `dtype` on `device`."""
    t = a.detach() if isinstance(a, torch.Tensor) else host_tensor(a)
    return t.to(device, dtype).contiguous()


def _stream(t: torch.Tensor):
    return C.c_void_p(raw_stream(t.device))


def _dev(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a torch tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise VBQError(f"{name}: tensor is on {t.device}; the VBQ kernels only run on a ROCm device "
                       "(there is no CPU implementation in this package)")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    return t.contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _doubles(vals: Sequence[float]):
    arr = (C.c_double * len(vals))(*[float(v) for v in vals])
    return arr


def _rows_channels(shape, layout):
    if len(shape) == 1:
        return shape[0], 1
    if len(shape) != 2:
        raise ValueError(f"expected a 1-D or 2-D tensor, got shape {tuple(shape)}")
    return (shape[0], shape[1]) if layout == LAYOUT_BC else (shape[1], shape[0])


# The argument checks the entry points share.  Each is the inline code it replaced: attribute reads and comparisons only.
def _pair(mu, sigma):
    mu = _dev(mu, torch.float32, "mu")
    sigma = _dev(sigma, torch.float32, "sigma")
    if mu.shape != sigma.shape:
        raise ValueError(f"mu {tuple(mu.shape)} and sigma {tuple(sigma.shape)} differ in shape")
    return mu, sigma


def _pair_bc(means_bc, spread_bc):
    means_bc = _dev(means_bc, torch.float32, "means")
    spread_bc = _dev(spread_bc, torch.float32, "spread")
    if means_bc.dim() != 2 or means_bc.shape != spread_bc.shape:
        raise ValueError(f"expected two [rows, C] tensors, got {tuple(means_bc.shape)} / {tuple(spread_bc.shape)}")
    return means_bc, spread_bc


def _table(t, Cc, T, name):
    t = _dev(t, torch.float32, name)
    if t.numel() != Cc * T:
        raise ValueError(f"{name} has {t.numel()} entries, expected C*T = {Cc}*{T}")
    return t


def _per_lambda(t, shape, name):
    """An f32 table with one slice per lambda (level_len [L, C, N+1], models [L, C, T]); otherwise e.g.
    "level_len shape (2, 2, 4) != (2, 2, 5)"."""
    t = _dev(t, torch.float32, name)
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} shape {tuple(t.shape)} != {shape}")
    return t


def _laid_out(t):
    """The strides of `t` are those a new tensor of its shape has: what a kernel that is handed one pointer assumes.  Read from
    the strides themselves, those of dimensions of size 1 included: is_contiguous() is true for every tensor of at most one
    element, whatever they are.  (Stricter than density: an [n, 1] view of a [1, n] tensor is refused.)"""
    want = 1
    for size, stride in zip(reversed(t.shape), reversed(t.stride())):
        if stride != want:
            return False
        want *= max(size, 1)
    return True


def _apart(name, t, others):
    """ValueError when the bytes of `t`, a tensor the call writes, intersect those of one of `others`: (name, tensor or None)
    pairs of what else the call reads or writes, each the tensor whose pointer goes to the library.  Half-open ranges from
    data_ptr() over numel() * element_size() bytes; an empty tensor intersects nothing."""
    n = t.numel() * t.element_size()
    if not n:
        return
    a = t.data_ptr()
    for other, o in others:
        if o is None:
            continue
        m, b = o.numel() * o.element_size(), o.data_ptr()
        if m and a < b + m and b < a + n:
            raise ValueError(f"{name} overlaps {other}: a tensor the call writes must share no memory with anything else it "
                             "reads or writes")


def _workspace(given, nbytes, device, floor=0, apart=()):
    """The caller's scratch, checked (a dense uint8 device tensor of at least `nbytes` bytes that touches nothing in `apart`),
    or a new one of max(nbytes, floor) bytes."""
    if given is None:
        return torch.empty(max(nbytes, floor), dtype=torch.uint8, device=device)
    if not isinstance(given, torch.Tensor) or given.numel() * given.element_size() < nbytes or not given.is_cuda \
            or given.device != device:
        raise ValueError(f"workspace must be a device tensor of at least {nbytes} bytes")
    if given.dtype != torch.uint8 or not _laid_out(given):
        raise ValueError(f"workspace: expected a contiguous {torch.uint8} device tensor of shape (>= {nbytes},)")
    _apart("workspace", given, apart)
    return given


def _out(given, shape, dtype, device, name, want=True, apart=()):
    """The caller's tensor for something the library writes, checked and never copied -- the object that comes back is the one
    that was given --, or a new one (None when not wanted).  A given tensor lies on `device` (None: on any ROCm device).  shape: the exact shape, or "any" where the call takes the element
    count from the tensor (such a tensor has to be given); dtype: the dtype, or a tuple of the ones the entry point takes;
    apart: see _apart."""
    if given is not None:
        ok = isinstance(given, torch.Tensor) and given.is_cuda and (device is None or given.device == device) and _laid_out(given)
        ok = ok and (given.dtype in dtype if isinstance(dtype, tuple) else given.dtype == dtype)
        if not (ok and (shape == "any" or tuple(given.shape) == shape)):
            raise ValueError(f"{name}: expected a contiguous {dtype} device tensor of shape {shape}")
        _apart(name, given, apart)
        return given
    return torch.empty(shape, dtype=dtype, device=device) if want else None


def _status(given, n, device, apart=()):
    """A caller's status words, uint32 [n], which the kernels OR their flags into: checked like any written tensor (an empty
    one has no address: the library would read it as "no status wanted")."""
    return _out(given, (n,), torch.uint32, device, "status", False, apart)


def _solve_inputs(mu, sigma, table_lm, lambdas, N, level_len, layout):
    """What K1 and K1t / K1h take alike -> (mu, sigma, rows, C, table_lm, L, level_len)."""
    mu, sigma = _pair(mu, sigma)
    rows, Cc = _rows_channels(mu.shape, layout)
    table_lm = _table(table_lm, Cc, table_size(N), "table_lm")
    L = len(lambdas)
    if L < 1:
        raise ValueError("need at least one lambda")
    if level_len is not None:
        level_len = _per_lambda(level_len, (L, Cc, N + 1), "level_len")
    return mu, sigma, rows, Cc, table_lm, L, level_len


def quantize(mu: torch.Tensor, sigma: torch.Tensor, table_lm: torch.Tensor, lambdas: Sequence[float], *,
             N: int = 10, level_len: Optional[torch.Tensor] = None, layout="bc", mode="f32",
             want_zhat: bool = False, want_bits: bool = False, out_idx: Optional[torch.Tensor] = None,
             out_zhat: Optional[torch.Tensor] = None, out_bits: Optional[torch.Tensor] = None,
             workspace: Optional[torch.Tensor] = None, rows: Optional[Sequence[int]] = None,
             workgroups_per_cu: int = 0, reserved_workgroups: Optional[int] = None):
    """K1 (vbq_quantize_f32).  mu, sigma: f32 [rows, C] (layout 'bc') / [C, rows] ('cb') / [n] (C = 1).
    table_lm: f32 [C, T] level-major.  level_len: optional f32 [L, C, N+1].
    Returns idx u16 [L, *mu.shape] and, when asked, zhat / bits f32 of the same shape.
    layout 'bc->cb': inputs channel-last [rows, C], outputs channel-major planes [L, C, rows] (no input transposes;
    f32 mode and lambdas in the fast kernel's range only, VBQError otherwise).
    rows=(r0, r1): only that row range is solved (vbq_quantize_rows_f32; the output tensors are still full-size) --
    the host cuts a pass into chunks to overlap K2 with K1; workgroups_per_cu, reserved_workgroups (slots this call's
    resident grid leaves to a kernel of another stream; None: 0): see include/vbq.h."""
    to_planes = layout in ("bc->cb", LAYOUT_BC_TO_CB)
    layout = LAYOUT_BC if to_planes else _LAYOUTS[layout]
    mode = _MODES[mode]
    rows_range = rows
    mu, sigma, rows, Cc, table_lm, L, level_len = _solve_inputs(mu, sigma, table_lm, lambdas, N, level_len, layout)
    h = _lib.lib()
    if to_planes and mu.dim() == 2 and Cc > 1:
        layout, oshape = LAYOUT_BC_TO_CB, (L, Cc, rows)
    else:
        oshape = (L,) + tuple(mu.shape)
    reads = (("mu", mu), ("sigma", sigma), ("table_lm", table_lm), ("level_len", level_len))
    idx = _out(out_idx, oshape, torch.uint16, mu.device, "out_idx", True, reads)
    zhat = _out(out_zhat, oshape, torch.float32, mu.device, "out_zhat", want_zhat, reads + (("out_idx", idx),))
    bits = _out(out_bits, oshape, torch.float32, mu.device, "out_bits", want_bits, reads + (("out_idx", idx), ("out_zhat", zhat)))
    want_zhat, want_bits = zhat is not None, bits is not None
    wsb = h.vbq_quantize_workspace_bytes(Cc, L, N)
    ws = _workspace(workspace, wsb, mu.device, 0, reads + (("out_idx", idx), ("out_zhat", zhat), ("out_bits", bits)))
    if mu.numel() == 0:
        out = (idx,) + ((zhat,) if want_zhat else ()) + ((bits,) if want_bits else ())
        return out if len(out) > 1 else idx
    if rows_range is None and not workgroups_per_cu and reserved_workgroups is None:
        check(h.vbq_quantize_f32(_ptr(mu), _ptr(sigma), rows, Cc, layout, _ptr(table_lm), _ptr(level_len),
                                 _doubles(lambdas), L, N, mode, _ptr(idx), _ptr(zhat), _ptr(bits), _ptr(ws), wsb,
                                 _stream(mu)), "vbq_quantize_f32")
    else:
        r0, r1 = (0, rows) if rows_range is None else (int(rows_range[0]), int(rows_range[1]))
        check(h.vbq_quantize_rows_f32(_ptr(mu), _ptr(sigma), rows, Cc, layout, _ptr(table_lm), _ptr(level_len),
                                      _doubles(lambdas), L, N, mode, _ptr(idx), _ptr(zhat), _ptr(bits), _ptr(ws), wsb,
                                      r0, r1, int(workgroups_per_cu), -1 if reserved_workgroups is None else int(reserved_workgroups),
                                      _stream(mu)), "vbq_quantize_rows_f32")
    out = (idx,)
    if want_zhat:
        out += (zhat,)
    if want_bits:
        out += (bits,)
    return out if len(out) > 1 else idx


def check_inputs(mu: torch.Tensor, sigma: torch.Tensor):
    """vbq_check_inputs_f32: raise ValueError when mu holds NaN / infinity or sigma holds NaN / infinity / values <= 0 --
    the inputs vbq_quantize_f32 does not define an answer for (synchronises: one 8-byte read)."""
    mu, sigma = _pair(mu, sigma)
    bad = torch.zeros(2, dtype=torch.uint32, device=mu.device)
    check(_lib.lib().vbq_check_inputs_f32(_ptr(mu), _ptr(sigma), mu.numel(), _ptr(bad), _stream(mu)), "vbq_check_inputs_f32")
    b = bad.cpu().numpy()
    if b[0] or b[1]:
        raise ValueError(f"invalid latents: {int(b[0])} non-finite means, {int(b[1])} standard deviations that are not finite and positive")


def level_counts(mu: torch.Tensor, sigma: torch.Tensor, table_lm: torch.Tensor, lambdas: Sequence[float], *,
                 N: int = 10, level_len: Optional[torch.Tensor] = None, layout="bc", out: Optional[torch.Tensor] = None,
                 workspace: Optional[torch.Tensor] = None, reserved_workgroups: Optional[int] = None):
    """K1t / K1h (vbq_level_counts_f32; thresholds for raw lengths at N = 10, dense otherwise): the solve of `quantize` followed by the per-(lambda, channel) histogram of the
    winners' bit levels, in one kernel with no per-element output.  Returns int64 [L, C, N+1] (added into `out`)."""
    to_planes = layout in ("bc->cb", LAYOUT_BC_TO_CB)
    layout = LAYOUT_BC if to_planes else _LAYOUTS[layout]
    mu, sigma, rows, Cc, table_lm, L, level_len = _solve_inputs(mu, sigma, table_lm, lambdas, N, level_len, layout)
    if to_planes and mu.dim() == 2 and Cc > 1:
        layout = LAYOUT_BC_TO_CB
    reads = (("mu", mu), ("sigma", sigma), ("table_lm", table_lm), ("level_len", level_len))
    if out is None:
        out = torch.zeros((L, Cc, N + 1), dtype=torch.int64, device=mu.device)
    else:
        out = _out(out, (L, Cc, N + 1), torch.int64, mu.device, "out", True, reads)
    h = _lib.lib()
    wsb = h.vbq_quantize_workspace_bytes(Cc, L, N)
    ws = _workspace(workspace, wsb, mu.device, 0, reads + (("out", out),))
    if mu.numel():
        check(h.vbq_level_counts_f32(_ptr(mu), _ptr(sigma), rows, Cc, layout, _ptr(table_lm), _ptr(level_len),
                                     _doubles(lambdas), L, N, _ptr(out), _ptr(ws), wsb,
                                     -1 if reserved_workgroups is None else int(reserved_workgroups), _stream(mu)),
              "vbq_level_counts_f32")
    return out


def code_lengths_from_counts(counts: torch.Tensor, lut: torch.Tensor, *, level_period: int = 0, want_len: bool = True,
                             want_model: bool = False, out_len: Optional[torch.Tensor] = None,
                             out_model: Optional[torch.Tensor] = None):
    """vbq_code_lengths_from_counts: f32 tensors shaped like `counts` -- (level +) lut[count] and / or lut[count].
    out_len / out_model: the caller's tensors, written instead of new ones (giving one asks for that result)."""
    if counts.dtype not in (torch.int64, torch.int32):
        raise ValueError("counts must be int64 or int32")
    counts = _dev(counts, counts.dtype, "counts")
    lut = _dev(lut, torch.float32, "lut")
    reads = (("counts", counts), ("lut", lut))
    out_len = _out(out_len, tuple(counts.shape), torch.float32, counts.device, "out_len", want_len, reads)
    out_model = _out(out_model, tuple(counts.shape), torch.float32, counts.device, "out_model", want_model,
                     reads + (("out_len", out_len),))
    check(_lib.lib().vbq_code_lengths_from_counts(_ptr(counts), int(counts.dtype == torch.int32), counts.numel(), _ptr(lut),
                                                  lut.numel(), int(level_period), _ptr(out_len), _ptr(out_model),
                                                  _stream(counts)), "vbq_code_lengths_from_counts")
    if out_len is not None and out_model is not None:
        return out_len, out_model
    return out_len if out_len is not None else out_model


def quantize_notebook(means: torch.Tensor, stds: torch.Tensor, codebook_lm: torch.Tensor, betas: Sequence[float], *,
                      N: int = 10, want_values: bool = True, out_idx: Optional[torch.Tensor] = None):
    """K1n (vbq_quantize_notebook_f64).  Returns (idx u16 [n_beta, *shape], values f32 or None)."""
    means = _dev(means, torch.float32, "means")
    stds = _dev(stds, torch.float32, "stds")
    if means.shape != stds.shape:
        raise ValueError("means and stds differ in shape")
    codebook_lm = _dev(codebook_lm, torch.float64, "codebook_lm")
    if codebook_lm.numel() != table_size(N):
        raise ValueError(f"codebook has {codebook_lm.numel()} entries, expected {table_size(N)}")
    nb = len(betas)
    n = means.numel()
    idx = _out(out_idx, (nb,) + tuple(means.shape), torch.uint16, means.device, "out_idx", True,
               (("means", means), ("stds", stds), ("codebook_lm", codebook_lm)))
    val = torch.empty((nb,) + tuple(means.shape), dtype=torch.float32, device=means.device) if want_values else None
    check(_lib.lib().vbq_quantize_notebook_f64(_ptr(means), _ptr(stds), n, _ptr(codebook_lm), _doubles(betas), nb, N,
                                               _ptr(idx), _ptr(val), _stream(means)), "vbq_quantize_notebook_f64")
    return idx, val


def histogram(idx: torch.Tensor, n_ch: int, *, N: int = 10, layout="bc", out: Optional[torch.Tensor] = None,
              dtype=torch.int64, rows: Optional[Sequence[int]] = None):
    """K2 (vbq_histogram_u16 / _i32).  idx: u16 [L, rows, C] / [L, C, rows] / [L, n].  Returns counts
    [L, C, T] (added into `out` when given; `out.dtype` int64 or int32 selects the entry point)."""
    layout = _LAYOUTS[layout]
    rows_range = rows
    idx = _dev(idx, torch.uint16, "idx")
    L = idx.shape[0]
    E = idx[0].numel()
    if E % n_ch:
        raise ValueError(f"{E} indices per lambda is not a multiple of n_ch={n_ch}")
    rows = E // n_ch
    T = table_size(N)
    if out is None:
        out = torch.zeros((L, n_ch, T), dtype=dtype, device=idx.device)
    else:
        if out.dtype not in (torch.int64, torch.int32):
            raise ValueError("out must be int64 or int32")
        if not out.is_contiguous():
            raise ValueError("out must be contiguous (counts are accumulated in place)")
        _dev(out, out.dtype, "out")                                       # (the refusals of a host tensor, in their words)
        out = _out(out, (L, n_ch, T), out.dtype, idx.device, "out", True, (("idx", idx),))
    h = _lib.lib()
    if rows_range is not None:
        check(h.vbq_histogram_rows_u16(_ptr(idx), rows, n_ch, layout, L, N, _ptr(out), int(out.dtype == torch.int32),
                                       int(rows_range[0]), int(rows_range[1]), _stream(idx)), "vbq_histogram_rows_u16")
        return out
    fn, name = (h.vbq_histogram_u16, "vbq_histogram_u16") if out.dtype == torch.int64 else \
               (h.vbq_histogram_u16_i32, "vbq_histogram_u16_i32")
    check(fn(_ptr(idx), rows, n_ch, layout, L, N, _ptr(out), _stream(idx)), name)
    return out


def histogram_models(idx: torch.Tensor, n_ch: int, counts: torch.Tensor, *, N: int = 10, lut: Optional[torch.Tensor] = None,
                     models: Optional[torch.Tensor] = None):
    """vbq_histogram_models_u16: counts[L, C, T] := histogram of the planes idx [L, C, rows] (assigned, not added) and, with
    `lut` / `models` (f32 [L, C, T]), models := lut[counts] in the same pass.  Returns (counts, models)."""
    idx = _dev(idx, torch.uint16, "idx")
    if idx.dim() != 3 or idx.shape[1] != n_ch:
        raise ValueError(f"idx must be planes [L, {n_ch}, rows], got {tuple(idx.shape)}")
    L, _, rows = idx.shape
    T = table_size(N)
    if counts.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"counts: expected a contiguous int32 / int64 device tensor of shape {(L, n_ch, T)}")
    counts = _out(counts, (L, n_ch, T), counts.dtype, idx.device, "counts", True, (("idx", idx),))
    if (lut is None) != (models is None):
        raise ValueError("lut and models go together")
    if models is not None:
        lut = _dev(lut, torch.float32, "lut")
        _apart("counts", counts, (("lut", lut),))
        models = _out(models, (L, n_ch, T), torch.float32, idx.device, "models", True,
                      (("idx", idx), ("lut", lut), ("counts", counts)))
    check(_lib.lib().vbq_histogram_models_u16(_ptr(idx), rows, n_ch, L, N, _ptr(counts), int(counts.dtype == torch.int32), _ptr(lut),
                                              lut.numel() if lut is not None else 0, _ptr(models), _stream(idx)),
          "vbq_histogram_models_u16")
    return counts, models


def index_max(idx: torch.Tensor) -> int:
    """vbq_index_max_u16: the largest index of a u16 array (synchronises).  For indices of foreign origin: K2 and
    gather are memory-safe for anything, but only indices < T are meaningful."""
    idx = _dev(idx, torch.uint16, "idx")
    m = torch.zeros(1, dtype=torch.uint32, device=idx.device)
    check(_lib.lib().vbq_index_max_u16(_ptr(idx), idx.numel(), _ptr(m), _stream(idx)), "vbq_index_max_u16")
    return int(m.cpu().item())


def moments(x: torch.Tensor, *, layout="bc", out: Optional[torch.Tensor] = None):
    """K3 (vbq_moments_f32).  Returns f64 [C, 2] = (sum x, sum x^2) per channel."""
    layout = _LAYOUTS[layout]
    x = _dev(x, torch.float32, "x")
    rows, Cc = _rows_channels(x.shape, layout)
    if out is None:
        out = torch.zeros((Cc, 2), dtype=torch.float64, device=x.device)
    else:
        out = _out(out, (Cc, 2), torch.float64, x.device, "out", True, (("x", x),))
    check(_lib.lib().vbq_moments_f32(_ptr(x), rows, Cc, layout, _ptr(out), _stream(x)), "vbq_moments_f32")
    return out


def numpy_sum_sq(x: torch.Tensor) -> torch.Tensor:
    """vbq_numpy_sum_sq_f32: np.sum(x.ravel()**2) of a float32 tensor in NumPy's own summation order -> f32 [1] (device)."""
    x = _dev(x, torch.float32, "x").reshape(-1)
    if x.data_ptr() % 16:                       # a view into a larger tensor: the block kernel loads 16 bytes per lane
        x = x.clone()
    out = torch.zeros(1, dtype=torch.float32, device=x.device)
    h = _lib.lib()
    wsb = h.vbq_numpy_sum_sq_workspace_bytes(x.numel())
    ws = torch.empty(max(wsb, 4), dtype=torch.uint8, device=x.device)
    check(h.vbq_numpy_sum_sq_f32(_ptr(x), x.numel(), _ptr(out), _ptr(ws), wsb, _stream(x)), "vbq_numpy_sum_sq_f32")
    return out


def unit_to_u8(x: torch.Tensor) -> torch.Tensor:
    """vbq_unit_to_u8_f32: np.clip(np.round(x * 255), 0, 255).astype(np.uint8) of a float32 device tensor (utils.py:555)."""
    x = _dev(x, torch.float32, "x")
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(_lib.lib().vbq_unit_to_u8_f32(_ptr(x), x.numel(), _ptr(out), _stream(x)), "vbq_unit_to_u8_f32")
    return out


def numpy_row_sums(x: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vbq_numpy_row_sums_f32: np.sum(x[r]) for every r of a contiguous float32 device tensor [rows, ...], in NumPy's own float32
    summation order (bit for bit) -> f32 [rows] on the device.  The reductions of the evaluation loop (utils.py:547-552) without
    bringing the per-lambda arrays to the host."""
    x = _dev(x, torch.float32, "x")
    rows = x.shape[0]
    n = x[0].numel() if rows else 0
    out = torch.empty(rows, dtype=torch.float32, device=x.device)
    h = _lib.lib()
    wsb = h.vbq_numpy_row_sums_workspace_bytes(rows, n)
    ws = _workspace(workspace, wsb, x.device, 4, (("x", x),))
    check(h.vbq_numpy_row_sums_f32(_ptr(x), rows, n, _ptr(out), _ptr(ws), wsb, _stream(x)), "vbq_numpy_row_sums_f32")
    return out


def gather(idx: torch.Tensor, tab: torch.Tensor, n_ch: int, *, N: int = 10, layout="bc", out_layout=None):
    """vbq_gather_f32: out[l][e] = tab[(l,) c(e), idx[l][e]].  tab: f32 [C, T] or [L, C, T] indexed by RANK.
    With out_layout != layout the result comes back transposed (e.g. idx [L, C, B] -> out [L, B, C])."""
    layout = _LAYOUTS[layout]
    out_layout = layout if out_layout is None else _LAYOUTS[out_layout]
    idx = _dev(idx, torch.uint16, "idx")
    tab = _dev(tab, torch.float32, "tab")
    L = idx.shape[0]
    E = idx[0].numel()
    rows = E // n_ch
    T = table_size(N)
    per_lambda = tab.dim() == 3
    if tuple(tab.shape) != ((L, n_ch, T) if per_lambda else (n_ch, T)):
        raise ValueError(f"tab shape {tuple(tab.shape)} does not match (L={L}, C={n_ch}, T={T})")
    oshape = tuple(idx.shape)
    if out_layout != layout and idx.dim() == 3 and n_ch == 1:
        oshape = (L, idx.shape[2], idx.shape[1])          # same memory, other view
    if out_layout != layout and n_ch > 1:
        if idx.dim() != 3:
            raise ValueError("a layout change needs idx of shape [L, rows, C] or [L, C, rows]")
        oshape = (L, idx.shape[2], idx.shape[1])
    out = torch.empty(oshape, dtype=torch.float32, device=idx.device)
    check(_lib.lib().vbq_gather_f32(_ptr(idx), rows, n_ch, layout, L, N, _ptr(tab), int(per_lambda), _ptr(out),
                                    out_layout, _stream(idx)), "vbq_gather_f32")
    return out


_SPREADS = {"sigma": 0, "variance": 1, "logvar": 2}


def _spread_kind(spread: str) -> int:
    try:
        return _SPREADS[spread]
    except KeyError:
        raise ValueError(f"spread must be one of {sorted(_SPREADS)}, got {spread!r}") from None


def prep_planes(means_bc: torch.Tensor, spread_bc: torch.Tensor, *, spread: str = "sigma",
                out_mu: Optional[torch.Tensor] = None, out_sigma: Optional[torch.Tensor] = None):
    """vbq_prep_planes_f32: channel-last [rows, C] means and spreads -> channel-major planes [C, rows] in ONE launch.
    spread: what `spread_bc` holds -- 'sigma', 'variance' (sigma = sqrt(.)) or 'logvar' (sigma = sqrt(exp(.)), the
    `tf.exp(posterior_logvars) ** 0.5` of quantizer.py:197,202 inside the launch)."""
    means_bc, spread_bc = _pair_bc(means_bc, spread_bc)
    r, c = means_bc.shape
    reads = (("means", means_bc), ("spread", spread_bc))
    out_mu = _out(out_mu, (c, r), torch.float32, means_bc.device, "out_mu", True, reads)
    out_sigma = _out(out_sigma, (c, r), torch.float32, means_bc.device, "out_sigma", True, reads + (("out_mu", out_mu),))
    check(_lib.lib().vbq_prep_planes_f32(_ptr(means_bc), _ptr(spread_bc), _spread_kind(spread), r, c, _ptr(out_mu),
                                         _ptr(out_sigma), _stream(means_bc)), "vbq_prep_planes_f32")
    return out_mu, out_sigma


def gather_latents(idx_planes: torch.Tensor, *, N: int = 10, table_sorted: Optional[torch.Tensor] = None,
                   level_len: Optional[torch.Tensor] = None, models: Optional[torch.Tensor] = None, want_zhat: bool = True,
                   want_raw_bits: bool = True, want_num_bits: bool = False, want_idx: bool = False):
    """vbq_gather_latents_u16: ONE pass over rank indices in planes [L, C, B] -> channel-last [L, B, C] results
    (Z_hat f32, raw_num_bits int32 / f32 with level_len, num_bits f32, idx u16; None for the ones not asked for)."""
    idx_planes = _dev(idx_planes, torch.uint16, "idx_planes")
    if idx_planes.dim() != 3:
        raise ValueError(f"idx_planes must be [L, C, B], got {tuple(idx_planes.shape)}")
    L, Cc, B = idx_planes.shape
    T = table_size(N)
    if want_zhat:
        table_sorted = _table(table_sorted, Cc, T, "table_sorted")
    if level_len is not None:
        level_len = _per_lambda(level_len, (L, Cc, N + 1), "level_len")
    if want_num_bits:
        models = _per_lambda(models, (L, Cc, T), "models")
    dev = idx_planes.device
    z = torch.empty((L, B, Cc), dtype=torch.float32, device=dev) if want_zhat else None
    raw = torch.empty((L, B, Cc), dtype=torch.int32 if level_len is None else torch.float32, device=dev) if want_raw_bits else None
    nb = torch.empty((L, B, Cc), dtype=torch.float32, device=dev) if want_num_bits else None
    qi = torch.empty((L, B, Cc), dtype=torch.uint16, device=dev) if want_idx else None
    check(_lib.lib().vbq_gather_latents_u16(_ptr(idx_planes), B, Cc, L, N, _ptr(table_sorted) if want_zhat else None, _ptr(level_len),
                                            _ptr(models) if want_num_bits else None, _ptr(z), _ptr(raw), _ptr(nb), _ptr(qi),
                                            _stream(idx_planes)), "vbq_gather_latents_u16")
    return z, raw, nb, qi


def compress_latents(means_bc: torch.Tensor, spread_bc: torch.Tensor, table_lm: torch.Tensor, table_sorted: torch.Tensor,
                     lambdas: Sequence[float], *, N: int = 10, spread: str = "sigma",
                     level_len: Optional[torch.Tensor] = None, models: Optional[torch.Tensor] = None,
                     workspace: Optional[torch.Tensor] = None):
    """vbq_compress_latents_f32: the per-image call of quantizer.py:190-240 in one C call (planes, solve, fused lookups).
    means / spreads channel-last [B, C] (spread: 'sigma' | 'variance' | 'logvar', see prep_planes); returns
    (Z_hat f32, raw_num_bits int32 | f32, num_bits f32 | None), [L, B, C]."""
    means_bc, spread_bc = _pair_bc(means_bc, spread_bc)
    B, Cc = means_bc.shape
    L = len(lambdas)
    T = table_size(N)
    if L < 1:
        raise ValueError("need at least one lambda")
    table_lm = _dev(table_lm, torch.float32, "table_lm")
    table_sorted = _dev(table_sorted, torch.float32, "table_sorted")
    if table_lm.numel() != Cc * T or table_sorted.numel() != Cc * T:
        raise ValueError(f"tables must hold C*T = {Cc}*{T} entries")
    if level_len is not None:
        level_len = _per_lambda(level_len, (L, Cc, N + 1), "level_len")
    if models is not None:
        models = _per_lambda(models, (L, Cc, T), "models")
    dev = means_bc.device
    h = _lib.lib()
    wsb = h.vbq_compress_latents_workspace_bytes(B, Cc, L, N)
    ws = _workspace(workspace, wsb, dev, 256, (("means", means_bc), ("spread", spread_bc), ("table_lm", table_lm),
                                               ("table_sorted", table_sorted), ("level_len", level_len), ("models", models)))
    z = torch.empty((L, B, Cc), dtype=torch.float32, device=dev)
    raw = torch.empty((L, B, Cc), dtype=torch.int32 if level_len is None else torch.float32, device=dev)
    nb = torch.empty((L, B, Cc), dtype=torch.float32, device=dev) if models is not None else None
    if B:
        check(h.vbq_compress_latents_f32(_ptr(means_bc), _ptr(spread_bc), _spread_kind(spread), B, Cc, _ptr(table_lm),
                                         _ptr(table_sorted), _ptr(level_len), _ptr(models), _doubles(lambdas), L, N, _ptr(z),
                                         _ptr(raw), _ptr(nb), _ptr(ws), ws.numel() * ws.element_size(), _stream(means_bc)),
              "vbq_compress_latents_f32")
    return z, raw, nb


def transpose(x: torch.Tensor, out: Optional[torch.Tensor] = None):
    """vbq_transpose_f32: [rows, cols] f32 -> [cols, rows] (channel-last <-> channel-major planes)."""
    x = _dev(x, torch.float32, "x")
    if x.dim() != 2:
        raise ValueError("transpose expects a 2-D tensor")
    r, c = x.shape
    out = _out(out, (c, r), torch.float32, x.device, "out", True, (("x", x),))
    check(_lib.lib().vbq_transpose_f32(_ptr(x), r, c, _ptr(out), _stream(x)), "vbq_transpose_f32")
    return out


def rd_sums(mu: torch.Tensor, sigma: torch.Tensor, idx: torch.Tensor, tab_sorted: torch.Tensor, n_ch: int, *, N: int = 10,
            layout="bc", rate: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """vbq_rd_sums_u16: f64 [L, 2] = per lambda (sum of (z - mu)^2 / (2 sigma^2), sum of rate[idx]) over all elements, z looked
    up in the SORTED table by rank index.  rate: f32 [C, T] or [L, C, T] (entropy models), or None."""
    layout = _LAYOUTS[layout]
    mu = _dev(mu, torch.float32, "mu")
    sigma = _dev(sigma, torch.float32, "sigma")
    idx = _dev(idx, torch.uint16, "idx")
    tab_sorted = _dev(tab_sorted, torch.float32, "tab_sorted")
    L = idx.shape[0]
    E = mu.numel()
    T = table_size(N)
    if idx[0].numel() != E or sigma.numel() != E or E % n_ch:
        raise ValueError("mu, sigma and idx[l] must hold the same number of elements, a multiple of n_ch")
    if tab_sorted.numel() != n_ch * T:
        raise ValueError(f"tab_sorted has {tab_sorted.numel()} entries, expected {n_ch}*{T}")
    per_lambda = 0
    if rate is not None:
        rate = _dev(rate, torch.float32, "rate")
        per_lambda = int(rate.dim() == 3)
        if tuple(rate.shape) != ((L, n_ch, T) if per_lambda else (n_ch, T)):
            raise ValueError(f"rate shape {tuple(rate.shape)} does not match (L={L}, C={n_ch}, T={T})")
    if out is None:
        out = torch.zeros((L, 2), dtype=torch.float64, device=mu.device)
    else:
        out = _out(out, (L, 2), torch.float64, mu.device, "out", True,
                   (("mu", mu), ("sigma", sigma), ("idx", idx), ("tab_sorted", tab_sorted), ("rate", rate)))
    check(_lib.lib().vbq_rd_sums_u16(_ptr(mu), _ptr(sigma), _ptr(idx), E // n_ch, n_ch, layout, L, N, _ptr(tab_sorted), _ptr(rate),
                                     per_lambda, _ptr(out), _stream(mu)), "vbq_rd_sums_u16")
    return out


def transpose_planes(x: torch.Tensor, out: Optional[torch.Tensor] = None):
    """vbq_transpose_planes: [batch, rows, cols] -> [batch, cols, rows] for uint16 / float32 / int32 stacks (e.g. plane
    indices [L, C, B] -> channel-last [L, B, C])."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise VBQError("transpose_planes: expected a tensor on a ROCm device")
    if x.dim() != 3 or x.element_size() not in (2, 4):
        raise ValueError("transpose_planes expects a 3-D tensor of 2- or 4-byte elements")
    x = x.contiguous()
    b, r, c = x.shape
    out = _out(out, (b, c, r), x.dtype, x.device, "out", True, (("x", x),))
    check(_lib.lib().vbq_transpose_planes(_ptr(x), b, r, c, x.element_size(), _ptr(out), _stream(x)), "vbq_transpose_planes")
    return out


def argmax_candidates(P: torch.Tensor, lens: torch.Tensor, mu: torch.Tensor, sigma: torch.Tensor,
                      lambdas: Sequence[float], *, mode="f32", want_j=False):
    """K1c (vbq_argmax_candidates_f32).  P: f32 [M, *shape]; lens: f32 [M, *shape] or [L, M, *shape]."""
    mode = _MODES[mode]
    P = _dev(P, torch.float32, "P")
    lens = _dev(lens, torch.float32, "lens")
    mu = _dev(mu, torch.float32, "mu")
    sigma = _dev(sigma, torch.float32, "sigma")
    M = P.shape[0]
    L = len(lambdas)
    if tuple(P.shape[1:]) != tuple(mu.shape) or mu.shape != sigma.shape:
        raise ValueError("P must be [M, *mu.shape] and sigma must match mu")
    per_lambda = lens.dim() == P.dim() + 1
    if tuple(lens.shape) != (((L,) if per_lambda else ()) + tuple(P.shape)):
        raise ValueError(f"lens shape {tuple(lens.shape)} incompatible with P {tuple(P.shape)} and L={L}")
    n = mu.numel()
    zhat = torch.empty((L,) + tuple(mu.shape), dtype=torch.float32, device=mu.device)
    bits = torch.empty_like(zhat)
    j = torch.empty((L,) + tuple(mu.shape), dtype=torch.int32, device=mu.device) if want_j else None
    check(_lib.lib().vbq_argmax_candidates_f32(_ptr(P), _ptr(lens), int(per_lambda), _ptr(mu), _ptr(sigma), n,
                                               _doubles(lambdas), L, M, mode, _ptr(j), _ptr(zhat), _ptr(bits),
                                               _stream(mu)), "vbq_argmax_candidates_f32")
    return (zhat, bits, j) if want_j else (zhat, bits)


def bmshj_cdf_pdf(params: torch.Tensor, x: torch.Tensor, *, cdf=True, pdf=True, logpdf=False):
    """K4 (vbq_bmshj_cdf_pdf_f32).  params: f32 [C, 43] effective parameters; x: f32 [..., C]."""
    params = _dev(params, torch.float32, "params")
    x = _dev(x, torch.float32, "x")
    Cc = params.shape[0]
    if params.shape[1] != _lib.BMSHJ_PARAMS_PER_CHANNEL or x.shape[-1] != Cc:
        raise ValueError(f"params must be [C, 43] and x [..., C]; got {tuple(params.shape)}, {tuple(x.shape)}")
    rows = x.numel() // Cc
    outs = [torch.empty_like(x) if f else None for f in (cdf, pdf, logpdf)]
    check(_lib.lib().vbq_bmshj_cdf_pdf_f32(_ptr(params), _ptr(x), rows, Cc, _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
                                           _stream(x)), "vbq_bmshj_cdf_pdf_f32")
    return tuple(outs)


def _icdf_args(params, xi, left, right, mid, flags, flags_shape):
    """What the two bisection calls check alike: params f32 [C, 43], xi f32 [..., C], the brackets and mid points f32 like xi --
    state the kernels update where it lies -- and flags u32 (or i32) of `flags_shape`."""
    params = _dev(params, torch.float32, "params")
    xi = _dev(xi, torch.float32, "xi")
    if params.dim() != 2 or params.shape[1] != _lib.BMSHJ_PARAMS_PER_CHANNEL or xi.dim() < 1 or xi.shape[-1] != params.shape[0]:
        raise ValueError(f"params must be [C, 43] and xi [..., C]; got {tuple(params.shape)}, {tuple(xi.shape)}")
    reads = (("params", params), ("xi", xi))
    left = _out(left, tuple(xi.shape), torch.float32, xi.device, "left", False, reads)
    right = _out(right, tuple(xi.shape), torch.float32, xi.device, "right", False, reads + (("left", left),))
    mid = _out(mid, tuple(xi.shape), torch.float32, xi.device, "mid", False, reads + (("left", left), ("right", right)))
    flags = _out(flags, flags_shape, (torch.uint32, torch.int32), xi.device, "flags", False,
                 reads + (("left", left), ("right", right), ("mid", mid)))
    if left is None or right is None or mid is None or flags is None:
        raise ValueError("left, right, mid and flags are the caller's tensors: none may be None")
    return params, xi, left, right, mid, flags


def bmshj_icdf_step(params, xi, left, right, mid, flags):
    """K4 (vbq_bmshj_icdf_step_f32): one in-place bisection update; flags u32[2] must be preset to (0, 0x7f800000)."""
    params, xi, left, right, mid, flags = _icdf_args(params, xi, left, right, mid, flags, (2,))
    Cc = params.shape[0]
    rows = xi.numel() // Cc
    check(_lib.lib().vbq_bmshj_icdf_step_f32(_ptr(params), _ptr(xi), rows, Cc, _ptr(left), _ptr(right), _ptr(mid),
                                             _ptr(flags), _stream(xi)), "vbq_bmshj_icdf_step_f32")


def bmshj_icdf_chain(params, xi, left, right, mid, flags, n_steps: int, tol: float, first: bool = True):
    """K4 (vbq_bmshj_icdf_chain_f32): n_steps bisection updates enqueued at once, the reference's stopping rule applied on the
    device between them; flags u32 [n_steps + 1, 2] is written (read it after a synchronisation)."""
    params, xi, left, right, mid, flags = _icdf_args(params, xi, left, right, mid, flags, (int(n_steps) + 1, 2))
    Cc = params.shape[0]
    rows = xi.numel() // Cc
    check(_lib.lib().vbq_bmshj_icdf_chain_f32(_ptr(params), _ptr(xi), rows, Cc, _ptr(left), _ptr(right), _ptr(mid), _ptr(flags),
                                              int(n_steps), float(tol), int(bool(first)), _stream(xi)), "vbq_bmshj_icdf_chain_f32")


def bmshj_nll_grad(params: torch.Tensor, x_cb: torch.Tensor, out: Optional[torch.Tensor] = None):
    """K4 (vbq_bmshj_nll_grad_f32).  params f32 [C, 43] effective; x_cb f32 [C, n] planes.
    Returns f64 [C, 44]: d(sum -log(pdf+1e-10))/d(params) and, in column 43, the sum itself."""
    params = _dev(params, torch.float32, "params")
    x_cb = _dev(x_cb, torch.float32, "x_cb")
    Cc, n = x_cb.shape
    if tuple(params.shape) != (Cc, _lib.BMSHJ_PARAMS_PER_CHANNEL):
        raise ValueError(f"params must be [{Cc}, 43], got {tuple(params.shape)}")
    if out is None:
        out = torch.zeros((Cc, 44), dtype=torch.float64, device=x_cb.device)
    else:
        out = _out(out, (Cc, 44), torch.float64, x_cb.device, "out", True, (("params", params), ("x_cb", x_cb)))
    check(_lib.lib().vbq_bmshj_nll_grad_f32(_ptr(params), _ptr(x_cb), n, Cc, _ptr(out), _stream(x_cb)),
          "vbq_bmshj_nll_grad_f32")
    return out


def budget_dp(fhat: torch.Tensor, K: int, budget: int, *, status: Optional[torch.Tensor] = None,
              workspace: Optional[torch.Tensor] = None):
    """vbq_budget_dp_f64: the allocation of exactly `budget` bits over the K coordinates of every row that maximises the summed
    score (utils.py:106-160).  fhat: f64 [N+1, rows * K] (or [N+1, rows, K]) = score of element row * K + k with exactly n bits.
    Returns (bits int32 [rows, K], objective f64 [rows]).  `status` (uint32 [1], zeroed by the caller) gets bit 0 set when a row
    held a NaN or +inf; `workspace` (uint8) replaces the one this call would allocate and may be smaller (more rounds)."""
    fhat = _dev(fhat, torch.float64, "fhat")
    N, K, budget = fhat.shape[0] - 1, int(K), int(budget)
    E = fhat[0].numel() if fhat.shape[0] else 0
    if K < 1 or E % K:
        raise ValueError(f"fhat holds {E} elements per level, not a multiple of K={K}")
    rows = E // K
    bits = torch.empty((rows, K), dtype=torch.int32, device=fhat.device)
    obj = torch.empty(rows, dtype=torch.float64, device=fhat.device)
    if status is not None:
        status = _status(status, 1, fhat.device, (("fhat", fhat),))
    h = _lib.lib()
    if workspace is None:
        wsb = h.vbq_budget_dp_workspace_bytes(rows, K, N, budget)
        workspace = torch.empty(wsb, dtype=torch.uint8, device=fhat.device) if wsb else None
    else:
        workspace = _workspace(workspace, 1, fhat.device, 0, (("fhat", fhat), ("status", status)))
    wsb = workspace.numel() if workspace is not None else 0
    check(h.vbq_budget_dp_f64(_ptr(fhat), rows, K, N, budget, _ptr(bits), _ptr(obj), _ptr(status), _ptr(workspace), wsb,
                              _stream(fhat)), "vbq_budget_dp_f64")
    return bits, obj


def budget_dp_sweep(fhat: torch.Tensor, K: int, budgets: Sequence[int], *, curve_len: int = 0, status: Optional[torch.Tensor] = None,
                    workspace: Optional[torch.Tensor] = None):
    """vbqb_budget_sweep_f64: budget_dp at every budget of `budgets` (ints, strictly ascending, at most 64 of them, each in
    [0, K * N]) from ONE forward pass at the largest, and with curve_len > 0 the optimal objective at every budget below
    curve_len <= K * N + 1 (include/vbq_budget.h, "Budget sweep").  fhat as for budget_dp.  Returns (bits int32 [S, rows, K],
    objective f64 [S, rows], curve f64 [rows, curve_len] or None); slice s equals budget_dp(fhat, K, budgets[s]) bit for bit and
    curve[r, n] is the objective budget_dp reports for row r at budget n.  No budgets and a curve is the curve-only pass, which
    keeps no back-pointers.  `status` and `workspace` as for budget_dp."""
    import operator
    from . import _lib_budget
    fhat = _dev(fhat, torch.float64, "fhat")
    N, K, curve_len = fhat.shape[0] - 1, int(K), operator.index(curve_len)
    E = fhat[0].numel() if fhat.shape[0] else 0
    if K < 1 or E % K:
        raise ValueError(f"fhat holds {E} elements per level, not a multiple of K={K}")
    rows = E // K
    budgets = [operator.index(b) for b in budgets]
    S = len(budgets)
    if any(not -(1 << 31) <= b < (1 << 31) for b in budgets) or not 0 <= curve_len < (1 << 31):
        raise ValueError(f"budgets {budgets} or curve_len {curve_len} outside the int32 range")
    bits = torch.empty((S, rows, K), dtype=torch.int32, device=fhat.device)
    obj = torch.empty((S, rows), dtype=torch.float64, device=fhat.device)
    curve = torch.empty((rows, curve_len), dtype=torch.float64, device=fhat.device) if curve_len else None
    if status is not None:
        status = _status(status, 1, fhat.device, (("fhat", fhat),))
    h = _lib_budget.lib()
    if workspace is None:
        wsb = h.vbqb_budget_sweep_workspace_bytes(rows, K, N, max([b + 1 for b in budgets] + [curve_len])) if S else 0
        workspace = torch.empty(wsb, dtype=torch.uint8, device=fhat.device) if wsb else None
    else:
        workspace = _workspace(workspace, 1, fhat.device, 0, (("fhat", fhat), ("status", status)))
    wsb = workspace.numel() if workspace is not None else 0
    _lib_budget.check(h.vbqb_budget_sweep_f64(_ptr(fhat), rows, K, N, (C.c_int32 * S)(*budgets), S, _ptr(bits), _ptr(obj),
                                              _ptr(curve), curve_len, _ptr(status), _ptr(workspace), wsb, _stream(fhat)),
                      "vbqb_budget_sweep_f64")
    return bits, obj, curve


def budget_patience(fhat: torch.Tensor, lamb: float, patience: int = 3):
    """vbq_budget_patience_f64: per element the scan of utils.encode_mode (utils.py:186-203) over g_b = fhat_b - lamb * b.
    fhat: f64 [N+1, E].  Returns (bits int32 [E], g f64 [E])."""
    fhat = _dev(fhat, torch.float64, "fhat")
    N = fhat.shape[0] - 1
    E = fhat[0].numel() if fhat.shape[0] else 0
    bits = torch.empty(E, dtype=torch.int32, device=fhat.device)
    g = torch.empty(E, dtype=torch.float64, device=fhat.device)
    check(_lib.lib().vbq_budget_patience_f64(_ptr(fhat), E, N, float(lamb), int(patience), _ptr(bits), _ptr(g), _stream(fhat)),
          "vbq_budget_patience_f64")
    return bits, g


def records_words(K: int, N: int, total_bits: int) -> int:
    """vbq_records_words: 32-bit words of one record of K coordinates at exactly total_bits raw bits; ValueError for sizes
    outside K >= 1, 1 <= N <= 10, 0 <= total_bits <= K * N."""
    n = int(_lib.lib().vbq_records_words(int(K), int(N), int(total_bits)))
    if n == 0:
        raise ValueError(f"no record for K={K} N={N} total_bits={total_bits} (need K >= 1, 1 <= N <= 10, 0 <= total_bits <= K*N)")
    return n


def records_pack(idx: torch.Tensor, total_bits: int, N: int, *, status: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vbq_records_pack_u16: rank indices u16 [R, K] -> the rows' fixed-size records, uint32 [R, record_words] (the "VBQr"
    record of include/vbq.h).  `status` (uint32 [1], zeroed by the caller) gets bit 0 set for an index >= T and bit 1 for a row
    whose bit lengths do not add up to total_bits; such a row's record is all zeros."""
    idx = _dev(idx, torch.uint16, "idx")
    if idx.dim() != 2:
        raise ValueError(f"idx must be [R, K], got shape {tuple(idx.shape)}")
    R, K = idx.shape
    words = _out(out, (R, records_words(K, N, total_bits)), torch.uint32, idx.device, "out", True, (("idx", idx),))
    if status is not None:
        status = _status(status, 1, idx.device, (("idx", idx), ("out", words)))
    check(_lib.lib().vbq_records_pack_u16(_ptr(idx), R, K, int(N), int(total_bits), _ptr(words), _ptr(status), _stream(idx)),
          "vbq_records_pack_u16")
    return words


# The status bits of vbq_records_unpack_f32 and vbq_records_topk_f32 that say what is wrong with a record (bit 3, a row id out of
# range, is about the call, not about a record).
RECORDS_UNPACK_STATUS = ((1, "a length field above N"), (2, "lengths that do not add up to total_bits"), (4, "non-zero padding"))


def _records_inputs(words, rows, K, N, total_bits, table_sorted, want_table=True):
    """What records_unpack and records_topk check alike: words [`rows`, record_words] and, where the code book is wanted,
    table_sorted holding T or K*T code points -> (n_tables, table f32 [n_tables, T])."""
    RW = records_words(K, N, total_bits)
    if words.dim() != 2 or words.shape[1] != RW:
        raise ValueError(f"words must be [{rows}, {RW}] for K={K} N={N} total_bits={total_bits}, got shape {tuple(words.shape)}")
    if not want_table:
        return 1, table_sorted
    T = table_size(N)
    if table_sorted is None or table_sorted.numel() not in (T, K * T):
        raise ValueError(f"table_sorted must hold T = {T} or K*T = {K}*{T} code points")
    n_tables = table_sorted.numel() // T
    return n_tables, _table(table_sorted, n_tables, T, "table_sorted")


def records_unpack(words: torch.Tensor, K: int, N: int, total_bits: int, table_sorted: Optional[torch.Tensor],
                   row_ids: Optional[torch.Tensor] = None, want_values: bool = True, want_idx: bool = False, *,
                   status: Optional[torch.Tensor] = None):
    """vbq_records_unpack_f32: records uint32 [R, record_words] -> (values f32 [rows, K] or None, idx u16 [rows, K] or None) of
    every row, or of the rows `row_ids` lists (int64 device tensor, any order, repeats allowed; IndexError outside [0, R) is the
    caller's check -- the kernel only refuses such a row).  table_sorted: f32 [T] / [1, T] (one code book) or [K, T] (one per
    column) in rank order; not needed without values.  The records are untrusted: `status` (uint32 [1], zeroed by the caller)
    gets bit 0 for a length field > N, bit 1 for lengths that do not add up to total_bits, bit 2 for non-zero padding, bit 3
    for a row id out of range, and such a row decodes to zeros.  With neither output wanted the call only validates."""
    words = _dev(words, torch.uint32, "words")
    K, N, total_bits = int(K), int(N), int(total_bits)
    n_tables, table_sorted = _records_inputs(words, "R", K, N, total_bits, table_sorted, want_values)
    R = words.shape[0]
    if row_ids is not None:
        row_ids = _dev(row_ids, torch.int64, "row_ids")
        if row_ids.dim() != 1:
            raise ValueError(f"row_ids must be one-dimensional, got shape {tuple(row_ids.shape)}")
    rows = R if row_ids is None else row_ids.numel()
    values = _out(None, (rows, K), torch.float32, words.device, "values", want_values)
    idx = _out(None, (rows, K), torch.uint16, words.device, "idx", want_idx)
    if status is not None:
        status = _status(status, 1, words.device, (("words", words), ("table_sorted", table_sorted), ("row_ids", row_ids)))
    check(_lib.lib().vbq_records_unpack_f32(_ptr(words), R, K, N, total_bits, _ptr(table_sorted) if want_values else None,
                                            n_tables, _ptr(row_ids), rows if row_ids is not None else 0, _ptr(values),
                                            _ptr(idx), _ptr(status), _stream(words)), "vbq_records_unpack_f32")
    return values, idx


_METRICS = {"dot": 0, "cosine": 1, 0: 0, 1: 1}


def _topk_args(queries, K, k, metric, exclude):
    """What records_topk and topk take alike -> (queries [Q, K], k, metric code, exclude [Q, E] or None, E)."""
    queries = _dev(queries, torch.float32, "queries")
    if queries.dim() != 2 or queries.shape[1] != K:
        raise ValueError(f"queries must be [Q, {K}], got shape {tuple(queries.shape)}")
    k = int(k)
    if not 1 <= k <= 64:
        raise ValueError(f"k = {k} outside 1..64")
    if metric not in _METRICS:
        raise ValueError(f"metric {metric!r} is neither 'dot' nor 'cosine'")
    E = 0
    if exclude is not None:
        exclude = _dev(exclude, torch.int64, "exclude")
        if exclude.dim() != 2 or exclude.shape[0] != queries.shape[0] or exclude.shape[1] > 8:
            raise ValueError(f"exclude must be [{queries.shape[0]}, E] with E <= 8, got shape {tuple(exclude.shape)}")
        E = exclude.shape[1]
    return queries, k, _METRICS[metric], (exclude if E else None), E


def _topk_outputs(h, V, K, Q, k, max_workgroups, workspace, device, reads):
    ids = torch.empty((Q, k), dtype=torch.int64, device=device)
    scores = torch.empty((Q, k), dtype=torch.float32, device=device)
    nbytes = int(h.vbq_topk_workspace_bytes(V, K, Q, k, int(max_workgroups))) if Q else 0
    return ids, scores, _workspace(workspace, nbytes, device, 1, reads)


def records_topk(words: torch.Tensor, K: int, N: int, total_bits: int, table_sorted: torch.Tensor, queries: torch.Tensor,
                 k: int = 10, metric="cosine", exclude: Optional[torch.Tensor] = None, *, status: Optional[torch.Tensor] = None,
                 max_workgroups: int = 0, workspace: Optional[torch.Tensor] = None):
    """vbq_records_topk_f32: the k rows of the records uint32 [V, record_words] that score highest against each query, without
    decoding the matrix (semantics: include/vbq.h, "Nearest rows").  queries f32 [Q, K], taken as given; metric "dot" or
    "cosine" (the score divided by 1e-8 + |row|); exclude int64 [Q, E <= 8], negative = none.  Returns (ids int64 [Q, k],
    scores f32 [Q, k]), ordered by score descending then id ascending, padded with -1 / -inf.  The records are untrusted:
    `status` (uint32 [1], zeroed by the caller) gets the unpack's bits and such a record counts as a row of zeros."""
    words = _dev(words, torch.uint32, "words")
    K, N, total_bits = int(K), int(N), int(total_bits)
    n_tables, table_sorted = _records_inputs(words, "V", K, N, total_bits, table_sorted)
    queries, k, metric, exclude, E = _topk_args(queries, K, k, metric, exclude)
    reads = (("words", words), ("table_sorted", table_sorted), ("queries", queries), ("exclude", exclude))
    if status is not None:
        status = _status(status, 1, words.device, reads)
    V, Q = words.shape[0], queries.shape[0]
    h = _lib.lib()
    ids, scores, ws = _topk_outputs(h, V, K, Q, k, max_workgroups, workspace, words.device, reads + (("status", status),))
    check(h.vbq_records_topk_f32(_ptr(words), V, K, N, total_bits, _ptr(table_sorted), n_tables, _ptr(queries), Q, k, metric,
                                 _ptr(exclude), E, _ptr(ids), _ptr(scores), _ptr(status), int(max_workgroups), _ptr(ws),
                                 ws.numel() * ws.element_size(), _stream(words)), "vbq_records_topk_f32")
    return ids, scores


def topk(emb: torch.Tensor, queries: torch.Tensor, k: int = 10, metric="cosine", exclude: Optional[torch.Tensor] = None, *,
         max_workgroups: int = 0, workspace: Optional[torch.Tensor] = None):
    """vbq_topk_f32: records_topk on a dense f32 [V, K] matrix -- the same kernel with a dense row loader, the same scores
    bit for bit."""
    emb = _dev(emb, torch.float32, "emb")
    if emb.dim() != 2:
        raise ValueError(f"emb must be [V, K], got shape {tuple(emb.shape)}")
    V, K = emb.shape
    queries, k, metric, exclude, E = _topk_args(queries, K, k, metric, exclude)
    Q = queries.shape[0]
    h = _lib.lib()
    ids, scores, ws = _topk_outputs(h, V, K, Q, k, max_workgroups, workspace, emb.device,
                                    (("emb", emb), ("queries", queries), ("exclude", exclude)))
    check(h.vbq_topk_f32(_ptr(emb), V, K, _ptr(queries), Q, k, metric, _ptr(exclude), E, _ptr(ids), _ptr(scores),
                         int(max_workgroups), _ptr(ws), ws.numel() * ws.element_size(), _stream(emb)), "vbq_topk_f32")
    return ids, scores


_BAG_MODES = {"sum": 0, "mean": 1, "max": 2, 0: 0, 1: 1, 2: 2}
BAG_BAD_ROW, BAG_BAD_OFFSETS = 8, 16             # status bits 3 and 4 of the bag calls (bits 0..2: RECORDS_UNPACK_STATUS)


def _bag_args(ids, offsets, weights, mode, status, out, K, device, rows):
    """What records_bag and bag take alike -> (ids [n], offsets [B + 1], weights [n] or None, mode code, status, out [B, K])."""
    ids = _dev(ids, torch.int64, "ids")
    offsets = _dev(offsets, torch.int64, "offsets")
    if ids.dim() != 1:
        raise ValueError(f"ids must be one-dimensional, got shape {tuple(ids.shape)}")
    if offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError(f"offsets must be [B + 1] (bag b is ids[offsets[b]:offsets[b + 1]]), got shape {tuple(offsets.shape)}")
    if mode not in _BAG_MODES:
        raise ValueError(f"mode {mode!r} is none of 'sum', 'mean', 'max'")
    mode = _BAG_MODES[mode]
    if weights is not None:
        if mode != 0:
            raise ValueError("weights go with mode 'sum' only")
        weights = _dev(weights, torch.float32, "weights")
        if weights.shape != ids.shape:
            raise ValueError(f"weights {tuple(weights.shape)} and ids {tuple(ids.shape)} differ in shape")
    reads = rows + (("ids", ids), ("offsets", offsets), ("weights", weights))
    out = _out(out, (offsets.numel() - 1, K), torch.float32, device, "out", True, reads)
    if status is not None:
        status = _status(status, 1, device, reads + (("out", out),))
    return ids, offsets, weights, mode, status, out


def records_bag(words: torch.Tensor, K: int, N: int, total_bits: int, table_sorted: torch.Tensor, ids: torch.Tensor,
                offsets: torch.Tensor, *, weights: Optional[torch.Tensor] = None, mode="sum",
                status: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vbq_records_bag_f32: per bag the sum, mean or max of the rows its ids list, straight from the records uint32
    [V, record_words]: no [len(ids), K] matrix exists (semantics: include/vbq.h, "Pooled rows").  ids int64 [n]; offsets int64
    [B + 1], bag b is ids[offsets[b]:offsets[b + 1]] in that order; weights f32 [n] with mode "sum" only.  Returns f32 [B, K].
    A negative id is padding.  `status` (uint32 [1], zeroed by the caller) gets the unpack's bits 0..2 for a damaged record
    (which counts as a row of zeros), bit 3 for an id >= V (skipped) and bit 4 for a bag whose offsets left [0, n] or ran
    backwards (clamped).  One wave pools one bag: many short bags are the case this is for, a few very long ones run
    serially."""
    words = _dev(words, torch.uint32, "words")
    K, N, total_bits = int(K), int(N), int(total_bits)
    n_tables, table_sorted = _records_inputs(words, "V", K, N, total_bits, table_sorted)
    ids, offsets, weights, mode, status, out = _bag_args(ids, offsets, weights, mode, status, out, K, words.device,
                                                         (("words", words), ("table_sorted", table_sorted)))
    check(_lib.lib().vbq_records_bag_f32(_ptr(words), words.shape[0], K, N, total_bits, _ptr(table_sorted), n_tables, _ptr(ids),
                                         ids.numel(), _ptr(offsets), offsets.numel() - 1, _ptr(weights), mode, _ptr(out),
                                         _ptr(status), _stream(words)), "vbq_records_bag_f32")
    return out


def bag(emb: torch.Tensor, ids: torch.Tensor, offsets: torch.Tensor, *, weights: Optional[torch.Tensor] = None, mode="sum",
        status: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vbq_bag_f32: records_bag on a dense f32 [V, K] matrix -- the same kernel with a dense row loader, the same result bit
    for bit."""
    emb = _dev(emb, torch.float32, "emb")
    if emb.dim() != 2:
        raise ValueError(f"emb must be [V, K], got shape {tuple(emb.shape)}")
    V, K = emb.shape
    ids, offsets, weights, mode, status, out = _bag_args(ids, offsets, weights, mode, status, out, K, emb.device, (("emb", emb),))
    check(_lib.lib().vbq_bag_f32(_ptr(emb), V, K, _ptr(ids), ids.numel(), _ptr(offsets), offsets.numel() - 1, _ptr(weights), mode,
                                 _ptr(out), _ptr(status), _stream(emb)), "vbq_bag_f32")
    return out


SCORES_BAD_ROW = 8                               # status bit 3 of the scores calls (bits 0..2: RECORDS_UNPACK_STATUS)


def _scores_args(queries, ids, K, metric, status, out, rows):
    """What records_scores and scores take alike -> (queries [Q, K], ids [Q, M], metric code, status, out [Q, M])."""
    queries = _dev(queries, torch.float32, "queries")
    if queries.dim() != 2 or queries.shape[1] != K:
        raise ValueError(f"queries must be [Q, {K}], got shape {tuple(queries.shape)}")
    ids = _dev(ids, torch.int64, "ids")
    if ids.dim() != 2 or ids.shape[0] != queries.shape[0]:
        raise ValueError(f"ids must be [{queries.shape[0]}, M], got shape {tuple(ids.shape)}")
    if metric not in _METRICS:
        raise ValueError(f"metric {metric!r} is neither 'dot' nor 'cosine'")
    reads = rows + (("queries", queries), ("ids", ids))
    out = _out(out, tuple(ids.shape), torch.float32, queries.device, "out", True, reads)
    if status is not None:
        status = _status(status, 1, queries.device, reads + (("out", out),))
    return queries, ids, _METRICS[metric], status, out


def records_scores(words: torch.Tensor, K: int, N: int, total_bits: int, table_sorted: torch.Tensor, queries: torch.Tensor,
                   ids: torch.Tensor, metric="cosine", *, status: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vbqx_records_scores_f32: the score of query q against each row ids[q, m] of the records uint32 [V, record_words], in one
    launch and without a [Q * M, K] matrix of the listed rows (semantics: include/vbq_ext.h, "Listed rows"; the scores are
    those records_topk reports, bit for bit).  queries f32 [Q, K], taken as given; ids int64 [Q, M]; metric "dot" or "cosine"
    (the score divided by 1e-8 + |row|).  Returns f32 [Q, M].  A negative id is padding and scores -inf; an id >= V scores
    -inf and sets bit 3 of `status` (uint32 [1], zeroed by the caller), a damaged record counts as a row of zeros and sets the
    unpack's bits 0..2."""
    from . import _lib_ext
    words = _dev(words, torch.uint32, "words")
    K, N, total_bits = int(K), int(N), int(total_bits)
    n_tables, table_sorted = _records_inputs(words, "V", K, N, total_bits, table_sorted)
    queries, ids, metric, status, out = _scores_args(queries, ids, K, metric, status, out,
                                                     (("words", words), ("table_sorted", table_sorted)))
    _lib_ext.check(_lib_ext.lib().vbqx_records_scores_f32(_ptr(words), words.shape[0], K, N, total_bits, _ptr(table_sorted),
                                                          n_tables, _ptr(queries), ids.shape[0], _ptr(ids), ids.shape[1], metric,
                                                          _ptr(out), _ptr(status), _stream(words)), "vbqx_records_scores_f32")
    return out


def scores(emb: torch.Tensor, queries: torch.Tensor, ids: torch.Tensor, metric="cosine", *,
           status: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vbqx_scores_f32: records_scores on a dense f32 [V, K] matrix -- the same kernel with a dense row loader, the same
    scores bit for bit."""
    from . import _lib_ext
    emb = _dev(emb, torch.float32, "emb")
    if emb.dim() != 2:
        raise ValueError(f"emb must be [V, K], got shape {tuple(emb.shape)}")
    V, K = emb.shape
    queries, ids, metric, status, out = _scores_args(queries, ids, K, metric, status, out, (("emb", emb),))
    _lib_ext.check(_lib_ext.lib().vbqx_scores_f32(_ptr(emb), V, K, _ptr(queries), ids.shape[0], _ptr(ids), ids.shape[1], metric,
                                                  _ptr(out), _ptr(status), _stream(emb)), "vbqx_scores_f32")
    return out


WINDOW_BAD_SEGMENT, WINDOW_BAD_FILE = 32, 128    # status bits 5 and 7 of the window decode (bits 0..3: the segment decoder's)


def _window_args(payload, sizes, offsets, files, fields, segs, freq, values, box, seg, N, channels, status, out):
    """The checks rans_decode_window and rans_map_decode_window share; `fields` = (count, names) of a descriptor.  -> the
    tensors as given or made (status zeroed, out empty), the box and F, n_ch_sel, n_ch, n_tables."""
    payload = _dev(payload, torch.uint16, "payload")
    sizes = _dev(sizes, torch.uint16, "sizes")
    offsets = _dev(offsets, torch.int64, "offsets")
    files = _dev(files, torch.int64, "files")
    segs = _dev(segs, torch.int32, "segs")
    freq = _dev(freq, torch.uint16, "freq")
    values = _dev(values, torch.float32, "values")
    T = table_size(N)
    if payload.dim() != 1 or sizes.dim() != 1 or offsets.shape != sizes.shape:
        raise ValueError(f"expected payload [n_words], sizes [M] and offsets [M], got {tuple(payload.shape)}, {tuple(sizes.shape)} "
                         f"and {tuple(offsets.shape)}")
    if files.dim() != 2 or files.shape[1] != fields[0]:
        raise ValueError(f"files must be [F, {fields[0]}] ({fields[1]}), got {tuple(files.shape)}")
    F = files.shape[0]
    if segs.dim() != 2 or segs.shape[0] != F:
        raise ValueError(f"segs must be [F = {F}, n_sel], got {tuple(segs.shape)}")
    if freq.dim() != 3 or freq.shape[2] != T or values.dim() != 2 or tuple(values.shape) != tuple(freq.shape[1:]):
        raise ValueError(f"expected freq [n_tables, C, {T}] and values [C, {T}], got {tuple(freq.shape)} and {tuple(values.shape)}")
    n_tables, n_ch = freq.shape[0], freq.shape[1]
    if channels is not None:
        channels = _dev(channels, torch.int32, "channels")
        if channels.dim() != 1:
            raise ValueError(f"channels must be one-dimensional, got shape {tuple(channels.shape)}")
    n_ch_sel = n_ch if channels is None else channels.numel()
    box = tuple(int(w) for w in box)
    if len(box) != 3 or min(box) < 0:
        raise ValueError(f"box must be three extents >= 0, got {box}")
    reads = (("payload", payload), ("sizes", sizes), ("offsets", offsets), ("files", files), ("segs", segs), ("freq", freq),
             ("values", values), ("channels", channels))
    if status is None:
        status = torch.zeros(F, dtype=torch.uint32, device=payload.device)
    else:
        status = _status(status, F, payload.device, reads)
    out = _out(out, (F,) + box + (n_ch_sel,), torch.float32, payload.device, "out", True, reads + (("status", status),))
    return payload, sizes, offsets, files, segs, freq, values, box, channels, status, out, F, n_ch_sel, n_ch, n_tables


def rans_decode_window(payload: torch.Tensor, sizes: torch.Tensor, offsets: torch.Tensor, files: torch.Tensor,
                       segs: torch.Tensor, freq: torch.Tensor, values: torch.Tensor, box: Sequence[int], *, seg: int, N: int = 10,
                       channels: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None):
    """vbq_rans_decode_window_f32 (include/vbq.h, "Window decode"): the box of extents box = (w0, w1, w2) of every listed file,
    straight from the concatenated payloads.  payload u16 [n_words]; sizes u16 [M] and offsets int64 [M] (their exclusive prefix
    sum) over all files; files int64 [F, 8] (seg_base, n, D1, D2, a0, a1, a2, table); segs int32 [F, n_sel], -1 = skip; freq
    u16 [n_tables, C, T]; values f32 [C, T]; channels int32 [C_sel] or None for all C in order.  Returns (out f32
    [F, w0, w1, w2, C_sel], status u32 [F]); positions no listed segment covers keep what `out` held.  `status` is OR-ed into:
    zeroed here unless given."""
    seg, N = int(seg), int(N)
    payload, sizes, offsets, files, segs, freq, values, box, channels, status, out, F, n_ch_sel, n_ch, n_tables = _window_args(
        payload, sizes, offsets, files, (8, "seg_base, n, D1, D2, a0, a1, a2, table"), segs, freq, values, box, seg, N, channels,
        status, out)
    check(_lib.lib().vbq_rans_decode_window_f32(_ptr(payload), payload.numel(), _ptr(sizes), _ptr(offsets), sizes.numel(),
                                                _ptr(files), F, _ptr(segs), segs.shape[1], _ptr(channels), n_ch_sel, n_ch, seg,
                                                N, _ptr(freq), n_tables, _ptr(values), box[0], box[1], box[2], _ptr(out),
                                                _ptr(status), _stream(payload)), "vbq_rans_decode_window_f32")
    return out, status


WINDOW_BAD_CLASS = 64                            # status bit 6 of the mapped window decode: a class outside the file's palette


def rans_map_decode_window(payload: torch.Tensor, sizes: torch.Tensor, offsets: torch.Tensor, files: torch.Tensor,
                           segs: torch.Tensor, freq: torch.Tensor, values: torch.Tensor, classes: Optional[torch.Tensor],
                           box: Sequence[int], *, seg: int, max_classes: int, N: int = 10,
                           channels: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None,
                           out: Optional[torch.Tensor] = None):
    """vbq_rans_map_decode_window_f32 (include/vbq.h, "Mapped window decode"): rans_decode_window with a table per symbol.
    files int64 [F, 16] (seg_base, n, D1, D2, a0, a1, a2, P, table[0..3], cls_base, 0, 0, 0); classes u8 [cls_bytes], a multiple
    of 8 bytes at an address that is one: the packed class blocks of the files (bitstream.pack_classes), file f's at byte
    cls_base_f -- or None when every file has cls_base = -1; max_classes the largest P of `files`, 1..4.  Everything else, and
    the result (out, status), as rans_decode_window."""
    seg, N, max_classes = int(seg), int(N), int(max_classes)
    given = [name for name, t in (("out", out), ("status", status)) if t is not None]
    payload, sizes, offsets, files, segs, freq, values, box, channels, status, out, F, n_ch_sel, n_ch, n_tables = _window_args(
        payload, sizes, offsets, files, (16, "seg_base, n, D1, D2, a0, a1, a2, P, table[0..3], cls_base, 0, 0, 0"), segs, freq,
        values, box, seg, N, channels, status, out)
    if classes is not None:
        classes = _dev(classes, torch.uint8, "classes")
        if classes.dim() != 1:
            raise ValueError(f"classes must be one-dimensional, got shape {tuple(classes.shape)}")
        for name in given:
            _apart(name, out if name == "out" else status, (("classes", classes),))
    check(_lib.lib().vbq_rans_map_decode_window_f32(_ptr(payload), payload.numel(), _ptr(sizes), _ptr(offsets), sizes.numel(),
                                                    _ptr(files), F, _ptr(segs), segs.shape[1], _ptr(channels), n_ch_sel, n_ch,
                                                    seg, N, _ptr(freq), n_tables, _ptr(values), _ptr(classes),
                                                    0 if classes is None else classes.numel(), max_classes, box[0], box[1],
                                                    box[2], _ptr(out), _ptr(status), _stream(payload)),
          "vbq_rans_map_decode_window_f32")
    return out, status


ENCODE_BAD_FILE = 128                            # status bit 7 of the batch encode


def rans_encode_files(idx: torch.Tensor, files: torch.Tensor, items: torch.Tensor, freq: torch.Tensor, M: int, *, seg: int,
                      N: int = 10, canon: Optional[torch.Tensor] = None, words: Optional[torch.Tensor] = None,
                      sizes: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """vbq_rans_encode_files_u16 (include/vbq.h, "Batch encode"): every listed segment of every file in one launch.  idx u16
    [n_idx], all files' rank indices; files int64 [F, 6] (idx_base, idx_stride, n, seg_base, table, 0); items int32 [n_items, 2]
    (file, segment), n_items a multiple of 64, a block of 64 of one table, file -1 = padding (bitstream.encode_plan builds
    both); freq u16 [n_tables, C, T]; canon u16 [C, T] or None.  Returns (words u16 [M, seg + 2], sizes u32 [M], status u32
    [F]): slot seg_base_f + c nseg_f + g holds segment g of channel c of file f as RansCodec.encode writes it; slots no item
    names keep what `words` / `sizes` held (new ones are zeroed).  `status` is OR-ed into: zeroed here unless given."""
    idx = _dev(idx, torch.uint16, "idx")
    files = _dev(files, torch.int64, "files")
    items = _dev(items, torch.int32, "items")
    freq = _dev(freq, torch.uint16, "freq")
    seg, N, M = int(seg), int(N), int(M)
    T = table_size(N)
    if files.dim() != 2 or files.shape[1] != 6:
        raise ValueError(f"files must be [F, 6] (idx_base, idx_stride, n, seg_base, table, 0), got {tuple(files.shape)}")
    if items.dim() != 2 or items.shape[1] != 2:
        raise ValueError(f"items must be [n_items, 2] (file, segment), got {tuple(items.shape)}")
    if freq.dim() != 3 or freq.shape[2] != T:
        raise ValueError(f"expected freq [n_tables, C, {T}], got {tuple(freq.shape)}")
    F, n_tables, n_ch = files.shape[0], freq.shape[0], freq.shape[1]
    if canon is not None:
        canon = _dev(canon, torch.uint16, "canon")
        if tuple(canon.shape) != (n_ch, T):
            raise ValueError(f"canon must be [{n_ch}, {T}], got {tuple(canon.shape)}")
    if M < 0:
        raise ValueError(f"M = {M} slots")
    reads = (("idx", idx), ("files", files), ("items", items), ("freq", freq), ("canon", canon))
    given = words is not None
    words = _out(words, (M, seg + 2), torch.uint16, idx.device, "words", True, reads)
    if not given:
        words.zero_()
    if sizes is None:
        sizes = torch.zeros(M, dtype=torch.uint32, device=idx.device)
    else:
        sizes = _out(sizes, (M,), torch.uint32, idx.device, "sizes", True, reads + (("words", words),))
    if status is None:
        status = torch.zeros(F, dtype=torch.uint32, device=idx.device)
    else:
        status = _status(status, F, idx.device, reads + (("words", words), ("sizes", sizes)))
    check(_lib.lib().vbq_rans_encode_files_u16(_ptr(idx), idx.numel(), _ptr(files), F, _ptr(items), items.shape[0], n_ch, seg, N,
                                               _ptr(freq), n_tables, _ptr(canon), _ptr(words), _ptr(sizes), M, _ptr(status),
                                               _stream(idx)), "vbq_rans_encode_files_u16")
    return words, sizes, status


def rans_sizes_files(idx: torch.Tensor, files: torch.Tensor, items: torch.Tensor, freq: torch.Tensor, *, lambda_stride: int,
                     seg: int, N: int = 10, canon: Optional[torch.Tensor] = None, totals: Optional[torch.Tensor] = None,
                     status: Optional[torch.Tensor] = None):
    """vbq_rans_sizes_files_u16 (include/vbq.h, "Batch sizes"): the coded words of every file at every lambda in one launch.
    idx u16 [n_idx], the rank indices of all files, one plane of lambda_stride indices per lambda; files int64 [F, 6] and items
    int32 [n_items, 2] as rans_encode_files takes them (idx_base, idx_stride and n are read; a block's files need share
    nothing); freq u16 [L, C, T]; canon u16 [C, T] or None.  Returns (totals u64 [L, F], status u32 [F]): totals[l, f] grows by
    the words of every listed segment of every channel of file f at lambda l.  `totals` is added to and `status` OR-ed into:
    zeroed here unless given."""
    idx = _dev(idx, torch.uint16, "idx")
    files = _dev(files, torch.int64, "files")
    items = _dev(items, torch.int32, "items")
    freq = _dev(freq, torch.uint16, "freq")
    seg, N, lambda_stride = int(seg), int(N), int(lambda_stride)
    T = table_size(N)
    if files.dim() != 2 or files.shape[1] != 6:
        raise ValueError(f"files must be [F, 6] (idx_base, idx_stride, n, seg_base, table, 0), got {tuple(files.shape)}")
    if items.dim() != 2 or items.shape[1] != 2:
        raise ValueError(f"items must be [n_items, 2] (file, segment), got {tuple(items.shape)}")
    if freq.dim() != 3 or freq.shape[2] != T:
        raise ValueError(f"expected freq [L, C, {T}], got {tuple(freq.shape)}")
    F, L, n_ch = files.shape[0], freq.shape[0], freq.shape[1]
    if canon is not None:
        canon = _dev(canon, torch.uint16, "canon")
        if tuple(canon.shape) != (n_ch, T):
            raise ValueError(f"canon must be [{n_ch}, {T}], got {tuple(canon.shape)}")
    reads = (("idx", idx), ("files", files), ("items", items), ("freq", freq), ("canon", canon))
    if totals is None:
        totals = torch.zeros((L, F), dtype=torch.int64, device=idx.device).view(torch.uint64)
    else:
        totals = _out(totals, (L, F), torch.uint64, idx.device, "totals", True, reads)
    if status is None:
        status = torch.zeros(F, dtype=torch.uint32, device=idx.device)
    else:
        status = _status(status, F, idx.device, reads + (("totals", totals),))
    check(_lib.lib().vbq_rans_sizes_files_u16(_ptr(idx), idx.numel(), lambda_stride, _ptr(files), F, _ptr(items), items.shape[0],
                                              n_ch, seg, N, _ptr(freq), L, _ptr(canon), _ptr(totals), _ptr(status),
                                              _stream(idx)), "vbq_rans_sizes_files_u16")
    return totals, status


def _map_files_args(idx, classes, files, palettes, items, freq, M, seg, N, canon, words, sizes, status):
    """What rans_map_encode_files and rans_map_sizes_files share: the checks and the outputs; `words` is False for the sizes
    entry.  -> (words or None, sizes, status)."""
    idx = _dev(idx, torch.uint16, "idx")
    classes = _dev(classes, torch.uint8, "classes")
    files = _dev(files, torch.int64, "files")
    palettes = _dev(palettes, torch.int32, "palettes")
    items = _dev(items, torch.int32, "items")
    freq = _dev(freq, torch.uint16, "freq")
    seg, N, M = int(seg), int(N), int(M)
    T = table_size(N)
    if files.dim() != 2 or files.shape[1] != 8:
        raise ValueError("files must be [F, 8] (idx_base, idx_stride, plane_stride, n, seg_base, palette, cls_base, 0), got "
                         f"{tuple(files.shape)}")
    if palettes.dim() != 2 or palettes.shape[1] != 4:
        raise ValueError(f"palettes must be [n_palettes, 4] (tables, class 0 first, -1 past P), got {tuple(palettes.shape)}")
    if items.dim() != 2 or items.shape[1] != 2:
        raise ValueError(f"items must be [n_items, 2] (file, segment), got {tuple(items.shape)}")
    if freq.dim() != 3 or freq.shape[2] != T:
        raise ValueError(f"expected freq [n_tables, C, {T}], got {tuple(freq.shape)}")
    F, n_tables, n_ch = files.shape[0], freq.shape[0], freq.shape[1]
    if canon is not None:
        canon = _dev(canon, torch.uint16, "canon")
        if tuple(canon.shape) != (n_ch, T):
            raise ValueError(f"canon must be [{n_ch}, {T}], got {tuple(canon.shape)}")
    if M < 0:
        raise ValueError(f"M = {M} slots")
    reads = (("idx", idx), ("classes", classes), ("files", files), ("palettes", palettes), ("items", items), ("freq", freq),
             ("canon", canon))
    given = words is not None
    if words is not False:
        words = _out(words, (M, seg + 2), torch.uint16, idx.device, "words", True, reads)
        if not given:
            words.zero_()
        reads += (("words", words),)
    if sizes is None:
        sizes = torch.zeros(M, dtype=torch.uint32, device=idx.device)
    else:
        sizes = _out(sizes, (M,), torch.uint32, idx.device, "sizes", True, reads)
    if status is None:
        status = torch.zeros(F, dtype=torch.uint32, device=idx.device)
    else:
        status = _status(status, F, idx.device, reads + (("sizes", sizes),))
    return idx, classes, files, palettes, items, freq, canon, words, sizes, status, F, n_tables, n_ch, M, seg, N


def rans_map_encode_files(idx: torch.Tensor, classes: torch.Tensor, files: torch.Tensor, palettes: torch.Tensor,
                          items: torch.Tensor, freq: torch.Tensor, M: int, *, seg: int, max_classes: int, N: int = 10,
                          canon: Optional[torch.Tensor] = None, words: Optional[torch.Tensor] = None,
                          sizes: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """vbq_rans_map_encode_files_u16 (include/vbq.h, "Mapped batch encode"): rans_encode_files with a table per symbol.  idx u16
    [n_idx], the index planes of all files; classes u8 [n_cls], their class bytes; files int64 [F, 8] (idx_base, idx_stride,
    plane_stride, n, seg_base, palette, cls_base, 0); palettes int32 [n_palettes, 4] (blocks of freq, class 0 first, -1 past P);
    items int32 [n_items, 2] (file, segment), n_items a multiple of 64, a block of 64 of one palette, file -1 = padding
    (bitstream.mapped_encode_plan builds all three); freq u16 [n_tables, C, T]; canon u16 [C, T] or None; max_classes the
    largest P in use, 1..4.  Returns (words u16 [M, seg + 2], sizes u32 [M], status u32 [F]): slot seg_base_f + c nseg_f + g
    holds segment g of channel c of file f as MappedRansCodec.encode writes it; slots no item names keep what `words` / `sizes`
    held (new ones are zeroed).  `status` is OR-ed into: zeroed here unless given."""
    idx, classes, files, palettes, items, freq, canon, words, sizes, status, F, n_tables, n_ch, M, seg, N = _map_files_args(
        idx, classes, files, palettes, items, freq, M, seg, N, canon, words, sizes, status)
    check(_lib.lib().vbq_rans_map_encode_files_u16(_ptr(idx), idx.numel(), _ptr(classes), classes.numel(), _ptr(files), F,
                                                   _ptr(palettes), palettes.shape[0], int(max_classes), _ptr(items),
                                                   items.shape[0], n_ch, seg, N, _ptr(freq), n_tables, _ptr(canon), _ptr(words),
                                                   _ptr(sizes), M, _ptr(status), _stream(idx)), "vbq_rans_map_encode_files_u16")
    return words, sizes, status


def rans_map_sizes_files(idx: torch.Tensor, classes: torch.Tensor, files: torch.Tensor, palettes: torch.Tensor,
                         items: torch.Tensor, freq: torch.Tensor, M: int, *, seg: int, max_classes: int, N: int = 10,
                         canon: Optional[torch.Tensor] = None, sizes: Optional[torch.Tensor] = None,
                         status: Optional[torch.Tensor] = None):
    """vbq_rans_map_sizes_files_u16: the sizes of rans_map_encode_files for the same arguments, without the words.  Returns
    (sizes u32 [M], status u32 [F])."""
    idx, classes, files, palettes, items, freq, canon, _, sizes, status, F, n_tables, n_ch, M, seg, N = _map_files_args(
        idx, classes, files, palettes, items, freq, M, seg, N, canon, False, sizes, status)
    check(_lib.lib().vbq_rans_map_sizes_files_u16(_ptr(idx), idx.numel(), _ptr(classes), classes.numel(), _ptr(files), F,
                                                  _ptr(palettes), palettes.shape[0], int(max_classes), _ptr(items),
                                                  items.shape[0], n_ch, seg, N, _ptr(freq), n_tables, _ptr(canon), _ptr(sizes),
                                                  M, _ptr(status), _stream(idx)), "vbq_rans_map_sizes_files_u16")
    return sizes, status


def rans_map_rates_files(idx: torch.Tensor, classes: torch.Tensor, files: torch.Tensor, palettes: torch.Tensor,
                         items: torch.Tensor, freq: torch.Tensor, *, lambda_stride: int, seg: int, max_classes: int,
                         N: int = 10, canon: Optional[torch.Tensor] = None, totals: Optional[torch.Tensor] = None,
                         status: Optional[torch.Tensor] = None):
    """vbq_rans_map_rates_files_u16 (include/vbq.h, "Mapped batch rates"): the coded words of every file under every candidate
    palette in one launch -- rans_sizes_files with a table per symbol.  idx u16 [n_idx], the rank indices of all files, one
    plane of lambda_stride indices per lambda; classes u8 [n_cls], the files' class bytes; files int64 [F, 8] and items int32
    [n_items, 2] as rans_map_encode_files takes them (idx_base, idx_stride, n and cls_base are read; a block's files need share
    nothing); palettes int32 [K, 4], per candidate the planes of idx (= the blocks of freq) of its classes, class 0 first, -1
    past P; freq u16 [L, C, T]; canon u16 [C, T] or None; max_classes the largest P of the candidates, 1..4.  Returns (totals
    u64 [K, F], status u32 [F]): totals[k, f] grows by the words of every listed segment of every channel of file f under
    candidate k.  `totals` is added to and `status` OR-ed into: zeroed here unless given."""
    idx = _dev(idx, torch.uint16, "idx")
    classes = _dev(classes, torch.uint8, "classes")
    files = _dev(files, torch.int64, "files")
    palettes = _dev(palettes, torch.int32, "palettes")
    items = _dev(items, torch.int32, "items")
    freq = _dev(freq, torch.uint16, "freq")
    seg, N, lambda_stride = int(seg), int(N), int(lambda_stride)
    T = table_size(N)
    if files.dim() != 2 or files.shape[1] != 8:
        raise ValueError("files must be [F, 8] (idx_base, idx_stride, plane_stride, n, seg_base, palette, cls_base, 0), got "
                         f"{tuple(files.shape)}")
    if palettes.dim() != 2 or palettes.shape[1] != 4:
        raise ValueError(f"palettes must be [K, 4] (planes, class 0 first, -1 past P), got {tuple(palettes.shape)}")
    if items.dim() != 2 or items.shape[1] != 2:
        raise ValueError(f"items must be [n_items, 2] (file, segment), got {tuple(items.shape)}")
    if freq.dim() != 3 or freq.shape[2] != T:
        raise ValueError(f"expected freq [L, C, {T}], got {tuple(freq.shape)}")
    F, K, L, n_ch = files.shape[0], palettes.shape[0], freq.shape[0], freq.shape[1]
    if canon is not None:
        canon = _dev(canon, torch.uint16, "canon")
        if tuple(canon.shape) != (n_ch, T):
            raise ValueError(f"canon must be [{n_ch}, {T}], got {tuple(canon.shape)}")
    reads = (("idx", idx), ("classes", classes), ("files", files), ("palettes", palettes), ("items", items), ("freq", freq),
             ("canon", canon))
    if totals is None:
        totals = torch.zeros((K, F), dtype=torch.int64, device=idx.device).view(torch.uint64)
    else:
        totals = _out(totals, (K, F), torch.uint64, idx.device, "totals", True, reads)
    if status is None:
        status = torch.zeros(F, dtype=torch.uint32, device=idx.device)
    else:
        status = _status(status, F, idx.device, reads + (("totals", totals),))
    check(_lib.lib().vbq_rans_map_rates_files_u16(_ptr(idx), idx.numel(), lambda_stride, _ptr(classes), classes.numel(),
                                                  _ptr(files), F, _ptr(palettes), K, int(max_classes), _ptr(items), items.shape[0],
                                                  n_ch, seg, N, _ptr(freq), L, _ptr(canon), _ptr(totals), _ptr(status),
                                                  _stream(idx)), "vbq_rans_map_rates_files_u16")
    return totals, status


# ---- batches of compact files (include/vbq.h, "Compact batch"): one wave per (file, part)
def _il_files_args(idx, files, items, freq, N, status):
    """What the four compact-batch calls check alike, `idx` having been checked by the caller (the encoders read it, the decoder
    writes it) -> (files, items, freq, status, F, n_tables, n_ch)."""
    files = _dev(files, torch.int64, "files")
    items = _dev(items, torch.int32, "items")
    freq = _dev(freq, torch.uint16, "freq")
    T = table_size(int(N))
    if files.dim() != 2 or files.shape[1] != 8:
        raise ValueError("files must be [F, 8] (idx_base, idx_stride, n, part_base, table, part, word_base, n_words_f), got "
                         f"{tuple(files.shape)}")
    if items.dim() != 2 or items.shape[1] != 2:
        raise ValueError(f"items must be [n_items, 2] (file, part), got {tuple(items.shape)}")
    if freq.dim() != 3 or freq.shape[2] != T:
        raise ValueError(f"expected freq [n_tables, C, {T}], got {tuple(freq.shape)}")
    F = files.shape[0]
    if status is None:
        status = torch.zeros(F, dtype=torch.uint32, device=idx.device)
    else:
        status = _status(status, F, idx.device, (("idx", idx), ("files", files), ("items", items), ("freq", freq)))
    return files, items, freq, status, F, freq.shape[0], freq.shape[1]


def _il_canon(canon, n_ch, N):
    if canon is None:
        return None
    canon = _dev(canon, torch.uint16, "canon")
    if tuple(canon.shape) != (n_ch, table_size(int(N))):
        raise ValueError(f"canon must be [{n_ch}, {table_size(int(N))}], got {tuple(canon.shape)}")
    return canon


def rans_il_sizes_files(idx: torch.Tensor, files: torch.Tensor, items: torch.Tensor, freq: torch.Tensor, P_all: int, *,
                        N: int = 10, canon: Optional[torch.Tensor] = None, sizes: Optional[torch.Tensor] = None,
                        status: Optional[torch.Tensor] = None):
    """vbq_rans_il_sizes_files_u16 (include/vbq.h, "Compact batch"): the words of every listed part of every file in one
    launch.  idx u16 [n_idx]; files int64 [F, 8] and items int32 [n_items, 2] (file, part), file -1 = padding
    (bitstream.compact_plan builds both); freq u16 [n_tables, C, T]; canon u16 [C, T] or None.  Returns (sizes u32 [P_all],
    status u32 [F]): entry part_base_f + p is what RansCodec.sizes_interleaved gives for that file alone; entries no item names
    keep what `sizes` held (a new one is zeroed).  `status` is OR-ed into: zeroed here unless given."""
    idx = _dev(idx, torch.uint16, "idx")
    given = status is not None
    files, items, freq, status, F, n_tables, n_ch = _il_files_args(idx, files, items, freq, N, status)
    canon = _il_canon(canon, n_ch, N)
    if given:
        _apart("status", status, (("canon", canon),))
    P_all = int(P_all)
    if P_all < 0:
        raise ValueError(f"P_all = {P_all} parts")
    if sizes is None:
        sizes = torch.zeros(P_all, dtype=torch.uint32, device=idx.device)
    else:
        sizes = _out(sizes, (P_all,), torch.uint32, idx.device, "sizes", True,
                     (("idx", idx), ("files", files), ("items", items), ("freq", freq), ("canon", canon), ("status", status)))
    check(_lib.lib().vbq_rans_il_sizes_files_u16(_ptr(idx), idx.numel(), _ptr(files), F, _ptr(items), items.shape[0], n_ch,
                                                 int(N), _ptr(freq), n_tables, _ptr(canon), _ptr(sizes), P_all, _ptr(status),
                                                 _stream(idx)), "vbq_rans_il_sizes_files_u16")
    return sizes, status


def rans_il_rates_files(idx: torch.Tensor, files: torch.Tensor, items: torch.Tensor, freq: torch.Tensor, P_all: int, *,
                        lambda_stride: int, N: int = 10, canon: Optional[torch.Tensor] = None,
                        sizes: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """vbq_rans_il_rates_files_u16 (include/vbq.h, "Compact batch"): the words of every listed part of every file at every
    lambda in one launch.  idx u16 [n_idx], one plane of lambda_stride indices per lambda; files int64 [F, 8] (every `table`
    0) and items int32 [n_items, 2] as rans_il_sizes_files takes them; freq u16 [L, C, T], one row block per lambda; canon u16
    [C, T] or None.  Returns (sizes u32 [L, P_all], status u32 [F]): sizes[l] is what rans_il_sizes_files gives on plane l
    with freq[l]; entries no item names keep what `sizes` held (a new one is zeroed).  `status` is OR-ed into: zeroed here
    unless given."""
    idx = _dev(idx, torch.uint16, "idx")
    given = status is not None
    files, items, freq, status, F, L, n_ch = _il_files_args(idx, files, items, freq, N, status)
    canon = _il_canon(canon, n_ch, N)
    if given:
        _apart("status", status, (("canon", canon),))
    P_all, lambda_stride = int(P_all), int(lambda_stride)
    if P_all < 0:
        raise ValueError(f"P_all = {P_all} parts")
    if sizes is None:
        sizes = torch.zeros((L, P_all), dtype=torch.uint32, device=idx.device)
    else:
        sizes = _out(sizes, (L, P_all), torch.uint32, idx.device, "sizes", True,
                     (("idx", idx), ("files", files), ("items", items), ("freq", freq), ("canon", canon), ("status", status)))
    check(_lib.lib().vbq_rans_il_rates_files_u16(_ptr(idx), idx.numel(), lambda_stride, _ptr(files), F, _ptr(items),
                                                 items.shape[0], n_ch, int(N), _ptr(freq), L, _ptr(canon), _ptr(sizes), P_all,
                                                 _ptr(status), _stream(idx)), "vbq_rans_il_rates_files_u16")
    return sizes, status


def rans_il_encode_files(idx: torch.Tensor, files: torch.Tensor, items: torch.Tensor, freq: torch.Tensor, sizes: torch.Tensor,
                         offsets: torch.Tensor, payload: torch.Tensor, *, N: int = 10, canon: Optional[torch.Tensor] = None,
                         status: Optional[torch.Tensor] = None):
    """vbq_rans_il_encode_files_u16: every listed part into payload u16 [n_words] at offsets int64 [P_all], with sizes u32
    [P_all] from rans_il_sizes_files (the same idx, files, items, freq and canon).  A part's words are those of
    RansCodec.encode_interleaved for its file alone.  Returns (payload, status u32 [F])."""
    idx = _dev(idx, torch.uint16, "idx")
    given = status is not None
    files, items, freq, status, F, n_tables, n_ch = _il_files_args(idx, files, items, freq, N, status)
    canon = _il_canon(canon, n_ch, N)
    sizes = _dev(sizes, torch.uint32, "sizes").reshape(-1)
    offsets = _dev(offsets, torch.int64, "offsets").reshape(-1)
    more = (("canon", canon), ("sizes", sizes), ("offsets", offsets))
    if given:
        _apart("status", status, more)
    payload = _out(payload, "any", torch.uint16, idx.device, "payload", False,
                   (("idx", idx), ("files", files), ("items", items), ("freq", freq), ("status", status)) + more)
    if payload is None:
        raise ValueError(f"payload: expected a contiguous {torch.uint16} device tensor of shape any")
    if offsets.numel() != sizes.numel():
        raise ValueError(f"{sizes.numel()} sizes and {offsets.numel()} offsets")
    check(_lib.lib().vbq_rans_il_encode_files_u16(_ptr(idx), idx.numel(), _ptr(files), F, _ptr(items), items.shape[0], n_ch,
                                                  int(N), _ptr(freq), n_tables, _ptr(canon), _ptr(sizes), _ptr(offsets),
                                                  sizes.numel(), _ptr(payload), payload.numel(), _ptr(status), _stream(idx)),
          "vbq_rans_il_encode_files_u16")
    return payload, status


def rans_il_decode_files(payload: torch.Tensor, sizes: torch.Tensor, offsets: torch.Tensor, files: torch.Tensor,
                         items: torch.Tensor, freq: torch.Tensor, idx: torch.Tensor, *, N: int = 10,
                         status: Optional[torch.Tensor] = None):
    """vbq_rans_il_decode_files_u16: every listed part of every file from payload u16 [n_words], sizes u32 [P_all] and offsets
    int64 [P_all] -- all UNTRUSTED -- into idx u16 [n_idx] at the positions the descriptors name (files [F, 8] with the word
    fields filled in); positions of no listed part keep what `idx` held.  Returns (idx, status u32 [F]): a part with a status
    bit decoded to zeros (read the words with coder._raise_status)."""
    idx = _out(idx, "any", torch.uint16, None, "idx", False)
    if idx is None:
        raise ValueError(f"idx: expected a contiguous {torch.uint16} device tensor of shape any")
    given = status is not None
    files, items, freq, status, F, n_tables, n_ch = _il_files_args(idx, files, items, freq, N, status)
    if idx.device != files.device:
        raise ValueError(f"idx: expected a contiguous {torch.uint16} device tensor of shape any")
    _apart("idx", idx, (("files", files), ("items", items), ("freq", freq)))
    payload = _dev(payload, torch.uint16, "payload").reshape(-1)
    sizes = _dev(sizes, torch.uint32, "sizes").reshape(-1)
    offsets = _dev(offsets, torch.int64, "offsets").reshape(-1)
    for name, t in (("idx", idx), ("status", status))[:1 + given]:
        _apart(name, t, (("payload", payload), ("sizes", sizes), ("offsets", offsets)))
    if offsets.numel() != sizes.numel():
        raise ValueError(f"{sizes.numel()} sizes and {offsets.numel()} offsets")
    check(_lib.lib().vbq_rans_il_decode_files_u16(_ptr(payload), payload.numel(), _ptr(sizes), _ptr(offsets), sizes.numel(),
                                                  _ptr(files), F, _ptr(items), items.shape[0], n_ch, int(N), _ptr(freq),
                                                  n_tables, _ptr(idx), idx.numel(), _ptr(status), _stream(idx)),
          "vbq_rans_il_decode_files_u16")
    return idx, status
