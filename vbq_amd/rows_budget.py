"""quantize_rows_to_budget(mu, sigma, total_bits): every row of a matrix quantized to EXACTLY total_bits raw bits.

Where quantize() picks a lambda and takes whatever rate falls out, and compress_to_budget searches lambda for a file size "at
most" a budget of the whole tensor, this solves the constrained problem per row: the allocation of total_bits over the K
coordinates, at most N each, with the largest Gaussian score (the budget DP of img-compression/utils.py:106-160, batched:
vbq_budget_dp_f64).  Rows of equal cost are fixed-size records, addressable without an entropy coder.
vbq_amd.embeddings.compress_to_records stores them as such (vbq_amd.bitstream, magic b"VBQr"); RecordEmbeddings looks rows up.

quantize_rows_to_budgets(mu, sigma, budgets) is the same at many budgets, and budget_curve(mu, sigma) the objective of every
row at EVERY budget, from one forward pass of the DP each (vbqb_budget_sweep_f64, include/vbq_budget.h): the recurrence does
not depend on the budget it is run for.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from ._lib import VBQError
from .api import _device_table
from .tables import table_size


def level_candidates(mu_t: torch.Tensor, sg_t: torch.Tensor, tab_lm: torch.Tensor, N: int):
    """Per level n = 0..N and element (r, k): the better of the two n-bit neighbours of mu (vbq_n_bit_intervals_f32) under the
    score -0.5 * ((c - mu) / sigma)**2 in f64; the right neighbour only when strictly better; level 0 is the root table[..., 0].
    mu_t, sg_t [R, K] and tab_lm [C, T] are f32 device tensors (ValueError for another dtype).  -> (scores f64, values f32) [N+1, R, K]."""
    mu_t, sg_t, tab_lm = (ops._dev(t, torch.float32, name) for t, name in ((mu_t, "mu_t"), (sg_t, "sg_t"), (tab_lm, "tab_lm")))
    (R, K), C = mu_t.shape, tab_lm.shape[0]
    z_cb = ops.transpose(mu_t) if C > 1 else mu_t.reshape(1, R * K)                  # [K, R] planes, or one plane of R*K
    B = z_cb.shape[1]
    left = torch.empty((C, N + 1, B), dtype=torch.float32, device=mu_t.device)
    right = torch.empty_like(left)
    _lib.check(_lib.lib().vbq_n_bit_intervals_f32(ops._ptr(z_cb), B, C, ops._ptr(tab_lm), N, ops._ptr(left), ops._ptr(right),
                                                  ops._stream(z_cb)), "vbq_n_bit_intervals_f32")
    if C > 1:
        left, right = left.permute(1, 2, 0), right.permute(1, 2, 0)                 # [N+1, R, K]
    else:
        left, right = left.reshape(N + 1, R, K), right.reshape(N + 1, R, K)
    mu64, sg64 = mu_t.to(torch.float64), sg_t.to(torch.float64)

    def score(c):
        t = (c.to(torch.float64) - mu64) / sg64
        return -0.5 * (t * t)
    s_l, s_r = score(left), score(right)
    take_r = s_r > s_l
    scores = torch.where(take_r, s_r, s_l).contiguous()
    values = torch.where(take_r, right, left).contiguous()
    root = tab_lm[:, 0].expand(R, K) if C > 1 else tab_lm[0, 0].expand(R, K)
    values[0] = root
    scores[0] = score(root)
    return scores, values


def quantize_rows_to_budget(mu, sigma, total_bits, *, table, N: int = 10):
    """Quantize every row of mu [R, K] to exactly total_bits raw bits, at most N per coordinate.

    mu, sigma  : f32 [R, K], torch (device) or NumPy.
    total_bits : an int, or an int array [R] with one budget per row (rows are grouped by budget, one launch per distinct value);
                 0 <= total_bits <= K * N.
    table      : level-major f32 code points, one code book [T] or one per column [K, T], T = 2**(N+1) - 1, monotone in xi.
    Returns device tensors (idx, num_bits, objective): idx uint16 [R, K] = the rank index of the chosen code point (the lower
    bound of its value in the sorted table, as quantize() gives it: feeds RansCodec, ops.histogram and ops.gather unchanged),
    num_bits int32 [R, K] = its bit length (every row sums to its budget), objective f64 [R] = the row's summed score
    -0.5 * ((c - mu) / sigma)**2 in float64, accumulated over ascending k.  The best allocation is exact: no other allocation
    of the same total has a larger objective.  Raises VBQError when a score is NaN or +inf (sigma <= 0, non-finite inputs)."""
    mu_t, sg_t, tab_lm, tab_sorted, C = _rows_args("quantize_rows_to_budget", mu, sigma, table, N)
    dev = mu_t.device
    R, K = mu_t.shape
    budgets = (total_bits.detach().cpu() if isinstance(total_bits, torch.Tensor) else ops.host_tensor(total_bits)).reshape(-1)
    if budgets.dtype.is_floating_point or budgets.numel() not in (1, R):
        raise ValueError("total_bits must be an int or an int array with one entry per row")
    budgets = budgets.to(torch.int64)
    num_bits = torch.empty((R, K), dtype=torch.int32, device=dev)
    objective = torch.empty(R, dtype=torch.float64, device=dev)
    if R == 0:
        return torch.empty((0, K), dtype=torch.uint16, device=dev), num_bits, objective
    scores, values = level_candidates(mu_t, sg_t, tab_lm, N)
    status = torch.zeros(1, dtype=torch.uint32, device=dev)
    if budgets.numel() == 1:
        num_bits, objective = ops.budget_dp(scores, K, int(budgets[0]), status=status)
    else:
        for b in torch.unique(budgets).tolist():
            rows = torch.nonzero(budgets == b).reshape(-1).to(dev)
            nb, ob = ops.budget_dp(scores[:, rows].contiguous(), K, int(b), status=status)
            num_bits[rows] = nb
            objective[rows] = ob
    idx, _ = _rank_indices(values, num_bits, tab_sorted, C)
    _raise_on_status("quantize_rows_to_budget", status)
    return idx, num_bits, objective


def _rows_args(who, mu, sigma, table, N):
    """The arguments the row calls share, on the current device: (mu f32 [R, K], sigma f32 [R, K], level-major table, sorted
    table, C = code books)."""
    if not torch.cuda.is_available():
        raise VBQError(f"no ROCm device visible: vbq_amd.{who} has no CPU implementation")
    dev = torch.device("cuda", torch.cuda.current_device())
    mu_t = (ops.host_tensor(mu) if not isinstance(mu, torch.Tensor) else mu.detach()).to(dev, torch.float32)
    sg_t = (ops.host_tensor(sigma) if not isinstance(sigma, torch.Tensor) else sigma.detach()).to(dev, torch.float32)
    if mu_t.dim() != 2 or mu_t.shape != sg_t.shape:
        raise ValueError(f"mu and sigma must be [R, K] of one shape, got {tuple(mu_t.shape)} and {tuple(sg_t.shape)}")
    R, K = mu_t.shape
    if K < 1:
        raise ValueError("K must be at least 1")
    T = table_size(N)
    shape = tuple(int(d) for d in np.shape(table))
    if shape not in ((T,), (1, T), (K, T)):
        raise ValueError(f"table must be [{T}] or [{K}, {T}] for N={N}, got {shape}")
    C = K if shape == (K, T) else 1
    tab_lm, tab_sorted = _device_table(table, C, N, dev, True)
    return mu_t.contiguous(), sg_t.contiguous(), tab_lm, tab_sorted, C


def _rank_indices(values, num_bits, tab_sorted, C):
    """num_bits int32 [R, K] -> (rank index uint16 [R, K] of the code point each element chose, the code point f32 [R, K])."""
    chosen = torch.gather(values, 0, num_bits.to(torch.int64)[None])[0]              # [R, K] f32: the code point itself
    if C > 1:
        idx = torch.searchsorted(tab_sorted, chosen.t().contiguous()).t()
    else:
        idx = torch.searchsorted(tab_sorted[0], chosen)
    return idx.to(torch.uint16).contiguous(), chosen


def _raise_on_status(who, status):
    if int(status.cpu().item()) & 1:
        raise VBQError(f"{who}: a score is NaN or +inf (non-finite mu, or sigma that is not positive)")


SWEEP_MAX_BUDGETS = 64                       # budgets of one vbqb_budget_sweep_f64 launch
CURVE_SCRATCH_BYTES = 64 << 20               # embeddings.records_distortion_curve: the f64 curves of one chunk of rows


def _budget_list(total_bits, K: int, N: int):
    import operator
    if isinstance(total_bits, torch.Tensor):
        total_bits = total_bits.cpu().tolist()
    budgets = [operator.index(b) for b in (total_bits.tolist() if isinstance(total_bits, np.ndarray) else total_bits)]
    for b in budgets:
        if not 0 <= b <= K * N:
            raise ValueError(f"budget {b} outside [0, K*N = {K * N}]")
    return budgets


def _sweep_in_order(scores, K: int, budgets, status):
    """ops.budget_dp_sweep for a budget list in any order and with repeats: the distinct values ascending, 64 to a launch,
    the slices back in the caller's order.  -> (bits int32 [S, R, K], objective f64 [S, R])."""
    distinct = sorted(set(budgets))
    bits, obj = [], []
    for i in range(0, max(len(distinct), 1), SWEEP_MAX_BUDGETS):
        b, o, _ = ops.budget_dp_sweep(scores, K, distinct[i:i + SWEEP_MAX_BUDGETS], status=status)
        bits.append(b)
        obj.append(o)
    bits = bits[0] if len(bits) == 1 else torch.cat(bits)
    obj = obj[0] if len(obj) == 1 else torch.cat(obj)
    if budgets == distinct:
        return bits, obj
    order = torch.tensor([distinct.index(b) for b in budgets], dtype=torch.int64, device=bits.device)
    return bits[order], obj[order]


def _rows_sweep(who, mu, sigma, budgets, table, N):
    """-> (idx uint16 [S, R, K], num_bits int32 [S, R, K], objective f64 [S, R], code points f32 [S, R, K])."""
    mu_t, sg_t, tab_lm, tab_sorted, C = _rows_args(who, mu, sigma, table, N)
    dev = mu_t.device
    R, K = mu_t.shape
    budgets = _budget_list(budgets, K, N)
    S = len(budgets)
    if R == 0 or S == 0:
        return (torch.empty((S, R, K), dtype=torch.uint16, device=dev), torch.empty((S, R, K), dtype=torch.int32, device=dev),
                torch.empty((S, R), dtype=torch.float64, device=dev), torch.empty((S, R, K), dtype=torch.float32, device=dev))
    scores, values = level_candidates(mu_t, sg_t, tab_lm, N)
    status = torch.zeros(1, dtype=torch.uint32, device=dev)
    num_bits, objective = _sweep_in_order(scores, K, budgets, status)
    idx = torch.empty((S, R, K), dtype=torch.uint16, device=dev)
    chosen = torch.empty((S, R, K), dtype=torch.float32, device=dev)
    for s in range(S):
        idx[s], chosen[s] = _rank_indices(values, num_bits[s], tab_sorted, C)
    _raise_on_status(who, status)
    return idx, num_bits, objective, chosen


def quantize_rows_to_budgets(mu, sigma, budgets, *, table, N: int = 10):
    """quantize_rows_to_budget at every budget of `budgets` (ints in [0, K * N], any order, repeats allowed) for the price of
    about the largest: the candidates are scored once, the budget DP runs ONE forward pass per 64 distinct budgets
    (ops.budget_dp_sweep) and each budget only walks its own back-pointers.
    Returns device tensors (idx uint16 [S, R, K], num_bits int32 [S, R, K], objective f64 [S, R]); slice s equals
    quantize_rows_to_budget(mu, sigma, budgets[s], table=table, N=N) bit for bit."""
    return _rows_sweep("quantize_rows_to_budgets", mu, sigma, budgets, table, N)[:3]


def budget_curve(mu, sigma, *, table, N: int = 10, max_bits=None):
    """The objective quantize_rows_to_budget reports for every row at EVERY budget: f64 [R, max_bits + 1] on the device, entry
    [r, b] for row r at total_bits = b (max_bits defaults to K * N).  One curve-only forward pass of the budget DP, which keeps
    no back-pointers.  A row's curve need not be monotone in b: the budget is spent exactly."""
    import operator
    mu_t, sg_t, tab_lm, _, _ = _rows_args("budget_curve", mu, sigma, table, N)
    R, K = mu_t.shape
    max_bits = K * N if max_bits is None else operator.index(max_bits)
    if not 0 <= max_bits <= K * N:
        raise ValueError(f"max_bits {max_bits} outside [0, K*N = {K * N}]")
    if R == 0:
        return torch.empty((0, max_bits + 1), dtype=torch.float64, device=mu_t.device)
    scores, _ = level_candidates(mu_t, sg_t, tab_lm, N)
    status = torch.zeros(1, dtype=torch.uint32, device=mu_t.device)
    curve = ops.budget_dp_sweep(scores, K, [], curve_len=max_bits + 1, status=status)[2]
    _raise_on_status("budget_curve", status)
    return curve
