"""Exact one-dimensional k-means of many channels on the device (include/vbq_kmeans.h, vbq_amd/kmeans).

On sorted samples the optimal clusters of 1-D k-means are contiguous segments, and a dynamic programme over (number of
clusters, prefix length) finds the GLOBAL optimum: no Lloyd iteration, no seed.  The recurrence does not depend on the level
count it is run for, so one pass at the largest count answers every smaller one: all level counts of all channels are one
launch.

    prefix_sums(samples)                  the kernel's inputs: sorted samples, shift (upper median), S1, S2 -- device tensors
    fit_channels(samples, levels)         per level: code points f64 [C, k], counts int64 [C, k], code lengths f64 [C, k]
    sse_curve(samples, Kmax)              the optimal within-cluster sum of squares at every level count 1..Kmax, f64 [C, Kmax]
    kmeans1d_dp / nearest_code_channels   the two C calls on device tensors

There is no CPU implementation: without a ROCm device every function raises."""
from __future__ import annotations

import collections
import ctypes as C
import operator
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib_kmeans, ops
from .ops import _dev, _ptr, _stream

MAX_LEVELS_PER_LAUNCH = 64
MAX_LEVEL_COUNT = 1024
WORKSPACE_CAP_BYTES = 4 << 30
"""What fit_channels allocates at most for the back-pointers (never less than one channel's slice): with fewer slices than
channels the workgroups take the channels in rounds."""

LevelFit = collections.namedtuple("LevelFit", "code_points counts code_lengths")


def _samples_2d(samples, who):
    """[B, C] float32 on the current device, from a host array or a tensor on any device."""
    dev = ops.current_device(who)
    dt = samples.dtype if isinstance(samples, (torch.Tensor, np.ndarray)) else np.asarray(samples).dtype
    if dt in (torch.float64, np.float64) and not isinstance(samples, (list, tuple)):
        raise ValueError("float64 samples are not supported: the comparison quantizers run in float32, the dtype of the "
                         "latents they are applied to (cast explicitly if f32 binning is what you want)")
    x = ops.upload(samples if isinstance(samples, torch.Tensor) else np.asarray(samples, dtype=np.float32), dev, torch.float32)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"expected samples of shape [B, C] with B, C >= 1, got {tuple(x.shape)}")
    return x


def _shape_2d(samples):
    shape = tuple(samples.shape) if isinstance(samples, (torch.Tensor, np.ndarray)) else np.shape(samples)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"expected samples of shape [B, C] with B, C >= 1, got {tuple(shape)}")
    return int(shape[0]), int(shape[1])


def _level_list(levels, n):
    """The caller's level counts as Python ints, checked: each in [1, min(n, 1024)]."""
    levels = [operator.index(k) for k in (levels.tolist() if isinstance(levels, (torch.Tensor, np.ndarray)) else levels)]
    if not levels:
        raise ValueError("no level counts given")
    for k in levels:
        if k < 1 or k > MAX_LEVEL_COUNT:
            raise ValueError(f"level count {k} outside [1, {MAX_LEVEL_COUNT}]")
        if k > n:
            raise ValueError(f"n_samples={n} should be >= n_clusters={k}.")                # sklearn's refusal, in its words
    return levels


def prefix_sums(samples):
    """samples [B, C] -> (sorted f32 [C, B], shift f64 [C], S1 f64 [C, B + 1], S2 f64 [C, B + 1]) on the device: every channel
    sorted ascending, shift = its upper median sorted[B // 2], y = f64(sorted) - shift, S1 / S2 = 0 followed by the running sums
    of y / y * y.  torch.sort, one cast, one subtraction, torch.cumsum in float64."""
    x = _samples_2d(samples, "vbq_amd.kmeans1d")
    B, Cn = x.shape
    xs = torch.sort(x.t().contiguous(), dim=1).values
    shift = xs[:, B // 2].to(torch.float64).contiguous()
    y = xs.to(torch.float64) - shift[:, None]
    if Cn == 1:
        # torch scans a tensor that is one row with another kernel (another order of additions) than the rows of a matrix:
        # a single channel is summed as two equal rows, so that a channel's sums do not depend on how many are fitted with it
        y = y.expand(2, B).contiguous()
    S1 = torch.zeros((Cn, B + 1), dtype=torch.float64, device=x.device)
    S2 = torch.zeros((Cn, B + 1), dtype=torch.float64, device=x.device)
    S1[:, 1:] = torch.cumsum(y, dim=1)[:Cn]
    S2[:, 1:] = torch.cumsum(y * y, dim=1)[:Cn]
    return xs, shift, S1, S2


def kmeans1d_dp(S1: torch.Tensor, S2: torch.Tensor, shift: torch.Tensor, levels: Sequence[int], *,
                status: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """vbqk_kmeans1d_f64 on prefix sums S1, S2 (f64 [C, n + 1]) and shift (f64 [C]); `levels` strictly ascending ints, at most 64,
    the largest at most min(n, 1024).  Returns (starts, codes, counts, sse): three lists with one entry per level -- int32 /
    float64 / int64 [C, k] views of the packed outputs -- and sse f64 [C, Kmax] with sse[c, q - 1] the optimum with q levels.
    `status` (uint32 [1], zeroed by the caller) gets bit 0 set when a channel held a NaN or an infinity; `workspace` (uint8)
    replaces the one this call would allocate and may be smaller (more rounds)."""
    S1 = _dev(S1, torch.float64, "S1")
    S2 = _dev(S2, torch.float64, "S2")
    shift = _dev(shift, torch.float64, "shift")
    if S1.dim() != 2 or S1.shape != S2.shape or S1.shape[1] < 2 or tuple(shift.shape) != (S1.shape[0],):
        raise ValueError(f"expected S1, S2 of shape [C, n + 1] and shift of shape [C], got {tuple(S1.shape)}, {tuple(S2.shape)}, "
                         f"{tuple(shift.shape)}")
    Cn, n = S1.shape[0], S1.shape[1] - 1
    levels = [operator.index(k) for k in levels]
    S = len(levels)
    if any(not -(1 << 31) <= k < (1 << 31) for k in levels):
        raise ValueError(f"levels {levels} outside the int32 range")
    total = Cn * sum(max(k, 0) for k in levels)
    Kmax = max(levels[-1], 1) if levels else 1
    dev = S1.device
    starts = torch.empty(total, dtype=torch.int32, device=dev)
    codes = torch.empty(total, dtype=torch.float64, device=dev)
    counts = torch.empty(total, dtype=torch.int64, device=dev)
    sse = torch.empty((Cn, Kmax), dtype=torch.float64, device=dev)
    reads = (("S1", S1), ("S2", S2), ("shift", shift))
    if status is not None:
        status = ops._status(status, 1, dev, reads)
    h = _lib_kmeans.lib()
    if workspace is None:
        wsb = h.vbqk_kmeans1d_workspace_bytes(n, Cn, Kmax)
        one = h.vbqk_kmeans1d_workspace_bytes(n, 1, Kmax)
        if wsb > WORKSPACE_CAP_BYTES and one:
            wsb = max(one, WORKSPACE_CAP_BYTES // one * one)
        workspace = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
    else:
        workspace = ops._workspace(workspace, 1, dev, 0, reads + (("status", status),))
    wsb = workspace.numel() if workspace is not None else 0
    _lib_kmeans.check(h.vbqk_kmeans1d_f64(_ptr(S1), _ptr(S2), _ptr(shift), n, Cn, (C.c_int32 * S)(*levels), S, _ptr(starts),
                                          _ptr(codes), _ptr(counts), _ptr(sse), _ptr(status), _ptr(workspace), wsb, _stream(S1)),
                      "vbqk_kmeans1d_f64")
    out, at = ([], [], []), 0
    for k in levels:
        for lst, flat in zip(out, (starts, codes, counts)):
            lst.append(flat[at:at + Cn * k].view(Cn, k))
        at += Cn * k
    return out[0], out[1], out[2], sse


def nearest_code_channels(x: torch.Tensor, codes: torch.Tensor, *, counts: Optional[torch.Tensor] = None):
    """vbqk_nearest_code_channels_f64: x f32 [B, C] channel-last, codes f64 [C, k] -> (index int32 [B, C], value f64 [B, C]), per
    channel what vbq_nearest_code_f64 gives for that column and code row; `counts` (int64 [C, k]) is added to."""
    x = _dev(x, torch.float32, "x")
    codes = _dev(codes, torch.float64, "codes")
    if x.dim() != 2 or codes.dim() != 2 or codes.shape[0] != x.shape[1]:
        raise ValueError(f"expected x [B, C] and codes [C, k], got {tuple(x.shape)} and {tuple(codes.shape)}")
    B, Cn = x.shape
    k = codes.shape[1]
    if counts is not None:
        counts = ops._out(counts, (Cn, k), torch.int64, x.device, "counts", True, (("x", x), ("codes", codes)))
    I = torch.empty((B, Cn), dtype=torch.int32, device=x.device)
    q = torch.empty((B, Cn), dtype=torch.float64, device=x.device)
    _lib_kmeans.check(_lib_kmeans.lib().vbqk_nearest_code_channels_f64(_ptr(x), B, Cn, _ptr(codes), k, _ptr(I), _ptr(q),
                                                                        _ptr(counts), _stream(x)),
                      "vbqk_nearest_code_channels_f64")
    return I, q


def _fit_in_order(S1, S2, shift, levels, status):
    """kmeans1d_dp for any list of level counts: the distinct values ascending, at most 64 per launch, and the answers in the
    caller's order (a repeated level gets the same tensors).  -> ([codes f64 [C, k]], [counts int64 [C, k]]) per entry."""
    distinct = sorted(set(levels))
    codes, counts = {}, {}
    for at in range(0, len(distinct), MAX_LEVELS_PER_LAUNCH):
        chunk = distinct[at:at + MAX_LEVELS_PER_LAUNCH]
        _, cd, ct, _ = kmeans1d_dp(S1, S2, shift, chunk, status=status)
        codes.update(zip(chunk, cd))
        counts.update(zip(chunk, ct))
    return [codes[k] for k in levels], [counts[k] for k in levels]


def _require_clean(status):
    if int(status.cpu().item()) & 1:
        raise ValueError("samples must not contain infs or NaNs")


def fit_channels(samples, levels, add_n_smoothing=1.0):
    """The globally optimal k-means code book of every channel of samples [B, C] (host or device, float32) at every level
    count of `levels` (any order, repeats allowed; each at most min(B, 1024)).  -> a list with one LevelFit per entry of
    `levels`: code_points f64 [C, k] ascending, counts int64 [C, k], code_lengths f64 [C, k] = -log2(counts / B), smoothed by
    add_n_smoothing only where a channel has an empty cluster (the reference's rule; an optimal segment is never empty).
    NumPy arrays."""
    from .baselines import _code_lengths
    B, _ = _shape_2d(samples)
    levels = _level_list(levels, B)
    _, shift, S1, S2 = prefix_sums(samples)
    status = torch.zeros(1, dtype=torch.uint32, device=S1.device)
    codes, counts = _fit_in_order(S1, S2, shift, levels, status)
    _require_clean(status)
    fits = []
    for cd, ct in zip(codes, counts):
        ct = ct.cpu().numpy()
        fits.append(LevelFit(cd.cpu().numpy(), ct, np.array([_code_lengths(row, B, add_n_smoothing) for row in ct])))
    return fits


def sse_curve(samples, Kmax):
    """-> f64 [C, Kmax] (NumPy): entry [c, q - 1] is the smallest within-cluster sum of squares any q code points reach on
    channel c of samples [B, C]."""
    B, _ = _shape_2d(samples)
    Kmax = _level_list([Kmax], B)[0]
    _, shift, S1, S2 = prefix_sums(samples)
    status = torch.zeros(1, dtype=torch.uint32, device=S1.device)
    sse = kmeans1d_dp(S1, S2, shift, [Kmax], status=status)[3]
    _require_clean(status)
    return sse.cpu().numpy()
