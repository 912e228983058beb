"""Float64 reference for the BMSHJ2018 prior (img-compression/learned_prior.py), test-only.

It works on the same float32 EFFECTIVE parameters the K4 kernels read ([C, 43] in the order of
vbq_amd.priors.pack_bmshj_params: per layer the row-major matrix, the bias and, for layers 0-2,
the factor), widened to float64:

    cdf64(params, x)        sigmoid of the logits chain of learned_prior.py:88-107
    pdf64(params, x)        d cdf64 / dx by torch autograd -- NOT the analytic Jacobian chain
                            (learned_prior.py:277-321) that both the kernels and the float32
                            NumPy restatement (vbq_oracle.BMSHJ2018Oracle) use
    root64(params, xi)      the float64 root of cdf64(z) = xi by bisection
    nll_grad64(params, x)   per channel sum(-log(pdf + 1e-10)) and its gradient with respect
                            to the 43 effective parameters (the [C, 44] layout of
                            ops.bmshj_nll_grad), plus sum_i |d l_i / d theta| per parameter

Every function runs on the device of its torch inputs (NumPy inputs run on the CPU).
"""
from __future__ import annotations

import numpy as np
import torch

NP = 43
DIMS = (1, 3, 3, 3, 1)
F64 = torch.float64


def _t(a, device=None):
    if isinstance(a, torch.Tensor):
        return a.to(device if device is not None else a.device, F64)
    return torch.as_tensor(np.asarray(a, dtype=np.float64), device=device)


def logits64(P, x):
    """learned_prior.py:88-107.  P: [..., 43] f64, broadcastable against x[..., None]; x: f64."""
    h, o = [x], 0
    for i in range(4):
        d, r = DIMS[i], DIMS[i + 1]
        M = [[P[..., o + k * d + j] for j in range(d)] for k in range(r)]
        o += r * d
        b = [P[..., o + k] for k in range(r)]
        o += r
        f = None
        if i < 3:
            f = [P[..., o + k] for k in range(r)]
            o += r
        hn = []
        for k in range(r):
            a = b[k]
            for j in range(d):
                a = a + M[k][j] * h[j]                                # matmul(matrix, logits) (:94)
            if f is not None:
                a = a + f[k] * torch.tanh(a)                          # (:105)
            hn.append(a)
        h = hn
    return h[0]


def cdf64(params, x):
    """cdf of x [..., C] under params [C, 43]; returns an f64 tensor on x's device."""
    xt = _t(x)
    return torch.sigmoid(logits64(_t(params, xt.device), xt))


def pdf64(params, x, chunk=1 << 22):
    """d cdf / dx by autograd of cdf64 (every element depends on its own x only)."""
    xt = _t(x)
    P = _t(params, xt.device)
    flat = xt.reshape(-1, xt.shape[-1])
    out = torch.empty_like(flat)
    step = max(1, chunk // flat.shape[1])
    for r0 in range(0, flat.shape[0], step):
        xx = flat[r0:r0 + step].clone().requires_grad_(True)
        with torch.enable_grad():
            c = torch.sigmoid(logits64(P, xx))
            g, = torch.autograd.grad(c.sum(), xx)
        out[r0:r0 + step] = g
    return out.reshape(xt.shape)


def root64(params, xi, iters=200):
    """z with cdf64(z) = xi, per element of xi [..., C] (every xi in (0, 1)): per-element bracket
    doubling from [-1, 1], then bisection until the bracket stops shrinking in f64."""
    xt = _t(xi)
    P = _t(params, xt.device)
    if not bool(((xt > 0) & (xt < 1)).all()):
        raise ValueError("root64: xi must lie in (0, 1)")
    lo = torch.full_like(xt, -1.0)
    hi = torch.full_like(xt, 1.0)
    for _ in range(1100):
        bad = torch.sigmoid(logits64(P, lo)) >= xt
        if not bool(bad.any()):
            break
        lo = torch.where(bad, lo * 2, lo)
    for _ in range(1100):
        bad = torch.sigmoid(logits64(P, hi)) <= xt
        if not bool(bad.any()):
            break
        hi = torch.where(bad, hi * 2, hi)
    if not bool(torch.isfinite(lo).all() and torch.isfinite(hi).all()):
        raise ValueError("root64: the cdf does not cross xi")
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        below = torch.sigmoid(logits64(P, mid)) < xt
        lo_n = torch.where(below, mid, lo)
        hi_n = torch.where(below, hi, mid)
        if torch.equal(lo_n, lo) and torch.equal(hi_n, hi):
            break
        lo, hi = lo_n, hi_n
    return 0.5 * (lo + hi)


def pdf_max64(params, x=None, n=4097):
    """Per-channel max of pdf64 over a dense grid between the 1e-4 and 1 - 1e-4 quantiles (and
    over x [..., C], if given): the scale of the pdf bound."""
    P = _t(params, x.device if isinstance(x, torch.Tensor) else None)
    C = P.shape[0]
    q = root64(P, torch.tensor([[1e-4] * C, [1 - 1e-4] * C], dtype=F64, device=P.device))
    u = torch.linspace(0, 1, n, dtype=F64, device=P.device)[:, None]
    grid = q[0] + (q[1] - q[0]) * u
    m = pdf64(P, grid).amax(dim=0)
    if x is not None:
        m = torch.maximum(m, pdf64(P, _t(x, P.device)).reshape(-1, C).amax(dim=0))
    return m


def nll_grad64(params, x_cb, chunk=1 << 21):
    """params [C, 43] (f32 values), x_cb [C, n] channel-major planes.  Returns (out, absg), both
    f64 [C, 44] on x_cb's device: out[:, :43] = d(sum_i l_i)/d theta and out[:, 43] = sum_i l_i with
    l_i = -log(pdf64(x_i) + 1e-10); absg[:, :43] = sum_i |d l_i / d theta| and absg[:, 43] =
    sum_i |l_i|.  The parameters are broadcast to one leaf copy per element, so a single backward
    pass yields every per-element gradient."""
    x = _t(x_cb)
    P = _t(params, x.device)
    C, n = x.shape
    out = torch.zeros((C, NP + 1), dtype=F64, device=x.device)
    absg = torch.zeros_like(out)
    step = max(1, chunk // C)
    for j0 in range(0, n, step):
        xs = x[:, j0:j0 + step]
        m = xs.shape[1]
        with torch.enable_grad():
            Pe = P[:, None, :].expand(C, m, NP).clone().requires_grad_(True)
            xx = xs.clone().requires_grad_(True)
            c = torch.sigmoid(logits64(Pe, xx))
            pdf, = torch.autograd.grad(c.sum(), xx, create_graph=True)
            li = -torch.log(pdf + 1e-10)
            ge, = torch.autograd.grad(li.sum(), Pe)
        li = li.detach()
        out[:, :NP] += ge.sum(dim=1)
        out[:, NP] += li.sum(dim=1)
        absg[:, :NP] += ge.abs().sum(dim=1)
        absg[:, NP] += li.abs().sum(dim=1)
    return out, absg


def pack64(matrices, biases, factors):
    """pack_bmshj_params for f64 torch tensors (keeps the autograd graph): [C, 43]."""
    C = matrices[0].shape[0]
    parts = []
    for i in range(4):
        parts += [matrices[i].reshape(C, -1), biases[i].reshape(C, -1)]
        if i < 3:
            parts.append(factors[i].reshape(C, -1))
    return torch.cat(parts, dim=1)
