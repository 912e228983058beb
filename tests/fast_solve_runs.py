"""The launches of tests/test_gpu_fast_solve_variants.py, shared with its control driver tools/fast_solve_control.py: the data
of tests/solve_cases.py at one bit depth with the C oracle's answers (computed once, for two channels and 33 lambdas; every
launch takes a slice), the forms a case is passed in, and the comparison.  The caller brings vbq_amd.ops.

Forms (mu, sigma as the call sees them):
    one        1-D, one code book, an odd element count (a half pair at the end)
    cb         planes [2, rows], rows odd: the second plane starts half a pair off, both end in a half pair
    cb-even    planes [2, rows - 1]: whole pairs only
    bc->cb     channel-last in [rows, 2], planes out
    single     one element
    view       1-D, a view that starts one element past a 16-byte boundary
Depths above ten take the first three and `single`, `view` only (planes and one code book)."""
import functools
from collections import namedtuple

import numpy as np
import torch

import launch_plans as LP
import solve_cases as SC
from oracle import c_oracle as CO
from oracle import vbq_oracle as O

F32 = np.float32
L_MAX = 33                                  # one lambda past a chunk: the second chunk is a one-lambda call
ROWS = {"dyadic": 2001, "near_midpoint": 1001, "edge": 301, "certificate_edge": 1001}
FORMS = ("one", "cb", "cb-even", "bc->cb", "single", "view")

Data = namedtuple("Data", "name lengths N tab mu sg lam level_len idx zhat bits")
"""One family at one depth: tab [2, T], mu, sg [rows, 2], L_MAX lambdas, level_len None or [L_MAX, 2, N + 1]; idx, zhat, bits
[L_MAX, rows, 2] from oracle.c_oracle.quantize(mode=0)."""


def forms(N):
    return tuple(f for f in FORMS if N <= 10 or f != "bc->cb")


@functools.lru_cache(maxsize=None)
def data(N):
    """The eight data sets of depth N: dyadic (raw / caller lengths), near mid-points of levels N // 2 and N (their caller
    table), edge (raw / caller lengths), the same mid-points with spread sigmas (the certificate's edge)."""
    dy = SC.with_lambdas(SC.dyadic_case(N, rows=ROWS["dyadic"], C=2), L_MAX)
    ed = SC.with_lambdas(SC.edge_case(N, rows=ROWS["edge"], C=2), L_MAX)
    cases = [(dy, "raw"), (dy._replace(level_len=SC.dyadic_level_len(N, L_MAX, 2)), "caller"),
             (SC.with_lambdas(SC.near_midpoint_case(N, N // 2, rows=ROWS["near_midpoint"], C=2), L_MAX), "caller"),
             (SC.with_lambdas(SC.near_midpoint_case(N, N, rows=ROWS["near_midpoint"], C=2), L_MAX), "caller"),
             (ed, "raw"), (ed._replace(level_len=SC.edge_level_len(N, L_MAX, 2)), "caller"),
             (SC.with_lambdas(SC.certificate_edge_case(N, N // 2, rows=ROWS["certificate_edge"], C=2), L_MAX), "caller"),
             (SC.with_lambdas(SC.certificate_edge_case(N, N, rows=ROWS["certificate_edge"], C=2), L_MAX), "caller")]
    out = []
    for case, lengths in cases:
        assert (case.level_len is None) == (lengths == "raw") and len(case.lam) == L_MAX
        idx, zh, bt = CO.quantize(case.mu, case.sg, case.tab, case.lam, N=N, level_len=case.level_len, mode=0, want_zhat=True,
                                  want_bits=True, threads=8)
        for a in (idx, zh, bt, case.mu, case.sg, case.tab):
            a.setflags(write=False)                       # shared among the tests: nobody changes it
        out.append(Data(case.name, lengths, N, case.tab, case.mu, case.sg, case.lam, case.level_len, idx, zh, bt))
    return out


def dev(a):
    return torch.as_tensor(np.array(a, order="C")).cuda()        # a copy: the shared arrays are read-only


def _shifted(a):
    """A device view of the 1-D array that starts one element past a 16-byte boundary."""
    t = dev(np.concatenate([[F32(7)], a]))[1:]
    assert t.data_ptr() % 16 == 4
    return t


def inputs(d, form):
    """-> (mu, sigma, table, layout argument, n_ch, row slice, channel slice) of `form`, host arrays except for `view`."""
    rows = d.mu.shape[0]
    if form in ("one", "single", "view"):
        r = slice(0, 1) if form == "single" else slice(0, rows)
        m, s = d.mu[r, 0], d.sg[r, 0]
        return m, s, d.tab[:1], "bc", 1, r, slice(0, 1)
    r = slice(0, rows - 1) if form == "cb-even" else slice(0, rows)
    if form == "bc->cb":
        return d.mu[r], d.sg[r], d.tab, "bc->cb", 2, r, slice(0, 2)
    return d.mu[r].T, d.sg[r].T, d.tab, "cb", 2, r, slice(0, 2)


def _level_len(d, L, ch):
    return None if d.level_len is None else np.ascontiguousarray(d.level_len[:L, ch])


def plan(d, L, form, **kw):
    """The kernels launch_quantize takes for the first L lambdas of d in `form`, chunk by chunk."""
    m, _, _, layout, n_ch, _, _ = inputs(d, form)
    return LP.solve_kernels(d.N, d.lam[:L], layout, n_ch, level_len=d.level_len is not None, elements=int(np.size(m)), **kw)


def _planes(a, form):
    """A per-element output as [L, rows, channels]."""
    if form in ("one", "single", "view"):
        return a[:, :, None]
    return a.transpose(0, 2, 1)


def quantize(ops, d, L, form, want_zhat=False, want_bits=False):
    """ops.quantize on the first L lambdas -> (idx, zhat | None, bits | None), each [L, rows, channels]."""
    m, s, tab, layout, n_ch, _, ch = inputs(d, form)
    m, s = (_shifted(m), _shifted(s)) if form == "view" else (dev(m), dev(s))
    ll = _level_len(d, L, ch)
    out = ops.quantize(m, s, dev(tab), d.lam[:L], N=d.N, layout=layout, level_len=None if ll is None else dev(ll),
                       want_zhat=want_zhat, want_bits=want_bits)
    out = [_planes(t.cpu().numpy(), form) for t in (out if isinstance(out, tuple) else (out,))]
    return out[0], (out[1] if want_zhat else None), (out[-1] if want_bits else None)


def expected(d, L, form):
    """The oracle's (idx, zhat, bits) for the same launch."""
    _, _, _, _, _, r, ch = inputs(d, form)
    return tuple(a[:L, r, ch] for a in (d.idx, d.zhat, d.bits))


def level_counts(ops, d, L, form):
    m, s, tab, layout, n_ch, _, ch = inputs(d, form)
    m, s = (_shifted(m), _shifted(s)) if form == "view" else (dev(m), dev(s))
    ll = _level_len(d, L, ch)
    got = ops.level_counts(m, s, dev(tab), d.lam[:L], N=d.N, layout=layout, level_len=None if ll is None else dev(ll))
    return got.cpu().numpy()


def expected_counts(d, L, form):
    """np.bincount of the oracle's levels -> [L, channels, N + 1]."""
    idx = expected(d, L, form)[0]
    lev = O.levels_of_sorted_ranks(d.N)[idx]
    return np.stack([[np.bincount(lev[l, :, c], minlength=d.N + 1) for c in range(idx.shape[2])] for l in range(L)])


def bit_equal(a, b):
    """Equal as bit patterns (f32 outputs: -0.0 and 0.0 differ, as they would in a file)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == F32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return a.shape == b.shape and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ the launches, by instance
INDEX_L = (5, L_MAX)            # K1<0>
OUTPUT_L = (1, 4, L_MAX)        # K1<1>
COUNT_L = (8, L_MAX)            # K1<2>
PRUNED_L = (1, 2, 3, 4)         # K1p<1>, K1p<2>; three and four lambdas are K1<0>'s (kPrunedMaxL)


def index_plan(L):
    return ["K1<0>"] * (L // LP.MAX_LAMBDA_CHUNK) + ([f"K1p<{L % 32}>"] if 1 <= L % 32 <= LP.PRUNED_MAX_L else
                                                     (["K1<0>"] if L % 32 else []))


def output_plan(L):
    return ["K1<1>"] * LP.cdiv(L, LP.MAX_LAMBDA_CHUNK)


def count_plan(L):
    return ["K1<2>"] * LP.cdiv(L, LP.MAX_LAMBDA_CHUNK)


def pruned_plan(L):
    return [f"K1p<{L}>" if L <= LP.PRUNED_MAX_L else "K1<0>"]
