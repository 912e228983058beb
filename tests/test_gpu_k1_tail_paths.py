"""The end of K1's lambda loop (k_quant_fast, vbq_quantize_fast.hip) bit for bit against the C oracle: the tie test that counts
the two elements of a lane together, the rank pair packed from the low halves of the two LDS words, the full-pair store
through a buffer descriptor and the short stores of a half pair, at row counts around one pair and one workgroup iteration.

Three channels of 513 rows at every depth, a caller length table, three lambdas (K1<0>; two or fewer are K1p's):
    0   dyadic data (tests/solve_cases.py) arranged in pairs: a cross-level tie on the even element only, on the odd one only,
        on both, on neither, in turn -- the merged flag re-solves both elements of a pair;
    1   the same arrangement one pair further on, so that a launch of one, two or three rows sees other kinds;
    2   mu one ulp above a mid-point of the deepest level, which alone is cheap: the right side is better by less than an ulp
        of the cost (the unchanged certificate), and every rank needs all N + 1 bits of its half word.
Every launch takes the first `rows` rows: one code book (each channel by itself) and planes.  The library reads its literal-scan
switch from the environment once per process, so that form is the variant suite's (tests/test_gpu_fast_solve_variants.py)."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import launch_plans as LP
import solve_cases as SC
from fast_solve_runs import bit_equal, dev
from oracle import c_oracle as CO
from oracle import vbq_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LAM = [2.0 ** -3, 1.0, 8.0]
ROWS = (1, 2, 3, 511, 512, 513)
MAX_ROWS = max(ROWS)
DEPTHS = (4, 10, 12)
KINDS = ((True, False), (False, True), (True, True), (False, False))       # (even element ties, odd element ties) of a pair


@pytest.fixture(scope="module")
def ops():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    from vbq_amd import ops as _ops
    return _ops


def _pairs(tie_rows, clean_rows, first_kind):
    """Row numbers of the pool for MAX_ROWS rows whose pairs run through KINDS from `first_kind` on."""
    t, c, out = 0, 0, []
    for r in range(MAX_ROWS + 1):
        wants_tie = KINDS[(r // 2 + first_kind) % 4][r % 2]
        if wants_tie:
            out.append(tie_rows[t % len(tie_rows)])
            t += 1
        else:
            out.append(clean_rows[c % len(clean_rows)])
            c += 1
    return np.array(out[:MAX_ROWS])


@functools.lru_cache(maxsize=None)
def data(N):
    """-> (tab [3, T], mu, sg [513, 3], level_len [3, 3, N + 1], the oracle's idx, zhat, bits [3, 513, 3], multi [3, 513, 3])."""
    ll_dy = SC.dyadic_level_len(N, len(LAM), 1)
    pool = SC.dyadic_case(N, rows=2000, C=1)._replace(lam=LAM, level_len=ll_dy)
    ev = SC.restate(pool)
    tie = np.flatnonzero(ev.multi.any(axis=0)[:, 0])
    clean = np.flatnonzero(~(ev.multi | ev.b_flag).any(axis=0)[:, 0])
    assert len(tie) >= 8 and len(clean) >= 20, (len(tie), len(clean))        # the arrangement cycles through them
    mid = SC.near_midpoint_case(N, N, rows=MAX_ROWS, C=1)
    ll_mid = np.repeat(mid.level_len[:1], len(LAM), axis=0)
    cols = [(pool.tab, pool.mu[_pairs(tie, clean, 0)], pool.sg[_pairs(tie, clean, 0)], ll_dy),
            (pool.tab, pool.mu[_pairs(tie, clean, 1)], pool.sg[_pairs(tie, clean, 1)], ll_dy),
            (mid.tab, mid.mu, mid.sg, ll_mid)]
    tab = np.concatenate([c[0] for c in cols], axis=0)
    mu = np.concatenate([c[1] for c in cols], axis=1)
    sg = np.concatenate([c[2] for c in cols], axis=1)
    ll = np.ascontiguousarray(np.concatenate([c[3] for c in cols], axis=1))
    case = SC.Case("k1-tail", N, tab, mu, sg, LAM, ll)
    ev = SC.restate(case)
    # what the arrangement is for: every kind of pair at one lambda, and the certificate's event on the third channel
    m = ev.multi[:, :MAX_ROWS - 1, 0]
    even, odd = m[:, 0::2], m[:, 1::2]
    assert (even & ~odd).any() and (~even & odd).any() and (even & odd).any() and (~even & ~odd).any()
    assert ev.b_flag[:, :, 2].any() and ev.b_merged[:, :, 2].any()
    assert ev.multi[:, 0, 0].any() and not ev.multi[:, 0, 1].any()          # the one-row launches: a tie, and none
    idx, zh, bt = CO.quantize(mu, sg, tab, LAM, N=N, level_len=ll, mode=0, want_zhat=True, want_bits=True, threads=8)
    assert idx[:, :, 2].max() >= 2 ** N                                     # a rank that needs bit N
    for a in (tab, mu, sg, ll, idx, zh, bt):
        a.setflags(write=False)
    return tab, mu, sg, ll, idx, zh, bt, ev.multi


def _launch(ops, N, rows, chans, **kw):
    """ops.quantize on the first `rows` rows of channels `chans` -> outputs as [L, rows, len(chans)] each."""
    tab, mu, sg, ll = data(N)[:4]
    ch = list(chans)
    lld = dev(ll[:, ch])
    if len(ch) == 1:
        assert LP.solve_kernels(N, LAM, "bc", 1, level_len=True, elements=rows, **kw) == ["K1<1>" if kw else "K1<0>"]
        out = ops.quantize(dev(mu[:rows, ch[0]]), dev(sg[:rows, ch[0]]), dev(tab[ch]), LAM, N=N, level_len=lld, **kw)
        out = out if isinstance(out, tuple) else (out,)
        return [t.cpu().numpy()[:, :, None] for t in out]
    out = ops.quantize(dev(mu[:rows, ch].T), dev(sg[:rows, ch].T), dev(tab[ch]), LAM, N=N, layout="cb", level_len=lld, **kw)
    out = out if isinstance(out, tuple) else (out,)
    return [t.cpu().numpy().transpose(0, 2, 1) for t in out]


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("N", DEPTHS)
def test_indices_at_the_pair_and_iteration_boundaries(ops, N, C):
    """K1<0>: the perm-packed pair through the buffer descriptor (whole pairs: 2, 512 rows; 512 = one workgroup iteration of 256
    lanes), the short stores of a half pair (1, 3, 511, 513 rows; planes of an odd row count store short everywhere)."""
    want = data(N)[4]
    for rows in ROWS:
        for chans in ([(0, 1, 2)] if C == 3 else [(0,), (1,), (2,)]):
            got = _launch(ops, N, rows, chans)[0]
            w = want[:, :rows, list(chans)]
            bad = np.argwhere(got != w)
            assert got.dtype == np.uint16 and bit_equal(got, w), (N, rows, chans, len(bad), bad[:5].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("N", DEPTHS)
def test_outputs_and_level_counts_share_the_merged_flag(ops, N):
    """K1<1> (Z_hat and lengths beside the indices) and K1<2> (levels counted, caller lengths) take the same merged tie flag."""
    tab, mu, sg, ll, idx, zh, bt, _ = data(N)
    lev = O.levels_of_sorted_ranks(N)
    for rows in (3, 512, 513):
        for chans in ((0, 1, 2), (1,)):
            ch = list(chans)
            got = _launch(ops, N, rows, chans, want_zhat=True, want_bits=True)
            for g, w, name in zip(got, (idx, zh, bt), ("idx", "zhat", "bits")):
                assert bit_equal(g, w[:, :rows, ch]), (N, rows, chans, name)
            m, s = (dev(mu[:rows, ch].T), dev(sg[:rows, ch].T)) if len(ch) > 1 else (dev(mu[:rows, ch[0]]), dev(sg[:rows, ch[0]]))
            cnt = ops.level_counts(m, s, dev(tab[ch]), LAM, N=N, layout="cb" if len(ch) > 1 else "bc", level_len=dev(ll[:, ch]))
            want = np.stack([[np.bincount(lev[idx[l, :rows, c]], minlength=N + 1) for c in ch] for l in range(len(LAM))])
            assert np.array_equal(cnt.cpu().numpy(), want), (N, rows, chans)


def test_all_planes_within_4gb_decision_at_its_boundaries(tmp_path):
    """The launchers' choice of the buffer-descriptor store, a pure host function (vbq_amd/csrc/vbq_index_planes.h), at its
    boundary values: a stand-alone C++ program (tests/host/index_planes_check.cpp) under the address and undefined-behaviour
    sanitizers, nothing allocated, no GPU."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "index_planes_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "vbq_amd", "csrc"), os.path.join(ROOT, "tests", "host", "index_planes_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "compiling the check failed:\n" + r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, f"index_planes_check exited with {r.returncode}:\n" + r.stderr[-4000:]
    assert r.stderr == "", "the sanitizers or the check wrote:\n" + r.stderr[-4000:]
