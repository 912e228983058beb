"""Every instance of the fast f32 solve (vbq_quantize_fast.hip) at every bit depth it is built for, N = 4 .. 12, on data that
reaches the two events it has to flag: k_quant_fast<N, 0 | 1 | 2> (K1: indices; indices with Z_hat / lengths; level counts)
and k_quant_pruned<N, 1 | 2> (K1p).  Every comparison is bit for bit with the C oracle (oracle.c_oracle.quantize, mode 0):
indices, Z_hat and lengths, level counts against np.bincount of the oracle's levels; on a subset of 6000 solves the winners'
scores also equal the exhaustive maximum over every code point (oracle/rd_f64.py).

Before every launch tests/launch_plans.solve_kernel says which kernel the call takes, and the test asserts that it is the
instance the case is named after.  Three things follow from the dispatch and are asserted rather than assumed:
  * k_quant_pruned is built for one and two lambdas only: launch_quant_pruned hands calls with more than
    kPrunedMaxL = 2 lambdas on, and indices-only calls with three or four lambdas take k_quant_fast<N, 0>.  They are run
    here all the same -- as K1<0> launches with three and four lambdas.
  * at N = 10 a raw-length counting call with an eligible sweep takes K1t and a raw-length indices-only sweep of 16 or
    more distinct lambdas K1e, which have their own tests; the sweeps here repeat their eight lambdas up to 33, so K1e is
    never taken, and K1t takes only the eight edge lambdas on their own (that launch is left out; the dyadic eight span
    more than its 16 octaves) and the 33rd lambda, a chunk of its own (the launch stays for its first 32).
  * depths above ten take planes and one code book only.

Data (tests/solve_cases.py; tests/test_solve_cases_host.py proves on the CPU that they reach the events at every depth):
dyadic tables with cross-level ties, mu one ulp off the mid-point of two neighbours under a length table that makes their
level win (sigma = 1, and sigmas that put dL - dR right at the tie certificate's bound), and the edge data of
test_gpu_literal_solve.py; raw lengths and caller tables; the forms of
tests/fast_solve_runs.py (one code book, planes of odd and even length with two different tables, channel-last in, one
element, a view one element past a 16-byte boundary).  Largest launch: 2001 x 2 elements, 33 lambdas.

test_flags_are_what_keeps_the_fast_solve_exact is the control: the same launches in child processes (VBQ_FAST_DEBUG is read
once per process) with every solve forced through the literal scan (still exact, K1p included: its `dbg` argument knows
this value only) and with the flags off (K1<0> and K1<1> then miss the oracle on the near-mid-point data, K1<2> on the
dyadic data, at all nine depths; K1p makes the reference's own comparisons, has no flag to switch off and stays exact)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fast_solve_runs as FR
import launch_plans as LP
import solve_cases as SC
from oracle import rd_f64 as R

pytestmark = pytest.mark.gpu
DEPTHS = SC.DEPTHS


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    from vbq_amd import ops as _ops
    t0 = time.perf_counter()
    yield _ops
    print(f"\n[test_gpu_fast_solve_variants] {time.perf_counter() - t0:.1f} s")


def ctx(d, L, form):
    return f"N={d.N} {d.name} lengths={d.lengths} L={L} form={form}"


def check_exhaustive(d, L, got_idx):
    """The first 600 rows of both channels at up to five lambdas (6000 solves): the chosen points' scores are the maxima over
    all 2^(N+1) - 1 code points."""
    sel = sorted({0, 1, L // 2, L - 2, L - 1} & set(range(L)))
    rows = slice(0, min(600, d.mu.shape[0]))
    ll = None if d.level_len is None else d.level_len[sel]
    lam = [d.lam[i] for i in sel]
    best = R.exhaustive_max(d.mu[rows], d.sg[rows], d.tab, lam, d.N, level_len=ll, mode="f32")
    mine = R.chosen_scores(d.mu[rows], d.sg[rows], d.tab, lam, d.N, got_idx[sel][:, rows], level_len=ll, mode="f32")
    assert np.array_equal(mine, best), ctx(d, L, "cb")


def test_the_depths_are_the_ones_built():
    assert tuple(sorted(LP.SOLVE_DEPTHS)) == DEPTHS


@pytest.mark.parametrize("N", DEPTHS)
def test_indices_k1_mode0(ops, N):
    for d in FR.data(N):
        for L in FR.INDEX_L:
            for form in FR.forms(N):
                assert FR.plan(d, L, form) == FR.index_plan(L), ctx(d, L, form)      # 33 lambdas: K1<0>, then K1p<1>
                got = FR.quantize(ops, d, L, form)[0]
                assert FR.bit_equal(got, FR.expected(d, L, form)[0]), ctx(d, L, form)
                if form == "cb" and L == FR.INDEX_L[0]:
                    check_exhaustive(d, L, got)


@pytest.mark.parametrize("N", DEPTHS)
def test_zhat_and_lengths_k1_mode1(ops, N):
    for d in FR.data(N):
        for L in FR.OUTPUT_L:
            for form in FR.forms(N):
                wz, wb = form != "view", form != "cb-even"            # both, Z_hat alone, lengths alone
                assert FR.plan(d, L, form, want_zhat=wz, want_bits=wb) == FR.output_plan(L), ctx(d, L, form)
                got = FR.quantize(ops, d, L, form, want_zhat=wz, want_bits=wb)
                want = FR.expected(d, L, form)
                assert FR.bit_equal(got[0], want[0]), ctx(d, L, form)
                assert not wz or FR.bit_equal(got[1], want[1]), ctx(d, L, form)
                assert not wb or FR.bit_equal(got[2], want[2]), ctx(d, L, form)


@pytest.mark.parametrize("N", DEPTHS)
def test_level_counts_k1_mode2(ops, N):
    launched = 0
    for d in FR.data(N):
        for L in FR.COUNT_L:
            for form in FR.forms(N):
                p = FR.plan(d, L, form, counting=True)
                if N == 10 and d.lengths == "raw" and p == ["K1t"]:
                    assert d.name == "edge" and L == 8               # the one whole launch here that K1t takes: not this file's
                    continue
                if N == 10 and d.lengths == "raw" and L == FR.L_MAX:
                    assert p == ["K1<2>", "K1t"], ctx(d, L, form)    # the 33rd lambda alone is a sweep K1t takes
                else:
                    assert p == FR.count_plan(L), ctx(d, L, form)
                got = FR.level_counts(ops, d, L, form)
                want = FR.expected_counts(d, L, form)
                assert got.dtype == np.int64 and np.array_equal(got, want), ctx(d, L, form)
                assert int(got.sum()) == want.shape[1] * FR.expected(d, L, form)[0].shape[1] * L, ctx(d, L, form)
                launched += 1
    assert launched >= (len(FR.data(N)) * 2 - 1) * len(FR.forms(N))


@pytest.mark.parametrize("N", DEPTHS)
def test_one_to_four_lambdas_k1p(ops, N):
    for d in FR.data(N):
        for L in FR.PRUNED_L:
            for form in FR.forms(N):
                assert FR.plan(d, L, form) == FR.pruned_plan(L), ctx(d, L, form)
                got = FR.quantize(ops, d, L, form)[0]
                assert FR.bit_equal(got, FR.expected(d, L, form)[0]), ctx(d, L, form)
                if form == "cb" and L == 2:
                    check_exhaustive(d, L, got)


def test_flags_are_what_keeps_the_fast_solve_exact():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "tools", "fast_solve_control.py")]

    children = [subprocess.Popen(cmd, env=dict(os.environ, VBQ_FAST_DEBUG=str(dbg)), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                 text=True) for dbg in (0, 1, 2)]           # side by side: three processes on the device

    def result(child):
        out, err = child.communicate(timeout=300)
        assert child.returncode in (0, 1), out + err
        return child.returncode, json.loads(out.splitlines()[-1]), out
    try:
        results = [result(c) for c in children]
    finally:
        for c in children:                                           # a time limit or a crash: nothing stays behind
            if c.poll() is None:
                c.kill()
                c.communicate()
    for rc, bad, out in results[:2]:
        assert rc == 0 and not bad, out
    rc, bad, out = results[2]
    print(out)
    assert rc == 1, out
    for N in DEPTHS:
        for inst in ("K1<0>", "K1<1>"):
            for n in (N // 2, N):
                assert bad.get(f"{N} {inst} near_midpoint[{n}]", 0) > 0, (N, inst, n, out)
        assert bad.get(f"{N} K1<2> dyadic", 0) > 0, (N, out)
    assert not [k for k in bad if " K1p<" in k], out                  # no flags in K1p: nothing to switch off
