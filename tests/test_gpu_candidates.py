"""K1c, the candidate solve of vbq_candidates.hip (k_argmax_candidates<F64>), against a NumPy restatement that calls
np.argmax on the scores, as the reference's NumPy backend does (utils.py:395-401) -- not the oracle's '>' loop.

Routes: ops.argmax_candidates (mode given), utils.batch_quantize_indep_dims / quantize_indep_dims (mode from the
lengths' dtype, utils._mode: integer lengths -> "f64").  The kernel walks the elements with a grid-stride loop over at
most 4096 x 256 threads and the lambdas in chunks of 8 (kLamChunk); per-lambda length tables are read at
l0 * M * n_elems for the chunk starting at lambda l0.
"""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import rd_f64 as R
from oracle import vbq_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    from vbq_amd import ops as _ops
    t0 = time.perf_counter()
    yield _ops
    print(f"\n[test_gpu_candidates] {time.perf_counter() - t0:.1f} s")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def np_argmax_solve(P, lens, mu, sg, lambdas, mode):
    """utils.py:387-401 with np.argmax: (j, Z_hat, bits), each [L, *mu.shape]."""
    per_lambda = lens.ndim == P.ndim + 1
    js, zs, bs = [], [], []
    for i, lam in enumerate(lambdas):
        Li = lens[i] if per_lambda else lens
        j = np.argmax(R.score(P, Li, mu[None], sg[None], lam, mode), axis=0)
        js.append(j)
        zs.append(np.take_along_axis(P, j[None], axis=0)[0])
        bs.append(np.take_along_axis(np.asarray(Li, F32), j[None], axis=0)[0])
    return np.stack(js), np.stack(zs), np.stack(bs)


def candidates(rng, M, n, L=None):
    """Candidate points around mu with duplicates and mirrored pairs (exact distortion ties), integer-valued lengths
    (exact score ties).  Values are multiples of 1/64 near mu = k/8 so that the mirrored distances are exact."""
    mu = (rng.integers(-40, 40, n) / 8).astype(F32)
    sg = np.exp(rng.normal(-1, 1, n)).astype(F32)
    P = (mu[None] + rng.integers(-256, 256, (M, n)) / 64).astype(F32)
    if M > 1:
        dup = rng.random((M, n)) < 0.2
        P[1:] = np.where(dup[1:], P[:-1], P[1:])                               # repeated candidates
        mir = rng.random((M, n)) < 0.2
        P[1:] = np.where(mir[1:], 2 * mu[None] - P[:-1], P[1:])                 # same distance on the other side
    shape = (M, n) if L is None else (L, M, n)
    lens = rng.integers(0, 12, shape).astype(F32)
    return P, lens, mu, sg


def compare(ops, P, lens, mu, sg, lam, mode):
    zh, bt, j = ops.argmax_candidates(dev(P), dev(lens), dev(mu), dev(sg), lam, mode=mode, want_j=True)
    wj, wz, wb = np_argmax_solve(P, lens, mu, sg, lam, mode)
    assert np.array_equal(host(j), wj)
    assert np.array_equal(host(zh), wz, equal_nan=True) and np.array_equal(host(bt), wb, equal_nan=True)


LAMS = [0.0, 2.0 ** -8 * np.sqrt(2.0), 0.1, 1.0, 7.0]


@pytest.mark.parametrize("mode", ["f32", "f64"])
@pytest.mark.parametrize("M", [1, 2, 21, 2047, 4095])
def test_candidate_counts(ops, mode, M):
    rng = np.random.default_rng(M)
    n = min(20000, 2_000_000 // M)
    P, lens, mu, sg = candidates(rng, M, n)
    compare(ops, P, lens, mu, sg, LAMS, mode)


@pytest.mark.parametrize("mode", ["f32", "f64"])
@pytest.mark.parametrize("per_lambda", [False, True])
@pytest.mark.parametrize("L", [1, 7, 8, 9, 17])
def test_lambda_chunks_and_per_lambda_lengths(ops, mode, per_lambda, L):
    rng = np.random.default_rng(L * 2 + per_lambda)
    M, n = 21, 3001
    P, lens, mu, sg = candidates(rng, M, n, L if per_lambda else None)
    lam = list(np.geomspace(1e-3, 10.0, L) * np.sqrt(2.0))
    lam[L // 2] = 0.0
    compare(ops, P, lens, mu, sg, lam, mode)


@pytest.mark.parametrize("mode", ["f32", "f64"])
def test_more_elements_than_the_grid(ops, mode):
    rng = np.random.default_rng(9)
    n = 4096 * 256 + 4099
    P, lens, mu, sg = candidates(rng, 2, n)
    compare(ops, P, lens, mu, sg, [0.1, 0.0], mode)


def test_utils_integer_lengths_score_in_f64(split_elements):
    """Integer lengths through utils take f64 (utils._mode), float lengths f32: quantize_indep_dims / batch_quantize_
    indep_dims over the whole sorted code book equal np.argmax of the matching arithmetic on elements where the two
    modes disagree."""
    from vbq_amd import utils
    tab, z, s = split_elements
    srt = np.sort(tab[0])
    lev = O.levels_of_sorted_ranks(10)
    K = len(z)
    cp = np.repeat(srt[None], K, axis=0)                                 # K x M, sorted (utils.py:341)
    cl = np.repeat(lev[None], K, axis=0).astype(np.int64)
    fun = utils.curry_normal_logpdf(loc=z, scale=s, ignore_const=True)
    lam = [0.0, 2.0 ** -8 * np.sqrt(2.0), 0.1, 0.3]
    Zd, Bd = utils.batch_quantize_indep_dims((1, K), cp, cl, fun, lam)
    Zf, Bf = utils.batch_quantize_indep_dims((1, K), cp, cl.astype(F32), fun, lam)
    apart = 0
    for i, l in enumerate(lam):
        for mode, (zd, bd) in (("f64", (Zd, Bd)), ("f32", (Zf, Bf))):
            j = np.argmax(R.score(srt[:, None], lev[:, None], z[None], s[None], l, mode), axis=0)
            assert np.array_equal(zd[l][0], srt[j]) and np.array_equal(bd[l][0], lev[j]), (mode, l)
        assert Bd[l].dtype == np.int32
        apart += int(np.sum(Zd[l][0] != Zf[l][0]))
    assert apart >= 20
    for k in range(0, K, max(1, K // 7)):
        f1 = utils.curry_normal_logpdf(loc=z[k:k + 1], scale=s[k:k + 1], ignore_const=True)
        zz, bb = utils.quantize_indep_dims(z[k:k + 1], cp[k:k + 1], cl[k:k + 1], f1, lam[2])
        j = np.argmax(R.score(srt, lev, z[k], s[k], lam[2], "f64"))
        assert zz[0] == srt[j] and bb[0] == lev[j]


@pytest.fixture(scope="module")
def split_elements():
    from oracle.mode_split import mode_splitting_set
    tab, z, s, _ = mode_splitting_set(seed=7, n=6000)
    return tab, z, s


def nan_candidates():
    """Per element (columns) a candidate set whose scores hold NaN: +-inf points against an infinite mu or sigma
    (inf - inf, inf / inf), and infinite lengths times lambda = 0.  Column 1 has none; column 6 has it at candidate 0."""
    inf = F32(np.inf)
    P = np.array([[0.5, 0.5, 0.5, 0.5, 0.75, 0.5, inf, 0.5],
                  [inf, 0.25, 0.25, 0.75, -inf, 0.25, 0.5, 0.25],
                  [0.25, inf, inf, 0.25, 0.25, 0.5, 0.75, 0.75],
                  [inf, 0.75, 0.75, inf, 0.25, 0.75, 0.25, 0.25]], F32)
    mu = np.array([inf, 0.5, 0.5, inf, 0.5, 0.5, 0.5, 0.5], F32)
    sg = np.array([1.0, 1.0, inf, 1.0, inf, 1.0, inf, 1.0], F32)
    lens = np.array([[1, 2, 1, 1, 1, 1, 1, 1],
                     [2, 3, 2, 2, 2, 2, 2, inf],
                     [3, 4, 3, 3, 3, inf, 3, 2],
                     [4, 5, 4, 4, 4, inf, 4, inf]], F32)
    return P, lens, mu, sg


def strict_scan(S):
    """The first maximum by a strict '>' scan from candidate 0 (the VBQ_MODE_F32 rule)."""
    want = np.zeros(S.shape[1], np.int64)
    best = S[0].copy()
    for k in range(1, S.shape[0]):
        up = S[k] > best
        best = np.where(up, S[k], best)
        want = np.where(up, k, want)
    return want


def test_nan_scores_f64_follow_np_argmax(ops):
    P, lens, mu, sg = nan_candidates()
    lam = [0.0, 0.5]
    S = np.stack([R.score(P, lens, mu[None], sg[None], l, "f64") for l in lam])
    assert np.sum(np.argmax(S[0], axis=0) != strict_scan(S[0])) >= 5       # the input tells the two rules apart
    zh, bt, j = ops.argmax_candidates(dev(P), dev(lens), dev(mu), dev(sg), lam, mode="f64", want_j=True)
    assert np.array_equal(host(j), np.argmax(S, axis=1))
    wj, wz, wb = np_argmax_solve(P, lens, mu, sg, lam, "f64")
    assert np.array_equal(host(j), wj) and np.array_equal(host(zh), wz) and np.array_equal(host(bt), wb)
    # the oracle's loop says the same
    with np.errstate(all="ignore"):
        _, _, win = O.rd_solve(P[:, None], lens[:, None], mu[None], sg[None], lam, mode="f64")
    assert np.array_equal(win[:, 0], wj)


def test_nan_scores_f32_keep_the_strict_scan(ops):
    """VBQ_MODE_F32 (include/vbq.h, K1c): a NaN score never replaces the running best -- candidate 0 if it scores NaN."""
    P, lens, mu, sg = nan_candidates()
    lam = [0.0, 0.5]
    zh, bt, j = ops.argmax_candidates(dev(P), dev(lens), dev(mu), dev(sg), lam, mode="f32", want_j=True)
    for i, l in enumerate(lam):
        assert np.array_equal(host(j)[i], strict_scan(R.score(P, lens, mu[None], sg[None], l, "f32")))
