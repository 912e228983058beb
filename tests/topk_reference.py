"""The nearest-row search of include/vbq.h ("Nearest rows") stated a second time, in NumPy and float64, and the rule by which a
float32 result is accepted against it.

    scores(q, emb, metric)      q64 . v64, for the cosine divided by 1e-8 + |v64|
    topk(q, emb, k, ...)        the first k rows by (score descending, id ascending) among the rows not excluded, padded with
                                id -1 / score -inf
    accept(ids, scores, ...)    AssertionError unless a float32 result is one the contract allows

The acceptance rule has no tuned number.  With u = 2^-24, gamma_n = n u / (1 - n u) and A_v = sum_k |q_k v_k| in float64, a
float32 score of row v may differ from the float64 one by
    dot      b_v = gamma_K A_v                       (K products and K - 1 sums, each rounded once)
    cosine   b_v = 2 gamma_{K+4} A_v / den64_v       (the numerator chain, the norm chain, sqrt, add and divide each contribute at
                                                      most gamma_K or a few u relative to A_v; the factor 2 covers the product of
                                                      the two)
and the rule is: ids distinct, in range, not excluded; scores non-increasing with equal scores in ascending id;
|score_i - s64_i| <= b_i; no eligible unreturned row j has s64_j > s64_last + b_j + b_last; padding only at the tail and only
when every eligible row is returned."""
import functools

import numpy as np

U = 2.0 ** -24

# (K, V, Q, k): a sample of K in {1, 5, 64, 65, 100, 300} x V in {1, 31, 33, 130, 2500} x Q in {1, 32, 33} x k in {1, 10, 64} in
# which every value occurs at least twice; k > V, odd K, the chunk of 64 coordinates, a second query block and a second and a
# twentieth tile of rows are all there.  Each is run with both metrics.
CASES = [(1, 1, 1, 1), (5, 31, 32, 10), (64, 33, 33, 64), (65, 130, 1, 10), (100, 2500, 33, 64), (300, 2500, 32, 10),
         (300, 130, 33, 1), (1, 2500, 1, 64), (5, 1, 33, 10), (64, 2500, 32, 1), (65, 31, 1, 64), (100, 33, 32, 10)]


def gamma(n):
    return n * U / (1.0 - n * U)


@functools.lru_cache(maxsize=None)
def case_data(K, V, Q):
    """(emb f32 [V, K], queries f32 [Q, K], exclude int64 [Q, 3]) of a case: the same arrays for every test that asks.  Every
    seventh row repeats the row before it (ties), the exclusions name rows, -1 and a row past the end."""
    rng = np.random.default_rng(1000 * K + 10 * V + Q)
    emb = rng.standard_normal((V, K)).astype(np.float32)
    emb[7::7] = emb[6:-1:7][:len(emb[7::7])]
    q = rng.standard_normal((Q, K)).astype(np.float32)
    exclude = rng.integers(0, V, (Q, 3)).astype(np.int64)
    exclude[::2, 1] = -1
    exclude[1::3, 2] = V + 5
    for a in (emb, q, exclude):
        a.setflags(write=False)
    return emb, q, exclude


def scores(q, emb, metric):
    """float64 [Q, V]."""
    q64, v64 = np.asarray(q, np.float64), np.asarray(emb, np.float64)
    s = q64 @ v64.T
    if metric == "cosine":
        s = s / (1e-8 + np.sqrt((v64 * v64).sum(axis=1)))[None, :]
    else:
        assert metric == "dot", metric
    return s


def bounds(q, emb, metric):
    """b_v of the module docstring, float64 [Q, V]."""
    q64, v64 = np.asarray(q, np.float64), np.asarray(emb, np.float64)
    K = v64.shape[1]
    A = np.abs(q64) @ np.abs(v64).T
    if metric == "cosine":
        return 2.0 * gamma(K + 4) * A / (1e-8 + np.sqrt((v64 * v64).sum(axis=1)))[None, :]
    return gamma(K) * A


def _eligible(V, exclude_row):
    ok = np.ones(V, dtype=bool)
    if exclude_row is not None:
        e = np.asarray(exclude_row, np.int64)
        ok[e[(e >= 0) & (e < V)]] = False
    return ok


def order(s, ids):
    """`ids` sorted by (score descending, id ascending); -0.0 == 0.0."""
    ids = np.asarray(ids, np.int64)
    return ids[np.lexsort((ids, -(s[ids] + 0.0)))]


def topk(q, emb, k, metric, exclude=None):
    """(ids int64 [Q, k], scores float64 [Q, k])."""
    s = scores(q, emb, metric)
    Q, V = s.shape
    ids = np.full((Q, k), -1, np.int64)
    out = np.full((Q, k), -np.inf)
    for i in range(Q):
        best = order(s[i], np.flatnonzero(_eligible(V, None if exclude is None else exclude[i])))[:k]
        ids[i, :best.size] = best
        out[i, :best.size] = s[i, best]
    return ids, out


def accept(ids, got, q, emb, k, metric, exclude=None):
    """AssertionError unless (ids [Q, k], got f32 [Q, k]) is an allowed result for the queries q [Q, K] and the rows emb."""
    ids, got = np.asarray(ids), np.asarray(got)
    s, b = scores(q, emb, metric), bounds(q, emb, metric)
    Q, V = s.shape
    assert ids.shape == (Q, k) and got.shape == (Q, k), (ids.shape, got.shape, (Q, k))
    for i in range(Q):
        ok = _eligible(V, None if exclude is None else exclude[i])
        n = min(k, int(ok.sum()))
        r, g = ids[i, :n].astype(np.int64), got[i, :n].astype(np.float64)
        assert (ids[i, n:] == -1).all() and (got[i, n:] == -np.inf).all(), (i, "the tail is not -1 / -inf", ids[i], got[i])
        assert ((r >= 0) & (r < V)).all(), (i, "an id out of range", r)
        assert np.unique(r).size == n, (i, "a repeated id", r)
        assert ok[r].all(), (i, "an excluded id", r)
        assert not np.isnan(g).any(), (i, "a NaN score")
        later = (g[1:] < g[:-1]) | ((g[1:] == g[:-1]) & (r[1:] > r[:-1]))
        assert later.all(), (i, "not ordered by score descending, id ascending", r, g)
        err = np.abs(g - s[i, r])
        assert (err <= b[i, r]).all(), (i, "a score off by more than its bound", err.max(), b[i, r].max())
        if n == k:
            rest = ok.copy()
            rest[r] = False
            worse = s[i] <= s[i, r[-1]] + b[i] + b[i, r[-1]]
            assert worse[rest].all(), (i, "a better row was left out", np.flatnonzero(rest & ~worse)[:5], r[-1])
