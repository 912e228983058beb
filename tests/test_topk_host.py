"""The float64 restatement of the nearest-row search (tests/topk_reference.py) against a brute-force sort, its acceptance rule
against float32 results that must pass and results that must not, and the argument checks of the C calls -- all without a
GPU."""
import ctypes as C

import numpy as np
import pytest

import topk_reference as TR

METRICS = ("dot", "cosine")


def _brute(q, emb, k, metric, exclude):
    """Every (score, id) pair of a query as Python tuples, sorted."""
    out_ids, out_s = [], []
    for i in range(q.shape[0]):
        pairs = []
        for v in range(emb.shape[0]):
            if exclude is not None and v in set(int(e) for e in exclude[i]):
                continue
            s = float(np.dot(q[i].astype(np.float64), emb[v].astype(np.float64)))
            if metric == "cosine":
                s /= 1e-8 + float(np.sqrt(np.sum(emb[v].astype(np.float64) ** 2)))
            pairs.append((-s, v))
        pairs.sort()
        pairs = pairs[:k] + [(np.inf, -1)] * (k - len(pairs[:k]))
        out_ids.append([p[1] for p in pairs])
        out_s.append([-p[0] for p in pairs])
    return np.array(out_ids, np.int64), np.array(out_s)


@pytest.mark.parametrize("metric", METRICS)
def test_reference_equals_a_brute_force_sort(metric):
    rng = np.random.default_rng(3)
    for V, K, Q, k in ((1, 3, 2, 4), (9, 1, 3, 3), (12, 4, 2, 12), (12, 4, 2, 5)):
        emb = rng.integers(-2, 3, (V, K)).astype(np.float32)         # small integers: many exact ties
        q = rng.integers(-2, 3, (Q, K)).astype(np.float32)
        for exclude in (None, rng.integers(-1, V + 1, (Q, 2))):
            ids, s = TR.topk(q, emb, k, metric, exclude)
            want_ids, want_s = _brute(q, emb, k, metric, exclude)
            assert np.array_equal(ids, want_ids), (V, K, Q, k)
            assert np.allclose(s, want_s, rtol=1e-15, atol=0), (V, K, Q, k)   # np.dot's order against the matrix product's


def _unfused_f32(q, emb, metric):
    """float32 [Q, V]: acc = acc + q_k * v_k with the product rounded on its own, ascending k; the cosine's denominator by the
    same kind of chain."""
    acc = np.zeros((q.shape[0], emb.shape[0]), np.float32)
    sq = np.zeros(emb.shape[0], np.float32)
    for kk in range(emb.shape[1]):
        acc = acc + q[:, kk, None] * emb[None, :, kk]
        sq = sq + emb[:, kk] * emb[:, kk]
    assert acc.dtype == np.float32 and sq.dtype == np.float32
    return acc / (np.float32(1e-8) + np.sqrt(sq))[None, :] if metric == "cosine" else acc


def _topk_f32(s, k, exclude):
    Q, V = s.shape
    ids = np.full((Q, k), -1, np.int64)
    out = np.full((Q, k), -np.inf, np.float32)
    for i in range(Q):
        best = TR.order(s[i], np.flatnonzero(TR._eligible(V, None if exclude is None else exclude[i])))[:k]
        ids[i, :best.size] = best
        out[i, :best.size] = s[i, best]
    return ids, out


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("K,V,Q,k", TR.CASES)
def test_accept_passes_for_a_float32_chain_that_is_not_fused(K, V, Q, k, metric):
    """The bound is not so tight that only the kernel's own fused chain meets it."""
    emb, q, exclude = TR.case_data(K, V, Q)
    for ex in (None, exclude):
        ids, s = _topk_f32(_unfused_f32(q, emb, metric), k, ex)
        TR.accept(ids, s, q, emb, k, metric, ex)


@pytest.mark.parametrize("metric", METRICS)
def test_accept_fails_for_what_the_contract_forbids(metric):
    K, V, Q, k = 100, 2500, 33, 64
    emb, q, exclude = TR.case_data(K, V, Q)
    ids, s = TR.topk(q, emb, k, metric, exclude)
    s = s.astype(np.float32)
    TR.accept(ids, s, q, emb, k, metric, exclude)
    # one id swapped for a clearly worse row, with that row's own score
    full = TR.scores(q, emb, metric)
    worst = int(np.argmin(full[5]))
    bad_ids, bad_s = ids.copy(), s.copy()
    bad_ids[5, -1], bad_s[5, -1] = worst, full[5, worst]
    with pytest.raises(AssertionError, match="better row"):
        TR.accept(bad_ids, bad_s, q, emb, k, metric, exclude)
    # a tie returned in descending id: rows 6 and 7 are copies, query with row 6 so that both lead
    qq = np.array(emb[6:7])
    tid, ts = TR.topk(qq, emb, 4, metric)
    assert ts[0, 0] == ts[0, 1] and tid[0, 0] < tid[0, 1]
    TR.accept(tid, ts.astype(np.float32), qq, emb, 4, metric)
    swapped = tid.copy()
    swapped[0, :2] = tid[0, 1], tid[0, 0]
    with pytest.raises(AssertionError, match="not ordered"):
        TR.accept(swapped, ts.astype(np.float32), qq, emb, 4, metric)
    # an excluded id returned
    row = int(np.flatnonzero((exclude[:, 0] >= 0) & (exclude[:, 0] < V))[0])
    bad_ids, bad_s = ids.copy(), s.copy()
    bad_ids[row, -1], bad_s[row, -1] = exclude[row, 0], full[row, exclude[row, 0]]
    with pytest.raises(AssertionError):
        TR.accept(bad_ids, bad_s, q, emb, k, metric, exclude)
    # and a padded tail where rows were to be had
    bad_ids, bad_s = ids.copy(), s.copy()
    bad_ids[0, -1], bad_s[0, -1] = -1, -np.inf
    with pytest.raises(AssertionError):
        TR.accept(bad_ids, bad_s, q, emb, k, metric, exclude)


def test_the_c_calls_check_their_arguments_before_any_device_work():
    from vbq_amd import _lib
    h = _lib.lib()
    ws = h.vbq_topk_workspace_bytes
    for V, K, Q, k in ((400_000, 300, 1, 10), (2500, 100, 33, 64), (1, 1, 1, 1)):
        for mw in (0, 1, 7):
            assert ws(V, K, Q, k, mw) >= Q * k * 12, (V, K, Q, k, mw)
    assert ws(2500, 100, 33, 64, 5) == 5 * 33 * 64 * 12
    for bad in ((0, 100, 1, 10, 0), (1 << 31, 100, 1, 10, 0), (10, 0, 1, 10, 0), (10, 4, 0, 10, 0), (10, 4, 1, 0, 0),
                (10, 4, 1, 65, 0), (10, 4, 1, 10, -1)):
        assert ws(*bad) == 0, bad
    p = C.c_void_p(64)                    # never dereferenced: every call below returns before any device work
    err = lambda: h.vbq_last_error().decode()

    def dense(emb=p, V=10, K=4, q=p, Q=3, k=5, metric=1, ex=None, E=0, ids=p, sc=p, mw=0, w=p, wb=1 << 20):
        return h.vbq_topk_f32(emb, V, K, q, Q, k, metric, ex, E, ids, sc, mw, w, wb, None)

    def records(words=p, V=10, K=4, N=10, tb=9, tab=p, nt=1, q=p, Q=3, k=5, metric=1, ex=None, E=0, ids=p, sc=p, st=None, mw=0,
                w=p, wb=1 << 20):
        return h.vbq_records_topk_f32(words, V, K, N, tb, tab, nt, q, Q, k, metric, ex, E, ids, sc, st, mw, w, wb, None)

    for call in (dense, records):
        for kw, what in ((dict(k=0), "k = 0"), (dict(k=65), "k = 65"), (dict(E=9, ex=p), "E = 9"), (dict(metric=2), "metric 2"),
                         (dict(V=0), "bad sizes"), (dict(K=0), "bad sizes"), (dict(Q=-1), "bad sizes"), (dict(mw=-1), "max_workgroups"),
                         (dict(q=None), "null pointer"), (dict(ids=None), "null pointer"), (dict(sc=None), "null pointer"),
                         (dict(w=None), "null pointer"), (dict(E=2), "null pointer")):
            assert call(**kw) == -1 and what in err(), (call.__name__, kw, err())
        assert call(Q=0, q=None, ids=None, sc=None, w=None) == 0
        assert call(wb=3 * 5 * 12 - 1, mw=1) == -4 and "workspace" in err()
    assert dense(emb=None) == -1 and "null pointer" in err()
    assert records(words=None) == -1 and "null pointer" in err()
    assert records(tab=None) == -1 and "null pointer" in err()
    for nt in (0, 2, 3, 5):
        assert records(nt=nt) == -1 and "n_tables" in err(), nt
    assert records(N=11) == -1 and records(N=0) == -1 and records(tb=41) == -1 and "total_bits" in err()
    # above the tiles' LDS the calls refuse and name the limit; every K <= 512 is below it, whatever N and total_bits
    assert dense(K=700) == -2 and "limit is 163840" in err() and "512" in err()
    assert records(K=700, tb=0) == -2 and "limit is 163840" in err()
    for N, tb in ((10, 5120), (10, 0), (1, 512), (3, 777)):
        for nt in (1, 512):
            assert records(K=512, N=N, tb=tb, nt=nt, w=None) == -1 and "null pointer" in err(), (N, tb, nt)
    assert dense(K=512, w=None) == -1 and "null pointer" in err()
