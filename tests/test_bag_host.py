"""The NumPy restatement of the pooled lookup (tests/bag_reference.py) on hand-computed cases, the argument checks of the two C
calls and every refusal of the Python layer that needs no device -- all without a GPU."""
import ctypes as C

import numpy as np
import pytest

import bag_reference as BR


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32).tolist()


def test_reference_on_hand_computed_cases():
    emb = np.array([[1.0, -2.0], [2.0, 0.5], [4.0, -8.0]], np.float32)
    ids = np.array([0, 1, 2, 2, -1, 1], np.int64)
    offsets = np.array([0, 3, 3, 6], np.int64)
    out, st = BR.bag(emb, ids, offsets)
    assert st == 0 and out.dtype == np.float32 and out.tolist() == [[7.0, -9.5], [0.0, 0.0], [6.0, -7.5]]
    out, st = BR.bag(emb, ids, offsets, mode="mean")                       # the padding does not count: 6 / 2, not 6 / 3
    assert st == 0 and _bits(out) == _bits([[np.float32(7) / np.float32(3), np.float32(-9.5) / np.float32(3)], [0, 0], [3.0, -3.75]])
    out, st = BR.bag(emb, ids, offsets, mode="max")
    assert st == 0 and out.tolist() == [[4.0, 0.5], [0.0, 0.0], [4.0, 0.5]]
    out, st = BR.bag(emb, ids, offsets, weights=np.array([2, 0.5, -1, 1, 9, 0], np.float32))
    assert st == 0 and out.tolist() == [[-1.0, 4.25], [0.0, 0.0], [4.0, -8.0]]
    # an id >= V is skipped, not counted, and reported
    out, st = BR.bag(emb, np.array([0, 3, 1], np.int64), np.array([0, 3], np.int64), mode="mean")
    assert st == BR.BAD_ROW and out.tolist() == [[1.5, -0.75]]
    # offsets: a reversed pair is an empty bag, an end past n is clamped; both reported, the other bags untouched
    out, st = BR.bag(emb, np.array([0, 1, 2], np.int64), np.array([0, 2, 1, 9], np.int64))
    assert st == BR.BAD_OFFSETS and out.tolist() == [[3.0, -1.5], [0.0, 0.0], [6.0, -7.5]]


def test_reference_max_keeps_the_value_met_first_on_a_tie_of_zeros():
    emb = np.array([[0.0, -0.0, -1.0], [-0.0, 0.0, -1.0]], np.float32)
    out, _ = BR.bag(emb, np.array([0, 1, 1, 0], np.int64), np.array([0, 2, 4], np.int64), mode="max")
    assert _bits(out) == [[0, 0x80000000, 0xBF800000], [0x80000000, 0, 0xBF800000]]
    # the sum starts at +0: a lone -0 sums to +0 but is its own maximum
    lone = dict(ids=np.array([0], np.int64), offsets=np.array([0, 1], np.int64))
    assert _bits(BR.bag(emb, **lone)[0]) == [[0, 0, 0xBF800000]]
    assert _bits(BR.bag(emb, **lone, mode="max")[0]) == [[0, 0x80000000, 0xBF800000]]


def test_reference_mean_and_max_of_a_bag_without_counted_entries_are_plus_zero():
    emb = np.full((2, 3), -5.0, np.float32)
    ids, offsets = np.array([-1, -7, -1], np.int64), np.array([0, 3, 3], np.int64)
    for mode in BR.MODES:
        out, st = BR.bag(emb, ids, offsets, mode=mode)
        assert st == 0 and _bits(out) == [[0, 0, 0], [0, 0, 0]], mode


def test_reference_rounds_the_weighted_product_before_it_adds():
    emb, ids, offsets, weights, want = BR.contraction_case()
    out, st = BR.bag(emb, ids, offsets, weights=weights)
    assert st == 0 and _bits(out) == _bits([[want]])
    fused = np.float32(float(weights[1]) * float(emb[1, 0]) - 1.0)          # exact in float64, rounded once
    assert fused == np.float32(2.0 ** -11 + 2.0 ** -24) and fused != want   # what a contracted kernel would return


def test_reference_padded_form():
    ids, offsets = np.array([5, 6, 7, 8], np.int64), np.array([0, 0, 3, 4], np.int64)
    assert BR.padded(ids, offsets).tolist() == [[-1, -1, -1], [5, 6, 7], [8, -1, -1]]


def test_the_c_calls_check_their_arguments_before_any_device_work():
    from vbq_amd import _lib
    h = _lib.lib()
    p = C.c_void_p(64)                    # never dereferenced: every call below returns before any device work
    err = lambda: h.vbq_last_error().decode()                                # noqa: E731

    def dense(emb=p, V=10, K=4, ids=p, n=6, off=p, B=3, w=None, mode=0, out=p, st=None):
        return h.vbq_bag_f32(emb, V, K, ids, n, off, B, w, mode, out, st, None)

    def records(words=p, V=10, K=4, N=10, tb=9, tab=p, nt=1, ids=p, n=6, off=p, B=3, w=None, mode=0, out=p, st=None):
        return h.vbq_records_bag_f32(words, V, K, N, tb, tab, nt, ids, n, off, B, w, mode, out, st, None)

    for call in (dense, records):
        for kw, what in ((dict(V=0), "bad sizes"), (dict(K=0), "bad sizes"), (dict(n=-1), "bad sizes"), (dict(B=-1), "bad sizes"),
                         (dict(mode=3), "mode 3"), (dict(mode=-1), "mode -1"), (dict(w=p, mode=1), "weights"),
                         (dict(w=p, mode=2), "weights"), (dict(ids=None), "null pointer"), (dict(off=None), "null pointer"),
                         (dict(out=None), "null pointer")):
            assert call(**kw) == -1 and what in err(), (call.__name__, kw, err())
        assert call(B=0, ids=None, off=None, out=None) == 0                  # no bags: nothing to do
        assert call(B=0, mode=3) == -1 and call(B=0, w=p, mode=1) == -1      # but still a checked call
    assert dense(emb=None) == -1 and "null pointer" in err()
    assert records(words=None) == -1 and "null pointer" in err()
    assert records(tab=None) == -1 and "null pointer" in err()
    for nt in (0, 2, 3, 5):
        assert records(nt=nt) == -1 and "n_tables" in err(), nt
    assert records(N=11) == -1 and records(N=0) == -1 and records(tb=41) == -1 and "total_bits" in err()
    # One bag's working set -- the staged record and two sets of K accumulators -- must fit 160 KiB of LDS: the header states that
    # every K <= 16804 does whatever N, total_bits and n_tables (ceil(14 K / 32) + 2 K <= 40960 words), the dense source up to
    # K = 20480.  At the limit the sizes pass (the next check, the pointers, fails); one past it the calls name the limit.
    KMAX = 16804
    assert (14 * KMAX + 31) // 32 + 2 * KMAX <= 40960 < (14 * (KMAX + 1) + 31) // 32 + 2 * (KMAX + 1)
    for N, tb in ((10, 10 * KMAX), (10, 0), (1, KMAX), (3, 7777)):
        for nt in (1, KMAX):
            assert records(K=KMAX, N=N, tb=tb, nt=nt, out=None) == -1 and "null pointer" in err(), (N, tb, nt)
            assert records(K=KMAX, N=N, tb=tb, nt=nt, B=0) == 0
    assert records(K=KMAX + 1, tb=10 * (KMAX + 1)) == -2 and "limit is 163840" in err() and str(KMAX) in err()
    assert records(K=KMAX + 1, tb=10 * (KMAX + 1), B=0) == -2                # also with nothing to do: the sizes come first
    assert records(K=KMAX + 1, tb=0, out=None) == -1 and "null pointer" in err()   # a shorter record still fits
    assert dense(K=20480, out=None) == -1 and "null pointer" in err()
    assert dense(K=20481) == -2 and "limit is 163840" in err() and str(KMAX) in err()


def test_python_layer_refuses_without_a_device():
    """embeddings.bag checks ids, offsets, weights and mode on the host before it looks for a device."""
    from vbq_amd import embeddings as E
    emb = np.zeros((5, 3), np.float32)
    ids, offsets = np.array([0, 1, -1, 4]), np.array([0, 2])
    ok = E._bag_args(ids, offsets, None, "sum", 5)
    assert ok[0].tolist() == [0, 1, -1, 4] and ok[1].tolist() == [0, 2, 4] and ok[2] is None
    two = E._bag_args(ids.reshape(2, 2), None, np.ones((2, 2)), "sum", 5)
    assert two[0].tolist() == [0, 1, -1, 4] and two[1].tolist() == [0, 2, 4] and two[2].dtype == np.float32
    empty = E._bag_args(np.zeros(0, np.int64), np.zeros(0, np.int64), None, "max", 5)
    assert empty[0].size == 0 and empty[1].tolist() == [0]
    for mode in ("avg", 0, None):
        with pytest.raises(ValueError, match="mode"):
            E.bag(emb, ids, offsets, mode=mode)
    for mode in ("mean", "max"):
        with pytest.raises(ValueError, match="weights go with mode 'sum'"):
            E.bag(emb, ids, offsets, mode=mode, weights=np.ones(4))
    for w in (np.ones(3), np.ones((2, 2)), np.ones((4, 1))):
        with pytest.raises(ValueError, match="differ in shape"):
            E.bag(emb, ids, offsets, weights=w)
    with pytest.raises(ValueError, match="differ in shape"):
        E.bag(emb, ids.reshape(2, 2), weights=np.ones(4))
    for poison in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="NaN or an infinity"):
            E.bag(emb, ids, offsets, weights=np.array([1, poison, 1, 1]))
    for bad in (np.array([0.0, 1.0]), np.array([True, False])):
        with pytest.raises(IndexError, match="integers"):
            E.bag(emb, bad, np.array([0]))
    for bad in ([0, 5], [-1, 1 << 40]):
        with pytest.raises(IndexError, match="outside"):
            E.bag(emb, np.array(bad), np.array([0]))
    with pytest.raises(IndexError, match="outside"):
        E.bag(emb, np.array([[0, 1], [2, 5]]))
    for bad in ([1, 2], [0, 3, 2], [0, 5], [-1, 2], []):
        with pytest.raises(ValueError, match="offsets must start at 0"):
            E.bag(emb, ids, np.array(bad, np.int64))
    with pytest.raises(ValueError, match="offsets"):
        E.bag(emb, ids, np.array([0.0, 2.0]))
    with pytest.raises(ValueError, match="offsets"):
        E.bag(emb, ids, np.array([[0, 2]]))
    with pytest.raises(ValueError, match="need offsets"):
        E.bag(emb, ids)
    with pytest.raises(ValueError, match="offsets must be None"):
        E.bag(emb, ids.reshape(2, 2), offsets)
    with pytest.raises(ValueError, match="ids must be"):
        E.bag(emb, ids.reshape(1, 2, 2))
    with pytest.raises(ValueError, match=r"\[V, K\]"):
        E.bag(emb.reshape(-1), ids, offsets)
