"""Listed rows (vbq_amd/ext/vbqx_scores.hip; include/vbq_ext.h) on the GPU, without a tolerance anywhere: both sources and both
metrics against the exact restatement tests/scores_reference.py, the record source against the dense one, both against the
scores the search reports, the independence of the grouping, status and padding, rerank's order, the write footprint, the
stream order and the memory claim.  Record files are built from synthetic rank indices (tests/records_reference.py) and the
pack kernel, as the record tests do.

Stream order (tests/stream_order.py, imported unchanged).  ARMED, blocking=False: ops.records_scores and ops.scores, the
wrappers of the two C calls -- they return their tensor with nothing read back.  NOT armed, blocking=True (late inputs and the
exact comparison, no arming assertion): RecordEmbeddings.scores / similarity / rerank and the module's three.  They share
most_similar's query checks, whose look for a non-finite coordinate reads the device before the launch; similarity reads its
ids on the host; and with device ids the status word is read after the launch -- the one blocking point that is this
feature's own."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import footprint as FP  # noqa: E402
import records_reference as RR  # noqa: E402
import scores_reference as SR  # noqa: E402
import stream_order as SO  # noqa: E402
import topk_reference as TR  # noqa: E402

gpu = pytest.mark.gpu
METRICS = ("dot", "cosine")

# (K, Q, M, V, N, total_bits, one code book per column): every K of {1, 5, 64, 65, 100, 300, 512} (the chunk of 64 coordinates,
# groups of 64, 16 and 8 pairs), every (Q, M) of {(1, 1), (1, 63), (1, 64), (1, 65), (43, 3), (33, 64), (130, 1)} (the wave
# boundary, groups that span queries, one id per query), every V of {1, 33, 130}, N of {1, 3, 10} and total_bits of {0, mid,
# K N} at least twice, both kinds of code book seven times.
CASES = [(1, 1, 1, 1, 1, "zero", False), (5, 1, 63, 33, 3, "mid", True), (64, 1, 64, 130, 10, "full", False),
         (65, 1, 65, 1, 1, "mid", True), (100, 43, 3, 33, 3, "full", False), (300, 33, 64, 130, 10, "mid", True),
         (512, 130, 1, 33, 10, "zero", False), (1, 130, 1, 130, 3, "full", True), (5, 33, 64, 1, 10, "mid", False),
         (64, 43, 3, 33, 1, "zero", True), (65, 1, 65, 130, 10, "full", True), (100, 1, 64, 1, 3, "zero", False),
         (300, 1, 63, 33, 1, "full", False), (512, 1, 1, 130, 10, "mid", True)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


@pytest.fixture(scope="module", autouse=True)
def ext_lib():
    from vbq_amd import build
    return build.build_ext()


@pytest.fixture(scope="module")
def spin():
    _need_gpu()
    sp, notes = SO.calibrate()
    print(f"\n[test_gpu_scores] {sp}: {notes}")
    return sp


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _table(rng, C, N):
    return np.sort(rng.normal(size=(C, 2 ** (N + 1) - 1)).astype(np.float32), axis=1)


def _pack(idx, N, total):
    from vbq_amd import ops
    st = torch.zeros(1, dtype=torch.uint32, device="cuda")
    words = ops.records_pack(_cuda(idx), total, N, status=st)
    assert int(st.cpu().item()) == 0
    return words


def _total_bits(K, N, kind):
    if kind != "mid":
        return 0 if kind == "zero" else K * N
    total = K * N // 3                                         # near a third, and the record ends inside a word
    while (K * N.bit_length() + total) % 32 == 0:
        total += 1
    return total


def _consumed(q, metric):
    """The queries as the Python layer hands them to the kernel (for the cosine divided by 1e-8 + |q| in torch): the
    restatement is about the C call, which takes queries as given."""
    from vbq_amd import embeddings as E
    return E._query_args(q, q.shape[1], metric, torch.device("cuda")).cpu().numpy()


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(i):
    """The record file, its dense twin, queries, ids and the restated rows of CASES[i]: built once for every test that asks."""
    from vbq_amd import bitstream as bs, embeddings as E
    K, Q, M, V, N, kind, per_column = CASES[i]
    c = Case()
    c.K, c.Q, c.M, c.V, c.N = K, Q, M, V, N
    c.total = _total_bits(K, N, kind)
    rng = np.random.default_rng(100 + i)
    c.table = _table(rng, K if per_column else 1, N)
    idx = RR.random_indices(rng, V, K, N, c.total)
    idx[7::7] = idx[6:-1:7][:len(idx[7::7])]                    # every seventh row repeats the row before it: ties
    c.words = _pack(idx, N, c.total)
    h = bs.RecordsHeader(N=N, shape=(V, K), C=c.table.shape[0], total_bits=c.total)
    c.rec = E.RecordEmbeddings(bs.write_records(h, c.table, c.words.cpu().numpy()))
    c.dense = c.rec.tensor()
    c.rows = SR.decode(c.words.cpu().numpy(), K, N, c.total, c.table)
    assert np.array_equal(_bits(c.dense), _bits(c.rows)), "the restated decode and tensor() differ"
    c.q = rng.standard_normal((Q, K)).astype(np.float32)
    c.ids = rng.integers(0, V, (Q, M)).astype(np.int64)
    c.rows.setflags(write=False)                                     # (q and ids go through torch.from_numpy: the tests copy them)
    return c


# ------------------------------------------------------------------------------------------------------------------ 1, 2
@gpu
@pytest.mark.parametrize("i", range(len(CASES)))
def test_both_sources_equal_the_exact_restatement(i):
    _need_gpu()
    from vbq_amd import embeddings as E
    c = _case(i)
    for metric in METRICS:
        want, st = SR.scores(_consumed(c.q, metric), c.rows, c.ids, metric)
        assert st == 0
        for ids in (c.ids, _cuda(c.ids)):                           # checked on the host; left to the kernel's status bit
            got_r, got_d = c.rec.scores(c.q, ids, metric), E.scores(c.dense, c.q, ids, metric)
            for got in (got_r, got_d):
                assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (c.Q, c.M)
            assert np.array_equal(_bits(got_r), _bits(want)), (CASES[i], metric, "records")
            assert np.array_equal(_bits(got_d), _bits(want)), (CASES[i], metric, "dense")


@gpu
@pytest.mark.parametrize("i", range(len(CASES)))
def test_record_source_equals_dense_source(i):
    """Through the C calls, queries as given (not normalised), and every row of the file listed for every query."""
    _need_gpu()
    from vbq_amd import ops
    c = _case(i)
    ids = _cuda(np.tile(np.arange(c.V, dtype=np.int64), (c.Q, 1)))
    q = _cuda(c.q)
    for metric in METRICS:
        st = torch.zeros(1, dtype=torch.uint32, device="cuda")
        a = ops.records_scores(c.words, c.K, c.N, c.total, _cuda(c.table), q, ids, metric, status=st)
        b = ops.scores(c.dense, q, ids, metric, status=st)
        assert int(st.cpu().item()) == 0 and np.array_equal(_bits(a), _bits(b)), (CASES[i], metric)


@gpu
@pytest.mark.parametrize("K", [40, 700])
def test_the_group_sizes_the_cases_do_not_reach(K):
    """CASES run groups of 64 (K = 1, 5), 16 (K = 64, 65, 100) and 8 pairs (K = 300, 512).  K = 40 takes 32, and K = 700 is 8
    again, past the K the search serves.  5 x 15 = 75 pairs: whole groups and a partial one."""
    _need_gpu()
    from vbq_amd import ops
    V, Q, M, N = 20, 5, 15, 3
    total = _total_bits(K, N, "mid")
    rng = np.random.default_rng(70)
    table = _table(rng, 1, N)
    words = _pack(RR.random_indices(rng, V, K, N, total), N, total)
    rows = SR.decode(words.cpu().numpy(), K, N, total, table)
    q, ids = rng.standard_normal((Q, K)).astype(np.float32), rng.integers(0, V, (Q, M)).astype(np.int64)
    for metric in METRICS:
        want, _ = SR.scores(q, rows, ids, metric)
        got = ops.records_scores(words, K, N, total, _cuda(table), _cuda(q), _cuda(ids), metric)
        assert np.array_equal(_bits(got), _bits(want))
        assert np.array_equal(_bits(ops.scores(_cuda(rows), _cuda(q), _cuda(ids), metric)), _bits(want))


# ------------------------------------------------------------------------------------------------------------------ 3
@gpu
@pytest.mark.parametrize("i", range(len(CASES)))
def test_scores_equal_the_scores_the_search_reports(i):
    """(ids, s) = most_similar(queries, k = min(V, 64)); scores(queries, ids) == s bit for bit, record file and dense matrix:
    the search's MFMA chain and the fmaf chain of one lane are the same chain."""
    _need_gpu()
    from vbq_amd import embeddings as E
    c = _case(i)
    k = min(c.V, 64)
    for metric in METRICS:
        ids, s = c.rec.most_similar(c.q, k=k, metric=metric)
        assert (ids >= 0).all()
        assert np.array_equal(_bits(c.rec.scores(c.q, ids, metric)), _bits(s)), (CASES[i], metric, "records")
        ids_d, s_d = E.most_similar(c.dense, c.q, k=k, metric=metric)
        assert np.array_equal(_bits(E.scores(c.dense, c.q, ids_d, metric)), _bits(s_d)), (CASES[i], metric, "dense")


@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("K,V,Q", [(1, 1, 1), (5, 33, 3), (65, 130, 2), (100, 33, 33), (300, 130, 1)])
def test_scores_equal_the_search_on_its_own_tied_data(K, V, Q, metric):
    """topk_reference.case_data: every seventh row repeats the row before it.  k = 64 > V leaves a -1 / -inf tail, which
    goes straight back in."""
    _need_gpu()
    from vbq_amd import embeddings as E
    emb, q, _ = TR.case_data(K, V, Q)
    ids, s = E.most_similar(emb, q, k=64, metric=metric)
    got = E.scores(emb, q, ids, metric)
    assert np.array_equal(_bits(got), _bits(s))
    assert (ids[:, min(V, 64):] == -1).all() and np.isneginf(got.cpu().numpy()[:, min(V, 64):]).all()


# ------------------------------------------------------------------------------------------------------------------ 4, 5, 6
@gpu
@pytest.mark.parametrize("i", [1, 4, 5, 10])
def test_result_does_not_depend_on_where_a_pair_stands(i):
    """Permuted columns permute the output; an id listed twice scores twice the same; the same pairs behind 5 more queries (a
    shift that is no multiple of any group size) keep their bits."""
    _need_gpu()
    from vbq_amd import embeddings as E
    c = _case(i)
    rng = np.random.default_rng(7)
    for metric in METRICS:
        for score in (c.rec.scores, lambda *a: E.scores(c.dense, *a)):
            base = _bits(score(c.q, c.ids, metric))
            perm = rng.permutation(c.M)
            assert np.array_equal(_bits(score(c.q, c.ids[:, perm], metric)), base[:, perm])
            twice = np.concatenate([c.ids, c.ids[:, ::-1], c.ids[:, :1]], axis=1)
            got = _bits(score(c.q, twice, metric))
            assert np.array_equal(got[:, :c.M], base) and np.array_equal(got[:, c.M:2 * c.M], base[:, ::-1])
            assert np.array_equal(got[:, -1], base[:, 0])
            lead_q = rng.standard_normal((5, c.K)).astype(np.float32)
            lead_ids = rng.integers(0, c.V, (5, c.M))
            got = _bits(score(np.concatenate([lead_q, c.q]), np.concatenate([lead_ids, c.ids]), "dot"))
            assert np.array_equal(got[5:], _bits(score(c.q, c.ids, "dot")))


# ------------------------------------------------------------------------------------------------------------------ 7
@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_padding_and_rows_out_of_range(metric, monkeypatch):
    _need_gpu()
    from vbq_amd import embeddings as E, ops
    c = _case(4)                                                     # K = 100, V = 33, 43 x 3 pairs
    q, table = _cuda(c.q), _cuda(c.table)
    ids = c.ids.copy()
    ids[::2, 1] = -1
    ids[5, 0] = -(1 << 40)
    want, st_want = SR.scores(c.q, c.rows, ids, metric)
    assert st_want == 0 and np.isneginf(want).sum() == 23
    for call in (lambda i, st: ops.records_scores(c.words, c.K, c.N, c.total, table, q, _cuda(i), metric, status=st),
                 lambda i, st: ops.scores(c.dense, q, _cuda(i), metric, status=st)):
        st = torch.zeros(1, dtype=torch.uint32, device="cuda")
        assert np.array_equal(_bits(call(ids, st)), _bits(want)) and int(st.cpu().item()) == 0     # padding sets no bit
        far = ids.copy()
        far[7, 2], far[42, 0] = c.V, 1 << 40
        want_far, st_far = SR.scores(c.q, c.rows, far, metric)
        assert np.array_equal(_bits(call(far, st)), _bits(want_far)) and int(st.cpu().item()) == st_far == 8
        assert call(far, None) is not None                          # d_status may be NULL
    # through Python: host ids are refused before any device work, a device tensor after the launch
    far = ids.copy()
    far[7, 2] = c.V
    launches = []
    real = (ops.records_scores, ops.scores)
    monkeypatch.setattr(ops, "records_scores", lambda *a, **k: launches.append("records") or real[0](*a, **k))
    monkeypatch.setattr(ops, "scores", lambda *a, **k: launches.append("dense") or real[1](*a, **k))
    for score in (lambda i: c.rec.scores(c.q, i, metric), lambda i: c.rec.rerank(c.q, i, metric=metric),
                  lambda i: E.scores(c.dense, c.q, i, metric), lambda i: E.rerank(c.dense, c.q, i, metric=metric)):
        with pytest.raises(IndexError, match="outside"):
            score(far)
        with pytest.raises(IndexError, match="outside"):
            score(far.tolist())
        assert launches == []
        with pytest.raises(IndexError, match="outside"):
            score(_cuda(far))
        assert len(launches) == 1
        launches.clear()
    want, _ = SR.scores(_consumed(c.q, metric), c.rows, ids, metric)
    for i in (ids, _cuda(ids)):                                     # padding alone raises nothing, in either form
        assert np.array_equal(_bits(c.rec.scores(c.q, i, metric)), _bits(want))
        assert np.array_equal(_bits(E.scores(c.dense, c.q, i, metric)), _bits(want))


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_a_damaged_record_scores_as_the_zero_row(metric):
    """Each of the three damages (a length field above N, lengths that do not add up, non-zero padding) on a file of K = 12,
    V = 40: the status word is the unpack's, the damaged row scores +-0, and every score is that of the dense matrix with
    that row zeroed -- the pairs beside it in the group are unaffected."""
    _need_gpu()
    from vbq_amd import ops
    N, K, V, Q, row = 10, 12, 40, 3, 23
    total = _total_bits(K, N, "mid")
    rng = np.random.default_rng(13)
    tab = _cuda(_table(rng, 1, N))
    words = _pack(RR.random_indices(rng, V, K, N, total), N, total)
    q = _cuda(rng.standard_normal((Q, K)).astype(np.float32))
    ids = _cuda(np.stack([rng.permutation(V) for _ in range(Q)]).astype(np.int64))
    dense = ops.records_unpack(words, K, N, total, tab)[0]
    dense[row] = 0.0
    want = ops.scores(dense, q, ids, metric)
    clean = words.cpu().numpy()
    assert (K * N.bit_length() + total) % 32 and clean.shape[1] == RR.record_words(K, N, total)
    for bit in (1, 2, 4):
        w = clean.copy()
        n0 = int(w[row, 0] & 0xF)
        if bit == 1:                                            # a length field > N
            w[row, 0] = (w[row, 0] & ~np.uint32(0xF)) | np.uint32(0xD)
        elif bit == 2:                                          # a valid length, but the lengths no longer add up
            w[row, 0] = (w[row, 0] & ~np.uint32(0xF)) | np.uint32(n0 + 1 if n0 < N else n0 - 1)
        else:                                                   # the last padding bit
            w[row, -1] |= np.uint32(1 << 31)
        damaged = _cuda(w.view(np.int32)).view(torch.uint32)
        st = torch.zeros(1, dtype=torch.uint32, device="cuda")
        got = ops.records_scores(damaged, K, N, total, tab, q, ids, metric, status=st)
        st_unpack = torch.zeros(1, dtype=torch.uint32, device="cuda")
        ops.records_unpack(damaged, K, N, total, None, want_values=False, status=st_unpack)
        st, st_unpack = int(st.cpu().item()), int(st_unpack.cpu().item())
        assert st == st_unpack and st & bit, (bit, st, st_unpack)
        assert np.array_equal(_bits(got), _bits(want))
        at = (ids == row).cpu().numpy()
        assert at.sum() == Q and (got.cpu().numpy()[at] == 0.0).all()


# ------------------------------------------------------------------------------------------------------------------ 8
@gpu
@pytest.mark.parametrize("i", [4, 5, 8])
def test_rerank_is_the_searchs_order_over_the_exact_scores(i):
    _need_gpu()
    from vbq_amd import embeddings as E
    c = _case(i)
    ids = c.ids.copy()
    ids[::2, c.M // 2] = -1                                          # padding in the middle; the random ids repeat anyway
    ids[:, -1] = ids[:, 0]
    for metric in METRICS:
        exact, _ = SR.scores(_consumed(c.q, metric), c.rows, ids, metric)
        want_ids = np.full(ids.shape, -1, np.int64)
        want_s = np.full(ids.shape, -np.inf, np.float32)
        for r in range(c.Q):
            ok = ids[r] >= 0
            by_row = np.zeros(c.V, np.float32)
            by_row[ids[r, ok]] = exact[r, ok]
            best = TR.order(by_row, ids[r, ok])
            want_ids[r, :best.size], want_s[r, :best.size] = best, by_row[best]
        for rerank in (c.rec.rerank, lambda *a, **k: E.rerank(c.dense, *a, **k)):
            got_ids, got_s = rerank(c.q, ids, metric=metric)
            assert got_ids.dtype == torch.int64 and np.array_equal(got_ids.cpu().numpy(), want_ids)
            assert np.array_equal(_bits(got_s), _bits(want_s))
            k = min(2, c.M)
            got_ids, got_s = rerank(c.q, _cuda(ids), k, metric)
            assert np.array_equal(got_ids.cpu().numpy(), want_ids[:, :k]) and np.array_equal(_bits(got_s), _bits(want_s[:, :k]))


@gpu
@pytest.mark.parametrize("i", [4, 5])
def test_rerank_of_a_search_result_returns_it_unchanged(i):
    """most_similar(k = 64) over V = 33 rows (a -1 / -inf tail) and over V = 130 rows (the 64 best)."""
    _need_gpu()
    from vbq_amd import embeddings as E
    c = _case(i)
    for metric in METRICS:
        for search, rerank in ((c.rec.most_similar, c.rec.rerank),
                               (lambda *a, **k: E.most_similar(c.dense, *a, **k), lambda *a, **k: E.rerank(c.dense, *a, **k))):
            ids, s = search(c.q, k=64, metric=metric)
            got_ids, got_s = rerank(c.q, ids, metric=metric)
            assert torch.equal(got_ids, ids) and np.array_equal(_bits(got_s), _bits(s))
            assert bool((ids[:, -1] == -1).all()) == (c.V < 64)


# ------------------------------------------------------------------------------------------------------------------ 9
@gpu
@pytest.mark.parametrize("offset", [0, 1])
def test_write_footprint(offset):
    """d_out between canaries, aligned and one element off; 43 x 3 = 129 pairs, no multiple of 64; both sources."""
    _need_gpu()
    from vbq_amd import _lib, _lib_ext, ops
    c = _case(4)
    assert (c.Q * c.M) % 64
    q, table = FP.shifted(c.q, offset, "cuda"), _cuda(c.table)
    ids = c.ids.copy()
    ids[3, 1], ids[42, 2] = -1, c.V                                  # -inf is a written value too
    ids = FP.shifted(ids, offset, "cuda")
    canary = FP.canary(torch.float32)
    for call in (lambda out: ops.records_scores(c.words, c.K, c.N, c.total, table, q, ids, "cosine", out=out),
                 lambda out: ops.scores(c.dense, q, ids, "cosine", out=out)):
        g = FP.Guarded((c.Q, c.M), torch.float32, "cuda", offset)
        want = call(None)
        assert call(g.view) is g.view
        g.assert_outside_intact("scores")
        assert (g.bits() != canary).all(), "an element of d_out was not written"
        assert np.array_equal(g.bits(), _bits(want))
    # a refused call leaves the whole buffer as it was: a metric the C call does not know, a K above the LDS limit
    g = FP.Guarded((c.Q, c.M), torch.float32, "cuda", offset)
    h = _lib_ext.lib()
    rc = h.vbqx_scores_f32(ops._ptr(c.dense), c.V, c.K, ops._ptr(q), c.Q, ops._ptr(ids), c.M, 7, g.ptr, None, ops._stream(c.dense))
    assert rc == -1 and b"metric 7" in h.vbqx_last_error()
    wide = torch.zeros((2, 20000), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.VBQError, match="every K <= 3500 fits"):
        ops.scores(wide, wide, ids[:2].clamp(0, 1), "dot", out=FP.Guarded((2, c.M), torch.float32, "cuda").view)
    rc = h.vbqx_records_scores_f32(ops._ptr(c.words), c.V, c.K, c.N, c.total, ops._ptr(table), 1, ops._ptr(q), c.Q, None, c.M, 1,
                                   g.ptr, None, ops._stream(c.dense))
    assert rc == -1 and b"null pointer" in h.vbqx_last_error()
    torch.cuda.synchronize()
    g.assert_untouched("refused scores")


# ------------------------------------------------------------------------------------------------------------------ 10
def _late_inputs(c, seed):
    rng = np.random.default_rng(seed)
    return [_cuda(rng.standard_normal((c.Q, c.K)).astype(np.float32)), _cuda(rng.integers(0, c.V, (c.Q, c.M)).astype(np.int64))]


@gpu
@pytest.mark.parametrize("name", ["ops.records_scores", "ops.scores"])
def test_the_c_calls_are_ordered_on_the_callers_stream_and_do_not_synchronize(name, spin):
    """Armed: the queries and ids arrive late on a side stream, and the call returns while the delay is still running."""
    _need_gpu()
    from vbq_amd import ops
    c = _case(4)
    table = _cuda(c.table)
    call = {"ops.records_scores": lambda b: ops.records_scores(c.words, c.K, c.N, c.total, table, b[0], b[1], "cosine"),
            "ops.scores": lambda b: ops.scores(c.dense, b[0], b[1], "cosine")}[name]
    late = SO.run_late(call, _late_inputs(c, 7), _late_inputs(c, SO.STALE_SEED), blocking=False, spin=spin, name=name)
    assert late.armed


@gpu
@pytest.mark.parametrize("source", ["records", "dense"])
@pytest.mark.parametrize("name", ["scores", "similarity", "rerank"])
def test_the_python_calls_are_ordered_on_the_callers_stream(name, source, spin):
    """Not armed (the module docstring says why): late queries and ids on a side stream, the exact answer."""
    _need_gpu()
    from vbq_amd import embeddings as E
    c = _case(4)
    on = c.rec if source == "records" else None
    fn = getattr(on, name) if on is not None else functools.partial(getattr(E, name), c.dense)
    call = {"scores": lambda b: fn(b[0], b[1]), "rerank": lambda b: fn(b[0], b[1], 2, "dot"),
            "similarity": lambda b: fn(b[1][:, 0], b[1][:, 1])}[name]
    SO.run_late(call, _late_inputs(c, 7), _late_inputs(c, SO.STALE_SEED), blocking=True, spin=spin, name=f"{source}.{name}")


# ------------------------------------------------------------------------------------------------------------------ 11
@gpu
def test_no_gathered_matrix_exists():
    """P = 4096 pairs at K = 300: the rows alone would be P K 4 = 4.9 MB; the call's peak stays below half of that."""
    _need_gpu()
    from vbq_amd import embeddings as E
    c = _case(5)                                                     # K = 300, V = 130
    Q, M = 4, 1024
    rng = np.random.default_rng(3)
    q, ids = _cuda(rng.standard_normal((Q, c.K)).astype(np.float32)), _cuda(rng.integers(0, c.V, (Q, M)).astype(np.int64))
    for score in (c.rec.scores, functools.partial(E.scores, c.dense)):
        score(q, ids)                                                # the library is loaded, the allocator warm
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = score(q, ids)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
        assert tuple(out.shape) == (Q, M) and rise < Q * M * c.K * 4 // 2, rise
        # where rows(ids) + a torch reduction holds the gathered matrix
        torch.cuda.reset_peak_memory_stats()
        rows = c.rec.rows(ids.reshape(-1))
        assert torch.cuda.max_memory_allocated() - before >= Q * M * c.K * 4 and rows.numel() == Q * M * c.K
