"""The fused nearest-row search (vbq_topk.hip) on the GPU: the dense source against the float64 restatement through its acceptance
rule (tests/topk_reference.py), the record source against the dense source bit for bit, the result's independence of the grid,
ties, exclusions, damaged records and the Python layer's refusals.  Record files are built from synthetic rank indices
(tests/records_reference.py) and the pack kernel, as the record tests do, so nothing here depends on the budget DP."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import records_reference as RR  # noqa: E402
import topk_reference as TR  # noqa: E402

gpu = pytest.mark.gpu
METRICS = ("dot", "cosine")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _table(rng, C, N):
    return np.sort(rng.normal(size=(C, 2 ** (N + 1) - 1)).astype(np.float32), axis=1)


def _pack(idx, N, total):
    from vbq_amd import ops
    st = torch.zeros(1, dtype=torch.uint32, device="cuda")
    words = ops.records_pack(_cuda(idx), total, N, status=st)
    assert int(st.cpu().item()) == 0
    return words


def _record_file(idx, N, total, table):
    """The "VBQr" bytes of rank indices [V, K] and a table f32 [C, T] in rank order."""
    from vbq_amd import bitstream as bs
    h = bs.RecordsHeader(N=N, shape=tuple(idx.shape), C=table.shape[0], total_bits=total)
    return bs.write_records(h, table, _pack(idx, N, total).cpu().numpy())


def _as_consumed(q, metric):
    """The queries as the Python layer hands them to the kernel (for the cosine divided by 1e-8 + |q| in float32 torch ops):
    the acceptance rule is about the C call, which takes queries as given."""
    from vbq_amd import embeddings as E
    return E._search_args(q, q.shape[1], 1, metric, None, torch.device("cuda"))[0].cpu().numpy()


def _mid_word(K, N):
    """A total_bits near K * N / 3 at which the record ends inside a word."""
    total = K * N // 3
    while (K * N.bit_length() + total) % 32 == 0:
        total += 1
    return total


@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("K,V,Q,k", TR.CASES)
def test_dense_source_is_accepted_by_the_float64_reference(K, V, Q, k, metric):
    _need_gpu()
    from vbq_amd import ops
    emb, q, exclude = TR.case_data(K, V, Q)
    for ex in (None, exclude):
        ids, scores = ops.topk(_cuda(emb), _cuda(q), k, metric, None if ex is None else _cuda(ex))
        assert ids.dtype == torch.int64 and scores.dtype == torch.float32 and ids.is_cuda and scores.is_cuda
        TR.accept(ids.cpu().numpy(), scores.cpu().numpy(), q, emb, k, metric, ex)


@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("per_column", [False, True])
@pytest.mark.parametrize("K,total", [(12, None), (12, 0), (65, None), (300, None)])
def test_record_source_equals_dense_source_bit_for_bit(K, total, per_column, metric):
    """The same chain and the same order: identical ids and identical score bits.  V = 200 is a whole tile of 128 rows and a
    partial one; Q = 33 a second block of queries."""
    _record_source_equals_dense_source(K, 10, total, per_column, metric)


@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("per_column", [False, True])
@pytest.mark.parametrize("N", [1, 3])
def test_record_source_equals_dense_source_at_short_length_fields(N, per_column, metric):
    """Length fields of W = 1 and W = 2 bits (the test above has W = 4 only) at K = 65: one whole chunk of 64 coordinates and a
    carry into the second.  At N = 1 the code book has three entries; the order (score descending, id ascending) is total, so
    the comparison stays exact, and the float64 reference accepts its own result on this data (no two of the 200 rows are
    equal, no row is all zeros)."""
    _record_source_equals_dense_source(65, N, None, per_column, metric)


def _record_source_equals_dense_source(K, N, total, per_column, metric):
    _need_gpu()
    from vbq_amd import embeddings as E
    V, Q, k = 200, 33, 64
    total = _mid_word(K, N) if total is None else total
    rng = np.random.default_rng(K + total)
    table = _table(rng, K if per_column else 1, N)
    rec = E.RecordEmbeddings(_record_file(RR.random_indices(rng, V, K, N, total), N, total, table))
    q = rng.standard_normal((Q, K)).astype(np.float32)
    dense = rec.tensor()
    ids, scores = rec.most_similar(q, k=k, metric=metric)
    want_ids, want_scores = E.most_similar(dense, q, k=k, metric=metric)
    assert torch.equal(ids, want_ids)
    assert torch.equal(scores.view(torch.int32), want_scores.view(torch.int32))
    if total:                                                   # total_bits = 0: every row is the same, ids 0 .. k-1 lead
        TR.accept(ids.cpu().numpy(), scores.cpu().numpy(), _as_consumed(q, metric), dense.cpu().numpy(), k, metric)
    else:
        assert torch.equal(ids, torch.arange(k, device="cuda").expand(Q, k))
    # ids= queries with the rows themselves and leaves each one's own row out
    own = [V - 1, 0, 130]
    ids2, scores2 = rec.most_similar(ids=own, k=5, metric=metric)
    ex = _cuda(np.array(own, np.int64)[:, None])
    want_ids, want_scores = E.most_similar(dense, dense[own], k=5, metric=metric, exclude=ex)
    assert torch.equal(ids2, want_ids) and torch.equal(scores2.view(torch.int32), want_scores.view(torch.int32))
    assert not (ids2 == ex).any()


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_result_does_not_depend_on_the_grid(metric):
    _need_gpu()
    from vbq_amd import ops
    K, V, Q, k = 100, 2500, 33, 64
    emb, q, exclude = TR.case_data(K, V, Q)
    e, qq, ex = _cuda(emb), _cuda(q), _cuda(exclude)
    got = [ops.topk(e, qq, k, metric, ex, max_workgroups=m) for m in (1, 3, 0)]
    for ids, scores in got[1:]:
        assert torch.equal(ids, got[0][0]) and torch.equal(scores.view(torch.int32), got[0][1].view(torch.int32))
    # and the record source: K = 65, the tile of 128 rows split 1, 3 and as many ways as the device takes
    N, K = 10, 65
    total = _mid_word(K, N)
    rng = np.random.default_rng(11)
    table = _cuda(_table(rng, 1, N))
    words = _pack(RR.random_indices(rng, V, K, N, total), N, total)
    qq = _cuda(rng.standard_normal((Q, K)).astype(np.float32))
    got = [ops.records_topk(words, K, N, total, table, qq, k, metric, max_workgroups=m) for m in (1, 3, 0)]
    for ids, scores in got[1:]:
        assert torch.equal(ids, got[0][0]) and torch.equal(scores.view(torch.int32), got[0][1].view(torch.int32))


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_ties_lead_in_ascending_id_and_exclusions_remove_them(metric):
    """Rows 7, 900 and 2499 are copies of row 3: identical rows give identical score bits."""
    _need_gpu()
    from vbq_amd import embeddings as E
    N, K, V = 10, 12, 2500
    total = _mid_word(K, N)
    rng = np.random.default_rng(12)
    idx = RR.random_indices(rng, V, K, N, total)
    idx[[7, 900, 2499]] = idx[3]
    rec = E.RecordEmbeddings(_record_file(idx, N, total, _table(rng, 1, N)))
    q = rec.rows([3])
    k = 10 if metric == "cosine" else 64
    ids, scores = rec.most_similar(q, k=k, metric=metric)
    ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
    if metric == "cosine":                                      # for the dot product a longer row may score higher still
        assert ids[0, :4].tolist() == [3, 7, 900, 2499]
        assert len(set(scores[0, :4].view(np.int32).tolist())) == 1 and scores[0, 4] < scores[0, 3]
    else:
        at = np.flatnonzero(np.isin(ids[0], [3, 7, 900, 2499]))
        assert ids[0, at].tolist() == [3, 7, 900, 2499] and at.tolist() == list(range(at[0], at[0] + 4))
        assert len(set(scores[0, at].view(np.int32).tolist())) == 1
    TR.accept(ids, scores, _as_consumed(q, metric), rec.tensor().cpu().numpy(), k, metric)
    ids3 = rec.most_similar(ids=[3], k=k, metric=metric)[0].cpu().numpy()
    assert ids3[0].tolist() == [i for i in ids[0].tolist() if i != 3] + ids3[0, -1:].tolist()
    if metric == "cosine":
        assert ids3[0, :3].tolist() == [7, 900, 2499]
    ids4 = rec.most_similar(ids=[3], k=k, metric=metric, exclude=[[900]])[0].cpu().numpy()
    assert ids4[0].tolist() == [i for i in ids3[0].tolist() if i != 900] + ids4[0, -1:].tolist()
    if metric == "cosine":
        assert ids4[0, :2].tolist() == [7, 2499]
    # k beyond the rows that are left: V = 3, the query's own row and one more excluded
    small = E.RecordEmbeddings(_record_file(idx[:3], N, total, _table(rng, 1, N)))
    i5, s5 = small.most_similar(ids=[1], k=4, metric=metric, exclude=[[0]])
    assert i5.cpu().numpy().tolist() == [[2, -1, -1, -1]] and np.isneginf(s5.cpu().numpy()[0, 1:]).all()


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_a_damaged_record_scores_as_the_zero_row(metric):
    """Through the C call.  The table holds 0.0 at the rank of code 0 of every length, so a record whose codes are all 0 really
    decodes to zeros: the file with that row and the file whose row 17 has a length field above N give the same result, and only
    the second sets the status bit.  Then each of the three damages (a length field above N, lengths that do not add up,
    non-zero padding) on a file of K = 12, V = 40: the status word is the unpack's, the result that of the dense matrix with the
    row zeroed."""
    _need_gpu()
    from vbq_amd import ops
    N, K, V, Q, k = 10, 65, 150, 3, 64
    total = _mid_word(K, N)
    rng = np.random.default_rng(13)
    table = _table(rng, 1, N)
    zero_ranks = RR.rank_of(np.arange(N + 1), np.zeros(N + 1, np.int64), N)
    table[0, zero_ranks] = 0.0
    idx = RR.random_indices(rng, V, K, N, total)
    n, _ = RR.length_and_code(idx[17], N)
    idx[17] = RR.rank_of(n, np.zeros(K, np.int64), N)
    words = _pack(idx, N, total)
    q = _cuda(-np.abs(rng.standard_normal((Q, K))).astype(np.float32))
    q[1] = -q[1]
    q[2] = 0.0                                                  # every score +-0: ids 0 .. k-1 lead, row 17 among them

    def run(w):
        st = torch.zeros(1, dtype=torch.uint32, device="cuda")
        ids, scores = ops.records_topk(w, K, N, total, _cuda(table), q, k, metric, status=st)
        return ids.cpu().numpy(), scores.cpu().numpy(), int(st.cpu().item())

    ids, scores, st = run(words)
    assert st == 0
    at = np.argwhere(ids == 17)
    assert 2 in at[:, 0] and all(scores[i, j] == 0.0 for i, j in at)               # the zero row takes part, with score 0
    w = words.cpu().numpy().copy()
    assert w[17, 0] & 0xF <= N
    w[17, 0] = (w[17, 0] & ~np.uint32(0xF)) | np.uint32(0xD)
    damaged = _cuda(w.view(np.int32)).view(torch.uint32)
    ids2, scores2, st2 = run(damaged)
    st = torch.zeros(1, dtype=torch.uint32, device="cuda")
    ops.records_unpack(damaged, K, N, total, None, want_values=False, status=st)
    assert st2 & 1 and st2 == int(st.cpu().item())              # the unpack's bits (the lengths no longer add up either)
    assert np.array_equal(ids2, ids) and scores2.tobytes() == scores.tobytes()
    # every bit set: every record fails, every row scores +-0, the ids lead in ascending order
    ids3, scores3, st3 = run(_cuda(np.full_like(w, 0xFFFFFFFF).view(np.int32)).view(torch.uint32))
    assert st3 & 1 and np.array_equal(ids3, np.tile(np.arange(k), (Q, 1))) and not scores3.any()
    # each damage on a small file of its own: the unpack's status word, and the result of the dense matrix with that row zeroed
    K, V, k, row = 12, 40, 40, 23
    total = _mid_word(K, N)
    tab = _cuda(_table(rng, 1, N))
    words = _pack(RR.random_indices(rng, V, K, N, total), N, total)
    q = _cuda(rng.standard_normal((Q, K)).astype(np.float32))
    dense = ops.records_unpack(words, K, N, total, tab)[0]
    dense[row] = 0.0
    want_ids, want_scores = ops.topk(dense, q, k, metric)
    clean = words.cpu().numpy()
    end = K * N.bit_length() + total
    assert end % 32 and clean.shape[1] == RR.record_words(K, N, total)
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
        st_topk = torch.zeros(1, dtype=torch.uint32, device="cuda")
        got_ids, got_scores = ops.records_topk(damaged, K, N, total, tab, q, k, metric, status=st_topk)
        st_unpack = torch.zeros(1, dtype=torch.uint32, device="cuda")
        ops.records_unpack(damaged, K, N, total, None, want_values=False, status=st_unpack)
        st_topk, st_unpack = int(st_topk.cpu().item()), int(st_unpack.cpu().item())
        assert st_topk == st_unpack and st_unpack & bit, (bit, st_topk, st_unpack)
        assert torch.equal(got_ids, want_ids) and torch.equal(got_scores.view(torch.int32), want_scores.view(torch.int32))


@gpu
def test_python_layer_refuses_what_the_contract_excludes():
    _need_gpu()
    import vbq_amd
    from vbq_amd import embeddings as E
    N, K, V = 10, 12, 40
    total = _mid_word(K, N)
    rng = np.random.default_rng(14)
    rec = E.RecordEmbeddings(_record_file(RR.random_indices(rng, V, K, N, total), N, total, _table(rng, 1, N)))
    dense = rec.tensor()
    q = rng.standard_normal((2, K)).astype(np.float32)
    ids, scores = rec.most_similar(q[0])                                            # [K] is one query; k = 10, cosine
    assert tuple(ids.shape) == (1, 10) and tuple(scores.shape) == (1, 10)
    assert torch.equal(ids, rec.most_similar(torch.from_numpy(q[:1]).cuda())[0])
    assert torch.equal(ids, E.most_similar(dense.cpu().numpy(), q[0])[0])
    with pytest.raises(ValueError, match="exactly one"):
        rec.most_similar()
    with pytest.raises(ValueError, match="exactly one"):
        rec.most_similar(q, ids=[1])
    for bad in ([V], [-1]):
        with pytest.raises(IndexError, match="outside"):
            rec.most_similar(ids=bad)
    for search in (rec.most_similar, lambda *a, **kw: E.most_similar(dense, *a, **kw)):
        for kk in (0, 65):
            with pytest.raises(ValueError, match="outside 1..64"):
                search(q, k=kk)
        with pytest.raises(ValueError, match="metric"):
            search(q, metric="l2")
        with pytest.raises(ValueError, match="queries must be"):
            search(q[:, :K - 1])
        with pytest.raises(ValueError, match="queries must be"):
            search(q[None])
        with pytest.raises(ValueError, match="exclude"):
            search(q, exclude=np.zeros((2, 9), np.int64))
        with pytest.raises(ValueError, match="exclude"):
            search(q, exclude=np.zeros((3, 1), np.int64))
        for poison in (np.nan, np.inf):
            bad = q.copy()
            bad[1, 3] = poison
            with pytest.raises(ValueError, match="NaN or an infinity"):
                search(bad)
    with pytest.raises(ValueError, match="at most 7"):
        rec.most_similar(ids=[1, 2], exclude=np.zeros((2, 8), np.int64))
    assert rec.most_similar(ids=[1, 2], exclude=np.full((2, 7), -1))[0].shape == (2, 10)
    with pytest.raises(ValueError, match=r"\[V, K\]"):
        E.most_similar(dense.reshape(-1), q)
    with pytest.raises(vbq_amd.VBQError, match="limit is 163840"):
        E.most_similar(torch.zeros((4, 700), device="cuda"), np.zeros(700, np.float32))
