"""The pooled lookup (vbq_bag.hip) on the GPU: the dense source against the NumPy float32 restatement (tests/bag_reference.py)
bit for bit, the record source against the dense source bit for bit, both sides of the code book's LDS / L2 choice, a launch
whose bag loop takes a second trip, the two forms of the ids, damaged records, ids past the matrix, damaged offsets and the
Python layer's refusals.  Record files are built from synthetic rank indices (tests/records_reference.py) and the pack kernel,
as the search's tests do, so nothing here depends on the budget DP."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bag_reference as BR  # noqa: E402
import records_reference as RR  # noqa: E402

gpu = pytest.mark.gpu
V = 40
VARIANTS = ("sum", "mean", "max", "weighted")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u32(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _table(rng, C, N):
    return np.sort(rng.normal(size=(C, 2 ** (N + 1) - 1)).astype(np.float32), axis=1)


def _pack(idx, N, total):
    from vbq_amd import ops
    st = torch.zeros(1, dtype=torch.uint32, device="cuda")
    words = ops.records_pack(_cuda(idx), total, N, status=st)
    assert int(st.cpu().item()) == 0
    return words


def _mid_word(K, N):
    """A total_bits near K * N / 3 at which the record ends inside a word."""
    total = K * N // 3
    while (K * N.bit_length() + total) % 32 == 0:
        total += 1
    return total


def _bag_list(long_bags=1):
    """(ids, offsets [B + 1], weights) over V rows: an empty bag first, in the middle and last, a bag of one, a bag with a
    repeated id, an all-padding bag, padding between real ids, `long_bags` bags of 130 entries (more than one chunk of 64 ids)."""
    rng = np.random.default_rng(1000 + long_bags)
    bags = [[], [3], [5, 5, 7, 5], [-1, -1, -1], [2, -1, 9, -1, -9, 4], [], [V - 1, 0]]
    bags += [rng.integers(0, V, 130).tolist() for _ in range(long_bags)] + [[]]
    ids = np.array([i for b in bags for i in b], np.int64)
    offsets = np.concatenate([[0], np.cumsum([len(b) for b in bags])]).astype(np.int64)
    return ids, offsets, rng.standard_normal(ids.size).astype(np.float32)


def _kw(variant, weights):
    return dict(mode="sum", weights=weights) if variant == "weighted" else dict(mode=variant)


@functools.lru_cache(maxsize=None)
def _dense_case(K):
    """(emb f32 [V, K], the bag list, {variant: the reference's result}) -- computed once, shared, never written to."""
    emb = np.random.default_rng(K).standard_normal((V, K)).astype(np.float32)
    emb[7, : K // 2] = emb[5, : K // 2]                                   # ties for the max within the repeated-id bag
    ids, offsets, weights = _bag_list()
    want = {}
    for v in VARIANTS:
        want[v], st = BR.bag(emb, ids, offsets, **_kw(v, weights))
        assert st == 0
    return emb, (ids, offsets, weights), want


def _table_in_lds(n_ids, n_bags, K, N, n_tables=1):
    """The library's rule (vbq_bag.hip): one wave per bag on a grid of at most 16 workgroups per CU; the one code book goes to
    LDS once a workgroup decodes, on average, four coordinates per table entry it would load."""
    grid = min(n_bags, 16 * torch.cuda.get_device_properties(0).multi_processor_count)
    return n_tables == 1 and -(-n_ids // grid) * K >= 4 * (2 ** (N + 1) - 1)


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("K", [12, 65, 300])
def test_dense_source_equals_the_reference_bit_for_bit(K, variant):
    _need_gpu()
    from vbq_amd import ops
    emb, (ids, offsets, weights), want = _dense_case(K)
    st = torch.zeros(1, dtype=torch.uint32, device="cuda")
    kw = _kw(variant, weights)
    if kw.get("weights") is not None:
        kw["weights"] = _cuda(weights)
    out = ops.bag(_cuda(emb), _cuda(ids), _cuda(offsets), status=st, **kw)
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == (offsets.size - 1, K)
    assert int(st.cpu().item()) == 0
    assert np.array_equal(_u32(out), want[variant].view(np.uint32))


@gpu
def test_weighted_sum_rounds_the_product_before_it_adds():
    """The case of tests/test_bag_host.py on which a contracted multiply-add gives another float."""
    _need_gpu()
    from vbq_amd import ops
    emb, ids, offsets, weights, want = BR.contraction_case()
    out = ops.bag(_cuda(emb), _cuda(ids), _cuda(offsets), weights=_cuda(weights))
    assert _u32(out).tolist() == [[int(np.float32(want).view(np.uint32))]]


def _record_case(K, N, total, per_column, long_bags=1):
    """(words, table on the device, dense = the decoded matrix, the bag list on the device and on the host)."""
    from vbq_amd import ops
    total = _mid_word(K, N) if total is None else total
    rng = np.random.default_rng(K + total + N)
    table = _cuda(_table(rng, K if per_column else 1, N))
    words = _pack(RR.random_indices(rng, V, K, N, total), N, total)
    dense = ops.records_unpack(words, K, N, total, table)[0]
    return words, table, dense, total, _bag_list(long_bags)


def _record_source_equals_dense_source(K, N, total, per_column, long_bags=1):
    from vbq_amd import ops
    words, table, dense, total, (ids, offsets, weights) = _record_case(K, N, total, per_column, long_bags)
    i, o, w = _cuda(ids), _cuda(offsets), _cuda(weights)
    for variant in VARIANTS:
        kw = _kw(variant, w)
        st = torch.zeros(1, dtype=torch.uint32, device="cuda")
        got = ops.records_bag(words, K, N, total, table, i, o, status=st, **kw)
        assert int(st.cpu().item()) == 0
        assert np.array_equal(_u32(got), _u32(ops.bag(dense, i, o, **kw))), variant
    return dense, (ids, offsets, weights), got


@gpu
@pytest.mark.parametrize("per_column", [False, True])
@pytest.mark.parametrize("K,total", [(12, None), (12, 0), (65, None), (65, 0), (300, None), (300, 0)])
def test_record_source_equals_dense_source_bit_for_bit(K, total, per_column):
    _need_gpu()
    _record_source_equals_dense_source(K, 10, total, per_column)


@gpu
@pytest.mark.parametrize("per_column", [False, True])
@pytest.mark.parametrize("N", [1, 3])
def test_record_source_equals_dense_source_at_short_length_fields(N, per_column):
    """Length fields of W = 1 and W = 2 bits at K = 65: one whole chunk of 64 coordinates and a carry into the second."""
    _need_gpu()
    _record_source_equals_dense_source(65, N, None, per_column)


@gpu
def test_both_sides_of_the_code_book_choice():
    """K = 300, N = 10, one code book of 2047 entries: the bag list with one bag of 130 entries reads it through L2, the list
    with three such bags keeps it in LDS (the library's rule, restated in _table_in_lds).  Either way the records give what the
    dense matrix gives, and that is the reference's result."""
    _need_gpu()
    K, N = 300, 10
    sides = set()
    for long_bags in (1, 3):
        ids, offsets, _ = _bag_list(long_bags)
        sides.add(bool(_table_in_lds(ids.size, offsets.size - 1, K, N)))
        dense, _, got = _record_source_equals_dense_source(K, N, None, False, long_bags)      # `got`: the weighted sum
        want, st = BR.bag(dense.cpu().numpy(), ids, offsets, weights=_bag_list(long_bags)[2])
        assert st == 0 and np.array_equal(_u32(got), want.view(np.uint32))
    assert sides == {False, True}
    assert _table_in_lds(150, 9, 65, 3) and not _table_in_lds(150, 9, 300, 10, n_tables=300)


@gpu
def test_more_bags_than_workgroups():
    """5000 bags of at most 3 ids at K = 12: the grid holds 16 workgroups per CU (4096 on 256 CUs), so the bag loop takes a second
    trip.  Dense against the reference, records against dense."""
    _need_gpu()
    from vbq_amd import ops
    K, N, B = 12, 10, 5000
    assert B > 16 * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(5)
    sizes = rng.integers(0, 4, B)
    ids = rng.integers(-1, V, int(sizes.sum())).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    words, table, dense, total, _ = _record_case(K, N, None, False)
    i, o = _cuda(ids), _cuda(offsets)
    for mode in BR.MODES:
        got = ops.bag(dense, i, o, mode=mode)
        want, st = BR.bag(dense.cpu().numpy(), ids, offsets, mode=mode)
        assert st == 0 and np.array_equal(_u32(got), want.view(np.uint32)), mode
        assert np.array_equal(_u32(ops.records_bag(words, K, N, total, table, i, o, mode=mode)), _u32(got)), mode


def _record_file(idx, N, total, table):
    from vbq_amd import bitstream as bs
    h = bs.RecordsHeader(N=N, shape=tuple(idx.shape), C=table.shape[0], total_bits=total)
    return bs.write_records(h, table, _pack(idx, N, total).cpu().numpy())


@gpu
def test_flat_ids_with_offsets_and_padded_rows_give_the_same():
    _need_gpu()
    from vbq_amd import embeddings as E
    K, N = 65, 10
    total = _mid_word(K, N)
    rng = np.random.default_rng(6)
    rec = E.RecordEmbeddings(_record_file(RR.random_indices(rng, V, K, N, total), N, total, _table(rng, 1, N)))
    dense = rec.tensor()
    ids, offsets, weights = _bag_list()
    two = BR.padded(ids, offsets)
    w2 = np.zeros(two.shape, np.float32)
    for b in range(offsets.size - 1):
        w2[b, :offsets[b + 1] - offsets[b]] = weights[offsets[b]:offsets[b + 1]]
    for variant in VARIANTS:
        flat = rec.bag(ids, offsets[:-1], **_kw(variant, weights))
        assert tuple(flat.shape) == (offsets.size - 1, K) and flat.is_cuda
        for other in (rec.bag(two, **_kw(variant, w2)), E.bag(dense, ids, offsets[:-1], **_kw(variant, weights)),
                      E.bag(dense.cpu().numpy(), _cuda(two), **_kw(variant, _cuda(w2)))):
            assert np.array_equal(_u32(other), _u32(flat)), variant


@gpu
def test_a_damaged_record_counts_as_a_row_of_zeros():
    """Each of the three damages (a length field above N, lengths that do not add up, non-zero padding) on a file of K = 12:
    the status word is the unpack's, bags that avoid the record are unchanged, bags that use it equal the reference on the
    matrix with that row zeroed -- it is counted, so the mean divides by the same count."""
    _need_gpu()
    from vbq_amd import ops
    K, N, row = 12, 10, 23
    words, table, dense, total, _ = _record_case(K, N, None, False)
    ids = np.array([1, row, 2, 4, 5, row, row, 30, -1, row, 8, 9, 10], np.int64)
    offsets = np.array([0, 3, 5, 6, 8, 10, 13], np.int64)                # bags 0, 2, 3, 4 use the row; 1 and 5 avoid it
    weights = np.random.default_rng(7).standard_normal(ids.size).astype(np.float32)
    i, o, w = _cuda(ids), _cuda(offsets), _cuda(weights)
    zeroed = dense.cpu().numpy().copy()
    zeroed[row] = 0.0
    clean = words.cpu().numpy()
    assert (K * N.bit_length() + total) % 32 and clean.shape[1] == RR.record_words(K, N, total)
    want = {v: BR.bag(zeroed, ids, offsets, **_kw(v, weights))[0] for v in VARIANTS}
    for bit in (1, 2, 4):
        d = clean.copy()
        n0 = int(d[row, 0] & 0xF)
        if bit == 1:                                            # a length field > N
            d[row, 0] = (d[row, 0] & ~np.uint32(0xF)) | np.uint32(0xD)
        elif bit == 2:                                          # a valid length, but the lengths no longer add up
            d[row, 0] = (d[row, 0] & ~np.uint32(0xF)) | np.uint32(n0 + 1 if n0 < N else n0 - 1)
        else:                                                   # the last padding bit
            d[row, -1] |= np.uint32(1 << 31)
        damaged = _cuda(d.view(np.int32)).view(torch.uint32)
        st_unpack = torch.zeros(1, dtype=torch.uint32, device="cuda")
        ops.records_unpack(damaged, K, N, total, None, want_values=False, status=st_unpack)
        for variant in VARIANTS:
            st = torch.zeros(1, dtype=torch.uint32, device="cuda")
            got = ops.records_bag(damaged, K, N, total, table, i, o, status=st, **_kw(variant, w))
            assert int(st.cpu().item()) == int(st_unpack.cpu().item()) and int(st.cpu().item()) & bit, (bit, variant)
            assert np.array_equal(_u32(got), want[variant].view(np.uint32)), (bit, variant)
            untouched = ops.records_bag(words, K, N, total, table, i, o, **_kw(variant, w))
            assert np.array_equal(_u32(got)[[1, 5]], _u32(untouched)[[1, 5]]), (bit, variant)


@gpu
def test_an_id_past_the_matrix_is_skipped_and_reported():
    _need_gpu()
    from vbq_amd import ops
    K, N = 12, 10
    words, table, dense, total, _ = _record_case(K, N, None, False)
    ids = np.array([1, V, 2, 3, 1 << 40, V - 1], np.int64)
    offsets = np.array([0, 3, 4, 6], np.int64)
    i, o = _cuda(ids), _cuda(offsets)
    for mode in BR.MODES:
        want, st_want = BR.bag(dense.cpu().numpy(), ids, offsets, mode=mode)
        assert st_want == BR.BAD_ROW
        for call in (lambda **kw: ops.bag(dense, i, o, **kw), lambda **kw: ops.records_bag(words, K, N, total, table, i, o, **kw)):
            st = torch.zeros(1, dtype=torch.uint32, device="cuda")
            got = call(mode=mode, status=st)
            assert int(st.cpu().item()) == ops.BAG_BAD_ROW == 8
            assert np.array_equal(_u32(got), want.view(np.uint32)), mode
    two = (dense[1] + dense[2]) / 2                             # the mean of bag 0 divides by 2, not by 3
    assert torch.equal(ops.bag(dense, i, o, mode="mean")[0], two)


@gpu
def test_damaged_offsets_are_clamped_and_reported():
    """One reversed pair and one end past n_ids: the guard is a clamp, nothing reads outside ids or weights; the other bags are
    exact."""
    _need_gpu()
    from vbq_amd import ops
    K, N = 12, 10
    words, table, dense, total, _ = _record_case(K, N, None, False)
    ids = np.arange(10, dtype=np.int64)
    offsets = np.array([0, 2, 6, 4, 7, 1 << 50], np.int64)      # bag 2 runs backwards, the last one ends past n_ids
    weights = np.random.default_rng(8).standard_normal(ids.size).astype(np.float32)
    want, st_want = BR.bag(dense.cpu().numpy(), ids, offsets, weights=weights)
    assert st_want == BR.BAD_OFFSETS and not want[2].any()
    i, o, w = _cuda(ids), _cuda(offsets), _cuda(weights)
    for call in (lambda **kw: ops.bag(dense, i, o, **kw), lambda **kw: ops.records_bag(words, K, N, total, table, i, o, **kw)):
        st = torch.zeros(1, dtype=torch.uint32, device="cuda")
        got = call(weights=w, status=st)
        assert int(st.cpu().item()) == ops.BAG_BAD_OFFSETS == 16
        assert np.array_equal(_u32(got), want.view(np.uint32))


def _latents(rng, R, K, N):
    import vbq_amd
    tab = vbq_amd.gaussian_table(np.array([1.0]), N=N)[0]
    mu = rng.standard_normal((R, K)).astype(np.float32)
    sg = np.clip(np.exp(-2 + 0.7 * rng.standard_normal((R, K))), 1e-4, 10).astype(np.float32)
    return mu, sg, tab


@gpu
def test_record_embeddings_bag_on_a_real_file():
    _need_gpu()
    from vbq_amd import embeddings as E
    N, R, K, total = 10, 30, 12, 41
    mu, sg, tab = _latents(np.random.default_rng(9), R, K, N)
    rec = E.RecordEmbeddings(E.compress_to_records(mu.reshape(R, 3, 4), sg.reshape(R, 3, 4), total, tab, N=N))
    ids = np.array([4, 4, 29, -1, 0, 17, 3], np.int64)
    starts = np.array([0, 0, 3, 6], np.int64)
    got = rec.bag(ids, starts, mode="mean")
    assert tuple(got.shape) == (4, 3, 4) and got.dtype == torch.float32 and got.is_cuda
    want, st = BR.bag(rec.tensor().cpu().numpy().reshape(R, K), ids, np.append(starts, ids.size), mode="mean")
    assert st == 0 and np.array_equal(_u32(got).reshape(4, K), want.view(np.uint32))
    assert tuple(rec.bag(np.zeros(0, np.int64), np.zeros(0, np.int64)).shape) == (0, 3, 4)
    assert not rec.bag(np.zeros(0, np.int64), np.zeros(2, np.int64)).any()          # no ids, two bags: zeros


@gpu
def test_python_layer_refuses_what_the_contract_excludes():
    _need_gpu()
    import vbq_amd
    from vbq_amd import embeddings as E, ops
    K, N = 12, 10
    total = _mid_word(K, N)
    rng = np.random.default_rng(14)
    rec = E.RecordEmbeddings(_record_file(RR.random_indices(rng, V, K, N, total), N, total, _table(rng, 1, N)))
    dense = rec.tensor()
    ids, offsets = np.array([0, 1, -1, 4]), np.array([0, 2])
    for bag in (rec.bag, lambda *a, **kw: E.bag(dense, *a, **kw)):
        assert tuple(bag(ids, offsets).shape) == (2, K)
        assert tuple(bag(_cuda(ids), _cuda(offsets), weights=_cuda(np.ones(4, np.float32))).shape) == (2, K)
        with pytest.raises(ValueError, match="mode"):
            bag(ids, offsets, mode="avg")
        for mode in ("mean", "max"):
            with pytest.raises(ValueError, match="weights go with mode 'sum'"):
                bag(ids, offsets, mode=mode, weights=np.ones(4))
        with pytest.raises(ValueError, match="differ in shape"):
            bag(ids, offsets, weights=np.ones(3))
        with pytest.raises(ValueError, match="NaN or an infinity"):
            bag(ids, offsets, weights=np.array([1, np.nan, 1, 1]))
        with pytest.raises(IndexError, match="integers"):
            bag(np.array([0.5]), np.array([0]))
        with pytest.raises(IndexError, match=f"row {V} outside"):
            bag(np.array([0, V]), np.array([0]))
        for bad in ([1, 2], [0, 3, 2], [0, 5]):
            with pytest.raises(ValueError, match="offsets must start at 0"):
                bag(ids, np.array(bad))
        with pytest.raises(ValueError, match="need offsets"):
            bag(ids)
        with pytest.raises(ValueError, match="offsets must be None"):
            bag(ids.reshape(2, 2), offsets)
    # the ops layer: shapes, dtypes, the mode and the weights' mode; the ranges are the kernel's to clamp and report
    i, o = _cuda(ids.astype(np.int64)), _cuda(np.array([0, 2, 4], np.int64))
    w = _cuda(np.ones(4, np.float32))
    for call in (lambda *a, **kw: ops.bag(dense, *a, **kw),
                 lambda *a, **kw: ops.records_bag(rec._words, K, N, total, rec._table, *a, **kw)):
        with pytest.raises(ValueError, match="mode"):
            call(i, o, mode="avg")
        with pytest.raises(ValueError, match="weights go with mode 'sum'"):
            call(i, o, mode="max", weights=w)
        with pytest.raises(ValueError, match="differ in shape"):
            call(i, o, weights=w[:3])
        with pytest.raises(ValueError, match="dtype"):
            call(i.to(torch.int32), o)
        with pytest.raises(ValueError, match="dtype"):
            call(i, o, weights=w.double())
        with pytest.raises(ValueError, match="one-dimensional"):
            call(i.view(2, 2), o)
        with pytest.raises(ValueError, match="offsets must be"):
            call(i, o[:0])
        with pytest.raises(ValueError, match="out"):
            call(i, o, out=torch.empty((3, K), device="cuda"))
        with pytest.raises(vbq_amd.VBQError, match="ROCm device"):
            call(i.cpu(), o)
    with pytest.raises(ValueError, match=r"\[V, K\]"):
        ops.bag(dense.reshape(-1), i, o)
    with pytest.raises(vbq_amd.VBQError, match="limit is 163840"):
        ops.bag(torch.zeros((2, 20481), device="cuda"), i[:1], o[:2])
