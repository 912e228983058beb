"""The kernels that size their dynamic LDS from their arguments, at the widest rows they accept: the record pack and unpack
(vbq_records.hip), the pooled lookup (vbq_bag.hip), listed rows (vbqx_scores.hip), the nearest-row search (vbq_topk.hip) and the
budget DP with its sweep (vbq_budget.hip, vbqb_sweep.hip).  Each takes anything up to the 160 KiB of a CU and raises its
dynamic LDS limit once a launch needs more than 64 KiB; an LDS access past the allocation does not fault on this hardware
(stores are dropped, loads give zero), so a size formula that is a few words short shows as a wrong answer at wide rows only.
Every case here is compared with the plain reference its kernel already has (tests/*_reference.py), bit for bit where the
reference is exact, at the first launch above 64 KiB, at the last shape accepted and -- refused, outputs untouched -- one step
past it.

The shapes are not written down: they come out of the accept / refuse rules restated in tests/launch_plans.py (kept equal to
the sources by tests/test_launch_plans_host.py), and every case asserts, BEFORE it launches, the regime it is named after --
LDS above 64 KiB, the tile, where the code book and the back-pointers live, workgroups per CU.  After a retuning the case fails
on the host with that message instead of testing something else; test_control_a_wrong_plan_is_noticed shows it does.  The other
dimensions are tiny: what a case costs is its NumPy reference."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bag_reference as BG  # noqa: E402
import budget_reference as BR  # noqa: E402
import footprint as FP  # noqa: E402
import launch_plans as LP  # noqa: E402
import records_reference as RR  # noqa: E402
import scores_reference as SR  # noqa: E402
import topk_reference as TR  # noqa: E402

gpu = pytest.mark.gpu
METRICS = ("dot", "cosine")
VARIANTS = ("sum", "mean", "max", "weighted")
UNSUPPORTED = -2                                     # VBQ_ERR_UNSUPPORTED
FAR = 1 << 20                                        # above every K and width a rule here accepts


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _cus():
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def _regime(cond, what):
    if not cond:
        pytest.fail(f"by the rules restated in tests/launch_plans.py this shape is not in the regime the case is named after: {what} "
                    "(a constant was retuned: move the shape)")


def _cuda(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


def _u32(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _status():
    return torch.zeros(1, dtype=torch.uint32, device="cuda")


def _table(rng, C, N):
    return np.sort(rng.normal(size=(C, LP.table_size(N))).astype(np.float32), axis=1)


def _pack(idx, N, total):
    from vbq_amd import ops
    st = _status()
    words = ops.records_pack(_cuda(idx), total, N, status=st)
    assert int(st.cpu().item()) == 0
    return words


def _mid_word(K, N):
    """A total_bits near K * N / 3 at which the record ends inside a word."""
    total = K * N // 3
    while (K * LP.length_field_bits(N) + total) % 32 == 0:
        total += 1
    return total


def _first_opt_in(lds_of, last):
    """The smallest K in [2, last] whose launch needs more than 64 KiB, for an lds_of that grows with K."""
    _regime(lds_of(1) <= LP.LDS_OPT_IN < lds_of(last), f"no K up to {last} crosses {LP.LDS_OPT_IN} bytes")
    return LP.widest(lambda K: lds_of(K) <= LP.LDS_OPT_IN, 1, last) + 1


# ====================================================================================================== records
RECORD_CASES = ("full", "mid", "per_column")


def _record_shape(name):
    """(K, N, total_bits, per_column) of a record case, its regime asserted: a record of exactly kRecordsMaxWords words."""
    N = 3 if name == "per_column" else 10
    K = LP.widest(lambda k: LP.record_fits(k, N, N * k), 1, FAR)
    _regime(LP.record_words(K, N, N * K) == LP.RECORDS_MAX_WORDS == 8192 and not LP.record_fits(K + 1, N, N * (K + 1)),
            f"records {name}: K = {K} at N = {N} is not a record of 8192 words with 8193 one step further")
    total = _mid_word(K, N) if name == "mid" else N * K
    _regime(LP.record_fits(K, N, total), f"records {name}: K = {K}, total_bits = {total}")
    return K, N, total, name == "per_column"


@functools.lru_cache(maxsize=None)
def _record_case(name):
    """(K, N, total, rank indices [3, K], the restated records, the code points) -- computed once, read-only."""
    K, N, total, per_column = _record_shape(name)
    rng = np.random.default_rng(len(name) + K)
    idx = RR.random_indices(rng, 3, K, N, total)
    want = RR.pack(idx, N, total)
    table = _table(rng, K if per_column else 1, N)
    for a in (idx, want, table):
        a.setflags(write=False)
    return K, N, total, idx, want, table


@gpu
@pytest.mark.parametrize("name", RECORD_CASES)
def test_records_pack_and_unpack_at_the_longest_record(name):
    """Three rows, so three workgroups; the pack word for word, the unpack's ranks and code points bit for bit."""
    _need_gpu()
    from vbq_amd import ops
    K, N, total, idx, want, table = _record_case(name)
    st = _status()
    words = ops.records_pack(_cuda(idx), total, N, status=st)
    assert int(st.cpu().item()) == 0 and tuple(words.shape) == want.shape
    assert np.array_equal(_u32(words), want), (name, K, total)
    back = RR.unpack(want, K, N, total)
    assert np.array_equal(back, idx)
    val, got = ops.records_unpack(words, K, N, total, _cuda(table), want_idx=True, status=st)
    assert int(st.cpu().item()) == 0
    assert np.array_equal(got.cpu().numpy(), back.astype(np.uint16)), (name, K, total)
    cols = np.arange(K)[None, :] if table.shape[0] > 1 else 0
    assert np.array_equal(_u32(val), table[cols, back].view(np.uint32)), (name, K, total)
    sel = _cuda(np.array([2, 0, 2], np.int64))                   # the same call by lookup
    val2, _ = ops.records_unpack(words, K, N, total, _cuda(table), sel, status=st)
    assert int(st.cpu().item()) == 0 and np.array_equal(_u32(val2), _u32(val)[[2, 0, 2]])


@gpu
def test_record_embeddings_rows_on_the_widest_record():
    _need_gpu()
    from vbq_amd import bitstream as bs, embeddings as E
    K, N, total, idx, want, table = _record_case("full")
    h = bs.RecordsHeader(N=N, shape=tuple(idx.shape), C=table.shape[0], total_bits=total)
    rec = E.RecordEmbeddings(bs.write_records(h, table, want))
    assert rec.shape == (3, K) and rec.header.record_words == LP.RECORDS_MAX_WORDS
    ids = [2, 0, 0, 1]
    assert np.array_equal(_u32(rec.rows(ids)), table[0, idx.astype(np.int64)][ids].view(np.uint32))


@gpu
@pytest.mark.parametrize("name", ["full", "per_column"])
def test_a_record_one_word_too_long_is_refused(name):
    _need_gpu()
    from vbq_amd import _lib, ops
    K, N, _, _ = _record_shape(name)
    K, total = K + 1, N * (K + 1)
    words = LP.record_words(K, N, total)
    assert words == LP.RECORDS_MAX_WORDS + 1
    h = _lib.lib()
    idx = torch.zeros((2, K), dtype=torch.uint16, device="cuda")
    g = FP.Guarded((2, words), torch.uint32, "cuda")
    assert h.vbq_records_pack_u16(ops._ptr(idx), 2, K, N, total, g.ptr, None, ops._stream(idx)) == UNSUPPORTED
    assert b"exceeds the limit of 8192" in h.vbq_last_error()
    src = torch.zeros((2, words), dtype=torch.uint32, device="cuda")
    table = torch.zeros(LP.table_size(N), dtype=torch.float32, device="cuda")
    gv, gi = FP.Guarded((2, K), torch.float32, "cuda"), FP.Guarded((2, K), torch.uint16, "cuda")
    assert h.vbq_records_unpack_f32(ops._ptr(src), 2, K, N, total, ops._ptr(table), 1, None, 0, gv.ptr, gi.ptr, None,
                                    ops._stream(src)) == UNSUPPORTED
    assert b"exceeds the limit of 8192" in h.vbq_last_error()
    torch.cuda.synchronize()
    for guard in (g, gv, gi):
        guard.assert_untouched(f"refused record call, {name}")


# ====================================================================================================== bags
BAG_V = 5
BAGS = [[], [3], [1, 1, 4, 1], [-1, 2, -1, 0]]          # an empty bag, a bag of one, a repeated id, padding between ids
BAG_CASES = ("dense_first", "dense_last", "records_first_lds", "records_first_l2", "records_last", "records_fit", "records_fit_plus_1")


def _bag_list():
    ids = np.array([i for b in BAGS for i in b], np.int64)
    offsets = np.concatenate([[0], np.cumsum([len(b) for b in BAGS])]).astype(np.int64)
    return ids, offsets, np.random.default_rng(4).standard_normal(ids.size).astype(np.float32)


def _bag_shape(name, cus):
    """(K, N, total_bits, n_tables or 0 for the dense source) of a bag case, its regime asserted."""
    n_ids, n_bags = sum(len(b) for b in BAGS), len(BAGS)
    plan = lambda K, N, total, C, records=True: LP.bag_plan(K, N, total, C, n_ids, n_bags, cus, records)      # noqa: E731
    if name.startswith("dense"):
        last = LP.widest(lambda K: plan(K, 1, 0, 0, False) is not None, 1, FAR)
        K = last if name == "dense_last" else _first_opt_in(lambda k: plan(k, 1, 0, 0, False).lds_bytes, last)
        p, shape = plan(K, 1, 0, 0, False), (K, 1, 0, 0)
        _regime(name != "dense_last" or (plan(K + 1, 1, 0, 0, False) is None and p.lds_bytes == LP.BAG_LDS_LIMIT),
                f"bag {name}: K = {K} is not the last K accepted, to the byte")
        want_in_lds = False
    elif name == "records_first_lds":                     # one code book of N = 10 beside the record and the accumulators
        mid = lambda k: plan(k, 10, _mid_word(k, 10), 1)                                                      # noqa: E731
        K = _first_opt_in(lambda k: mid(k).lds_bytes, LP.widest(lambda k: mid(k) is not None, 1, FAR))
        p, shape, want_in_lds = mid(K), (K, 10, _mid_word(K, 10), 1), True
    elif name == "records_first_l2":                      # a code book per column (N = 3: 15 entries each) stays in L2
        full = lambda k: plan(k, 3, 3 * k, k)                                                                 # noqa: E731
        K = _first_opt_in(lambda k: full(k).lds_bytes, LP.widest(lambda k: full(k) is not None, 1, FAR))
        p, shape, want_in_lds = full(K), (K, 3, 3 * K, K), False
    elif name == "records_last":                          # N = 10 at the full budget: no room for the code book
        full = lambda k: plan(k, 10, 10 * k, 1)                                                               # noqa: E731
        K = LP.widest(lambda k: full(k) is not None, 1, FAR)
        p, shape, want_in_lds = full(K), (K, 10, 10 * K, 1), False
        _regime(p.lds_bytes == LP.BAG_LDS_LIMIT and K == LP.BAG_ALWAYS_K, f"bag {name}: K = {K} does not fill the LDS to the byte")
    else:                                                 # the budget up to which the code book fits beside K = 16000, and one more bit
        K = 16000
        _regime(plan(K, 10, 0, 1) is not None and plan(K, 10, 0, 1).table_in_lds and not plan(K, 10, 10 * K, 1).table_in_lds,
                f"bag {name}: K = {K} does not have the code book in LDS at total_bits = 0 and out of it at the full budget")
        fit = LP.widest(lambda t: plan(K, 10, t, 1).table_in_lds, 0, 10 * K)
        total = fit + (name == "records_fit_plus_1")
        p, shape, want_in_lds = plan(K, 10, total, 1), (K, 10, total, 1), name == "records_fit"
        _regime(name != "records_fit" or p.lds_bytes == LP.BAG_LDS_LIMIT, f"bag {name}: {p.lds_bytes} bytes is not an exact fit")
    _regime(p is not None and p.lds_bytes > LP.LDS_OPT_IN and p.table_in_lds == want_in_lds,
            f"bag {name}: {shape} plans {p}, wanted more than {LP.LDS_OPT_IN} bytes and table_in_lds = {want_in_lds}")
    return shape


def _bag_kw(variant, weights):
    return dict(mode="sum", weights=weights) if variant == "weighted" else dict(mode=variant)


@gpu
@pytest.mark.parametrize("name", BAG_CASES)
def test_bags_equal_the_reference_bit_for_bit(name):
    """All three modes and the weighted sum.  The record source against the dense source, and both against the reference."""
    _need_gpu()
    from vbq_amd import ops
    K, N, total, n_tables = _bag_shape(name, _cus())
    rng = np.random.default_rng(K)
    ids, offsets, weights = _bag_list()
    i, o, w = _cuda(ids), _cuda(offsets), _cuda(weights)
    if n_tables:
        table = _cuda(_table(rng, n_tables, N))
        words = _pack(RR.random_indices(rng, BAG_V, K, N, total), N, total)
        dense = ops.records_unpack(words, K, N, total, table)[0]
    else:
        emb = rng.standard_normal((BAG_V, K)).astype(np.float32)
        emb[4, : K // 2] = emb[1, : K // 2]                          # ties for the max within the repeated-id bag
        dense = _cuda(emb)
    host = dense.cpu().numpy()
    for variant in VARIANTS:
        want, st_want = BG.bag(host, ids, offsets, **_bag_kw(variant, weights))
        assert st_want == 0
        st = _status()
        got = ops.bag(dense, i, o, status=st, **_bag_kw(variant, w))
        assert int(st.cpu().item()) == 0 and np.array_equal(_u32(got), want.view(np.uint32)), (name, variant, "dense")
        if n_tables:
            got = ops.records_bag(words, K, N, total, table, i, o, status=st, **_bag_kw(variant, w))
            assert int(st.cpu().item()) == 0 and np.array_equal(_u32(got), want.view(np.uint32)), (name, variant, "records")


@gpu
def test_a_damaged_wide_record_counts_as_a_row_of_zeros():
    """Each of the three damages in the LAST chunk of 64 coordinates of the widest record the bags take: a length field above
    N, a length changed so that the sum is off, the last padding bit."""
    _need_gpu()
    from vbq_amd import ops
    K, N, total, _ = _bag_shape("records_last", _cus())
    row, rng = 2, np.random.default_rng(8)
    table = _cuda(_table(rng, 1, N))
    words = _pack(RR.random_indices(rng, BAG_V, K, N, total), N, total)
    ids, offsets, weights = np.array([1, row, 4, row, 3], np.int64), np.array([0, 2, 3, 4, 5], np.int64), None
    weights = rng.standard_normal(ids.size).astype(np.float32)           # bags 0 and 2 use the row, 1 and 3 avoid it
    i, o, w = _cuda(ids), _cuda(offsets), _cuda(weights)
    zeroed = ops.records_unpack(words, K, N, total, table)[0].cpu().numpy()
    zeroed[row] = 0.0
    want = {v: BG.bag(zeroed, ids, offsets, **_bag_kw(v, weights))[0] for v in VARIANTS}
    clean = words.cpu().numpy()
    end = K * LP.length_field_bits(N) + total
    k = K - 3                                                           # in the last chunk: K - 3 >= 64 * ((K - 1) // 64)
    assert end % 32 and clean.shape[1] == LP.record_words(K, N, total) and k // 64 == (K - 1) // 64
    assert LP.length_field_bits(N) == 4
    shift = np.uint32(4 * (k % 8))
    for bit in (1, 2, 4):
        d = clean.copy()
        n0 = int(d[row, k // 8] >> shift) & 0xF
        field = ~(np.uint32(0xF) << shift)
        if bit == 1:                                                    # a length field > N
            d[row, k // 8] = (d[row, k // 8] & field) | (np.uint32(0xD) << shift)
        elif bit == 2:                                                  # a valid length, but the lengths no longer add up
            d[row, k // 8] = (d[row, k // 8] & field) | (np.uint32(n0 + 1 if n0 < N else n0 - 1) << shift)
        else:                                                           # the last padding bit
            d[row, -1] |= np.uint32(1 << 31)
        damaged = _cuda(d.view(np.int32)).view(torch.uint32)
        st_unpack = _status()
        ops.records_unpack(damaged, K, N, total, None, want_values=False, status=st_unpack)
        for variant in VARIANTS:
            st = _status()
            got = ops.records_bag(damaged, K, N, total, table, i, o, status=st, **_bag_kw(variant, w))
            assert int(st.cpu().item()) == int(st_unpack.cpu().item()) and int(st.cpu().item()) & bit, (bit, variant)
            assert np.array_equal(_u32(got), want[variant].view(np.uint32)), (bit, variant)


@gpu
def test_bags_one_step_past_the_limit_are_refused():
    _need_gpu()
    from vbq_amd import _lib, ops
    cus = _cus()
    ids, offsets, _ = _bag_list()
    i, o = _cuda(ids), _cuda(offsets)
    K = _bag_shape("dense_last", cus)[0] + 1
    g = FP.Guarded((len(BAGS), K), torch.float32, "cuda")
    with pytest.raises(_lib.VBQError, match=f"K = {K} .* the limit is {LP.BAG_LDS_LIMIT} "):
        ops.bag(torch.zeros((BAG_V, K), device="cuda"), i, o, out=g.view)
    g.assert_untouched("refused dense bag")
    K = _bag_shape("records_last", cus)[0] + 1
    words = torch.zeros((BAG_V, LP.record_words(K, 10, 10 * K)), dtype=torch.uint32, device="cuda")
    g = FP.Guarded((len(BAGS), K), torch.float32, "cuda")
    with pytest.raises(_lib.VBQError, match=f"K = {K} .* the limit is {LP.BAG_LDS_LIMIT} "):
        ops.records_bag(words, K, 10, 10 * K, torch.zeros(LP.table_size(10), device="cuda"), i, o, out=g.view)
    torch.cuda.synchronize()
    g.assert_untouched("refused record bag")


# ====================================================================================================== listed rows
SCORES_V = 7
SCORES_CASES = ("dense_below", "dense_first", "dense_last", "records_last", "records_per_column_last")


def _scores_shape(name):
    """(K, N, total_bits, n_tables or 0 for the dense source) of a scores case, its regime asserted."""
    dense = lambda K: LP.scores_plan(K, 1, 0, False)                                                          # noqa: E731
    if name.startswith("dense"):
        last = LP.widest(lambda K: dense(K) is not None, 1, FAR)
        first = _first_opt_in(lambda K: dense(K).lds_bytes, last)
        K = {"dense_below": first - 1, "dense_first": first, "dense_last": last}[name]
        p, shape = dense(K), (K, 1, 0, 0)
        _regime(name != "dense_last" or dense(K + 1) is None, f"scores {name}: K = {K} is not the last K accepted")
    else:
        N, per_column = (3, True) if name == "records_per_column_last" else (10, False)
        full = lambda K: LP.scores_plan(K, N, N * K, True)                                                    # noqa: E731
        K = LP.widest(lambda k: full(k) is not None, 1, FAR)
        p, shape = full(K), (K, N, N * K, K if per_column else 1)
        _regime(full(K + 1) is None and K >= LP.SCORES_ALWAYS_K, f"scores {name}: K = {K} is not the last K accepted")
    _regime(p is not None and p.G == LP.SCORES_MIN_GROUP == 8 and (p.lds_bytes > LP.LDS_OPT_IN) == (name != "dense_below"),
            f"scores {name}: {shape} plans {p}")
    return shape, p


def _pairs(rng, G, flip):
    """ids [Q, M] of 8 G + 3 pairs -- eight whole groups and three pairs -- with padding, and `far` = the same with one id >= V."""
    P = 8 * G + 3
    ids = rng.integers(0, SCORES_V, P).astype(np.int64)
    ids[[2, G, P - 1]] = -1
    far = ids.copy()
    far[P - 2] = SCORES_V
    shape = (1, P) if flip else (P, 1)                               # one query for all pairs; a query of its own per pair
    return ids.reshape(shape), far.reshape(shape)


@gpu
@pytest.mark.parametrize("name", SCORES_CASES)
def test_scores_equal_the_exact_restatement(name):
    _need_gpu()
    from vbq_amd import ops
    (K, N, total, n_tables), plan = _scores_shape(name)
    rng = np.random.default_rng(K)
    if n_tables:
        table = _table(rng, n_tables, N)
        words = _pack(RR.random_indices(rng, SCORES_V, K, N, total), N, total)
        rows = SR.decode(words.cpu().numpy(), K, N, total, table)
        assert rows.any(axis=1).all()                                # every record is one the format allows
        calls = [lambda q, i, m, st: ops.records_scores(words, K, N, total, _cuda(table), q, i, m, status=st)]
        if LP.scores_plan(K, 1, 0, False) is not None:               # the dense source on the same rows
            calls.append(lambda q, i, m, st: ops.scores(_cuda(rows), q, i, m, status=st))
    else:
        rows = rng.standard_normal((SCORES_V, K)).astype(np.float32)
        rows[3] = rows[5]
        calls = [lambda q, i, m, st: ops.scores(_cuda(rows), q, i, m, status=st)]
    ids, far = _pairs(rng, plan.G, SCORES_CASES.index(name) % 2 == 1)
    q = rng.standard_normal((ids.shape[0], K)).astype(np.float32)
    for metric in METRICS:
        want, st_want = SR.scores(q, rows, ids, metric)
        want_far, st_far = SR.scores(q, rows, far, metric)
        assert st_want == 0 and st_far == SR.BAD_ROW and np.isneginf(want).sum() == 3
        for call in calls:
            st = _status()
            got = call(_cuda(q), _cuda(ids), metric, st)
            assert int(st.cpu().item()) == 0 and np.array_equal(_u32(got), _u32(want)), (name, metric)
            got = call(_cuda(q), _cuda(far), metric, st)
            assert int(st.cpu().item()) == SR.BAD_ROW and np.array_equal(_u32(got), _u32(want_far)), (name, metric)


@gpu
def test_scores_one_step_past_the_limit_are_refused():
    _need_gpu()
    from vbq_amd import _lib, ops
    ids = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
    K = _scores_shape("dense_last")[0][0] + 1
    g = FP.Guarded((2, 3), torch.float32, "cuda")
    wide = torch.zeros((2, K), device="cuda")
    with pytest.raises(_lib.VBQError, match=f"K = {K} .* the limit is {LP.SCORES_LDS_LIMIT} "):
        ops.scores(wide, wide, ids, "dot", out=g.view)
    g.assert_untouched("refused dense scores")
    K = _scores_shape("records_last")[0][0] + 1
    words = torch.zeros((2, LP.record_words(K, 10, 10 * K)), dtype=torch.uint32, device="cuda")
    g = FP.Guarded((2, 3), torch.float32, "cuda")
    with pytest.raises(_lib.VBQError, match=f"K = {K} .* the limit is {LP.SCORES_LDS_LIMIT} "):
        ops.records_scores(words, K, 10, 10 * K, torch.zeros(LP.table_size(10), device="cuda"), torch.zeros((2, K), device="cuda"),
                           ids, "cosine", out=g.view)
    torch.cuda.synchronize()
    g.assert_untouched("refused record scores")


@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["always", "last"])
def test_scores_equal_the_scores_the_search_reports_at_its_widest_rows(name, metric):
    """scores(queries, ids) == the scores most_similar reports for the same (query, row), bit for bit, at K = 512 and at the
    last K the dense search takes."""
    _need_gpu()
    from vbq_amd import embeddings as E
    last = LP.widest(lambda K: LP.topk_plan(K, 1, 0, 0, False) is not None, 1, FAR)
    K = last if name == "last" else LP.TOPK_ALWAYS_K
    p = LP.topk_plan(K, 1, 0, 0, False)
    _regime(p.per_cu == 1 and p.R == LP.TOPK_MIN_ROWS and LP.scores_plan(K, 1, 0, False) is not None, f"K = {K} plans {p}")
    emb, q, _ = TR.case_data(K, 130, 2)
    ids, s = E.most_similar(emb, q, k=64, metric=metric)
    assert (ids >= 0).all()
    assert np.array_equal(_u32(E.scores(emb, q, ids, metric)), _u32(s)), (K, metric)


# ====================================================================================================== the search
TOPK_REGIMES = ((128, 2), (64, 2), (32, 2), (64, 1), (32, 1))              # (rows per tile, workgroups per CU), in ascending K
TOPK_CASES = [(R, per_cu, at) for R, per_cu in TOPK_REGIMES for at in ("first", "mid", "last")][1:]     # (128, 2) begins at K = 1


def _topk_dense_k(R, per_cu, at):
    """The first, a middle or the last K of a regime of the dense source, the regime asserted."""
    plan = lambda K: LP.topk_plan(K, 1, 0, 0, False)                                                          # noqa: E731
    last = LP.widest(lambda K: plan(K) is not None, 1, FAR)
    ks = [K for K in range(1, last + 1) if (plan(K).R, plan(K).per_cu) == (R, per_cu)]
    _regime(ks and ks == list(range(ks[0], ks[-1] + 1)), f"no K of the dense search takes tiles of {R} rows at {per_cu} workgroups per CU")
    K = {"first": ks[0], "mid": (ks[0] + ks[-1]) // 2 | 1, "last": ks[-1]}[at]                               # the middle one odd: K2 = K + 1
    p = plan(K)
    _regime((p.R, p.per_cu) == (R, per_cu) and (per_cu == 2 or p.lds_bytes > LP.TOPK_LDS_TWO_PER_CU > LP.LDS_OPT_IN)
            and (at != "last" or plan(K + 1) is None or (plan(K + 1).R, plan(K + 1).per_cu) != (R, per_cu)), f"K = {K} plans {p}")
    return K, p


def _topk_run(call, V, K, Q, k, what):
    """One search in a workspace of exactly vbq_topk_workspace_bytes between canaries -> (ids, scores) on the host."""
    from vbq_amd import _lib
    ws = FP.guarded_workspace(_lib.lib().vbq_topk_workspace_bytes(V, K, Q, k, 0), "cuda")
    ids, scores = call(ws.view)
    torch.cuda.synchronize()
    ws.assert_outside_intact(what)
    return ids.cpu().numpy(), scores.cpu().numpy()


@gpu
@pytest.mark.parametrize("R,per_cu,at", TOPK_CASES)
def test_dense_search_in_every_regime_and_on_either_side_of_every_flip(R, per_cu, at):
    """Both metrics, one query and a second block of queries, k = 1 and 64, a row count with two rows in its last tile and one
    with seven, with and without exclusions; the tied rows of topk_reference.case_data."""
    _need_gpu()
    from vbq_amd import ops
    K, _ = _topk_dense_k(R, per_cu, at)
    for V in (130, R + 7):
        for Q in (1, 33):
            emb, q, exclude = TR.case_data(K, V, Q)
            e, qq, ex = _cuda(emb), _cuda(q), _cuda(exclude)
            for metric in METRICS:
                for k in (1, 64):
                    for excl in (None, exclude):
                        what = f"topk K={K} V={V} Q={Q} k={k} {metric} exclude={excl is not None}"
                        ids, scores = _topk_run(lambda ws: ops.topk(e, qq, k, metric, None if excl is None else ex, workspace=ws),
                                                V, K, Q, k, what)
                        TR.accept(ids, scores, q, emb, k, metric, excl)


TOPK_RECORD_CASES = ("always", "last", "code_book_in_lds", "code_book_in_l2", "per_column_last")


def _topk_record_shape(name):
    """(K, N, total_bits, n_tables) of a record search, its regime asserted: one workgroup per CU, more than 80 KiB."""
    if name == "always":                                 # kTopkAlwaysK at N = 10 and the full budget
        shape, want = (LP.TOPK_ALWAYS_K, 10, 10 * LP.TOPK_ALWAYS_K, 1), (LP.TOPK_MIN_ROWS, False)
    elif name in ("last", "per_column_last"):
        N = 10 if name == "last" else 3
        full = lambda K: LP.topk_plan(K, N, N * K, 1 if name == "last" else K, True)                         # noqa: E731
        K = LP.widest(lambda k: full(k) is not None, 1, FAR)
        _regime(full(K + 1) is None and K >= LP.TOPK_ALWAYS_K, f"record search {name}: K = {K} is not the last K accepted")
        shape, want = (K, N, N * K, 1 if name == "last" else K), (LP.TOPK_MIN_ROWS, False)
    else:                                                # tiles of 64 rows with the one code book beside them, and without room for it
        K = 300 if name == "code_book_in_lds" else 350
        shape, want = (K, 10, _mid_word(K, 10), 1), (64, name == "code_book_in_lds")
    p = LP.topk_plan(*shape, True)
    _regime(p is not None and p.per_cu == 1 and p.lds_bytes > LP.TOPK_LDS_TWO_PER_CU > LP.LDS_OPT_IN and (p.R, p.table_in_lds) == want,
            f"record search {name}: {shape} plans {p}, wanted one workgroup per CU and (R, table_in_lds) = {want}")
    return shape


@gpu
@pytest.mark.parametrize("name", TOPK_RECORD_CASES)
def test_record_search_above_eighty_kib(name):
    """The record source equals the dense source bit for bit, and the float64 reference accepts the result."""
    _need_gpu()
    from vbq_amd import ops
    K, N, total, n_tables = _topk_record_shape(name)
    V, Q, k = 130, 33, 64
    rng = np.random.default_rng(K + total)
    table = _cuda(_table(rng, n_tables, N))
    idx = RR.random_indices(rng, V, K, N, total)
    idx[7::7] = idx[6:-1:7][:len(idx[7::7])]                          # every seventh row repeats the row before it
    words = _pack(idx, N, total)
    dense = ops.records_unpack(words, K, N, total, table)[0]
    q = rng.standard_normal((Q, K)).astype(np.float32)
    exclude = TR.case_data(5, V, Q)[2]
    qq, ex = _cuda(q), _cuda(exclude)
    for metric in METRICS:
        for excl in (None, exclude):
            what = f"record search {name} {metric} exclude={excl is not None}"
            st = _status()
            ids, scores = _topk_run(lambda ws: ops.records_topk(words, K, N, total, table, qq, k, metric, None if excl is None else ex,
                                                                status=st, workspace=ws), V, K, Q, k, what)
            assert int(st.cpu().item()) == 0
            TR.accept(ids, scores, q, dense.cpu().numpy(), k, metric, excl)
            if LP.topk_plan(K, 1, 0, 0, False) is not None:
                ids_d, scores_d = _topk_run(lambda ws: ops.topk(dense, qq, k, metric, None if excl is None else ex, workspace=ws),
                                            V, K, Q, k, what + " (dense)")
                assert np.array_equal(ids, ids_d) and np.array_equal(_u32(scores), _u32(scores_d)), what


@gpu
def test_searches_one_step_past_the_limit_are_refused():
    _need_gpu()
    from vbq_amd import _lib, ops
    h = _lib.lib()
    V, Q, k = 4, 2, 3
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    K = LP.widest(lambda K: LP.topk_plan(K, 1, 0, 0, False) is not None, 1, FAR) + 1
    emb, q = torch.zeros((V, K), device="cuda"), torch.zeros((Q, K), device="cuda")
    gi, gs = FP.Guarded((Q, k), torch.int64, "cuda"), FP.Guarded((Q, k), torch.float32, "cuda")
    assert h.vbq_topk_f32(ops._ptr(emb), V, K, ops._ptr(q), Q, k, 1, None, 0, gi.ptr, gs.ptr, 0, ops._ptr(ws), ws.numel(),
                          ops._stream(emb)) == UNSUPPORTED
    assert f"K = {K} ".encode() in h.vbq_last_error() and f"the limit is {LP.TOPK_LDS_LIMIT} ".encode() in h.vbq_last_error()
    K = _topk_record_shape("last")[0] + 1
    words = torch.zeros((V, LP.record_words(K, 10, 10 * K)), dtype=torch.uint32, device="cuda")
    table, q = torch.zeros(LP.table_size(10), device="cuda"), torch.zeros((Q, K), device="cuda")
    assert h.vbq_records_topk_f32(ops._ptr(words), V, K, 10, 10 * K, ops._ptr(table), 1, ops._ptr(q), Q, k, 0, None, 0, gi.ptr, gs.ptr,
                                  None, 0, ops._ptr(ws), ws.numel(), ops._stream(words)) == UNSUPPORTED
    assert f"K = {K} ".encode() in h.vbq_last_error() and f"the limit is {LP.TOPK_LDS_LIMIT} ".encode() in h.vbq_last_error()
    torch.cuda.synchronize()
    gi.assert_untouched("refused search: ids")
    gs.assert_untouched("refused search: scores")


# ====================================================================================================== the budget DP and its sweep
def _budget_scores(rng, N, R, K):
    """The recipe of tests/test_gpu_budget_dp.py: 0 at some depth, falling off steeply above it."""
    err = np.abs(rng.standard_normal((1, R, K))) * 2.0 ** (-np.arange(N + 1))[:, None, None] * rng.uniform(0.5, 2, (N + 1, R, K))
    return -0.5 * (err / np.exp(-3 + rng.standard_normal((1, R, K)))) ** 2


def _budget_flip(K, N):
    """The last width (budget + 1) at which the back-pointers of K coordinates stay in LDS, the regime asserted: more than
    64 KiB there, the value rows alone one step further."""
    _regime(LP.budget_plan(K, N, K * N + 1) is not None and not LP.budget_plan(K, N, K * N + 1).bp_in_lds,
            f"K = {K}, N = {N} keeps its back-pointers in LDS at every budget")
    width = LP.widest(lambda w: LP.budget_plan(K, N, w).bp_in_lds, 1, K * N + 1)
    p, q = LP.budget_plan(K, N, width), LP.budget_plan(K, N, width + 1)
    _regime(p.bp_in_lds and p.lds_bytes > LP.LDS_OPT_IN and not q.bp_in_lds and p.threads == q.threads == 256,
            f"K = {K}, N = {N}: width {width} plans {p}, width {width + 1} plans {q}")
    return width


def _budget_widest(K, N):
    """The widest value rows that fit, the regime asserted: the whole LDS, back-pointers in the workspace."""
    width = LP.widest(lambda w: LP.budget_plan(K, N, w) is not None, 1, K * N + 2)
    p = LP.budget_plan(K, N, width)
    _regime(width <= K * N and p.lds_bytes == LP.BUDGET_LDS_BYTES > LP.LDS_OPT_IN and not p.bp_in_lds
            and LP.budget_plan(K, N, width + 1) is None,
            f"K = {K}, N = {N}: width {width} plans {p}")
    return width


@functools.lru_cache(maxsize=None)
def _budget_case(K, N, R):
    fhat = _budget_scores(np.random.default_rng(K + N + R), N, R, K)
    fhat.setflags(write=False)
    return fhat


@functools.lru_cache(maxsize=None)
def _budget_reference(K, N, R, budget):
    bits, obj = BR.budget_dp_rows(_budget_case(K, N, R), budget)
    bits.setflags(write=False)
    obj.setflags(write=False)
    return bits, obj


@functools.lru_cache(maxsize=None)
def _budget_curve(K, N, R, width):
    """The last value row T[K-1][0 .. width-1]: the forward pass of budget_reference.budget_dp_rows (the same candidates, the
    same np.argmax) without its back-pointers.  The recurrence does not depend on the budget, so entry n is the objective
    budget_dp_rows reports at budget n; the tests hold it against budget_dp_rows at the budgets they walk."""
    fhat = _budget_case(K, N, R)
    T = np.full((R, width), -np.inf)
    top = min(width, N + 1)
    T[:, :top] = fhat[:top, :, 0].T
    rr = np.arange(R)[:, None]
    for k in range(1, K):
        cand = np.full((N + 1, R, width), -np.inf)
        for m in range(min(N, width - 1) + 1):
            cand[m, :, m:] = fhat[m, :, k][:, None] + T[:, :width - m]
        T = cand[np.argmax(cand, axis=0), rr, np.arange(width)[None, :]]
    T.setflags(write=False)
    return T


def _dp_equals_reference(K, N, R, budget, **kw):
    from vbq_amd import ops
    bits, obj = ops.budget_dp(_cuda(_budget_case(K, N, R)), K, budget, **kw)
    want_bits, want_obj = _budget_reference(K, N, R, budget)
    assert np.array_equal(bits.cpu().numpy(), want_bits), (K, budget)
    assert np.array_equal(_u64(obj.cpu().numpy()), _u64(want_obj)), (K, budget)


def _sweep_equals_reference(K, N, R, budgets, curve_len, **kw):
    from vbq_amd import ops
    bits, obj, curve = ops.budget_dp_sweep(_cuda(_budget_case(K, N, R)), K, budgets, curve_len=curve_len, **kw)
    for s, b in enumerate(budgets):
        want_bits, want_obj = _budget_reference(K, N, R, b)
        assert np.array_equal(bits[s].cpu().numpy(), want_bits), (K, budgets, b)
        assert np.array_equal(_u64(obj[s].cpu().numpy()), _u64(want_obj)), (K, budgets, b)
    if curve_len:
        want = _budget_curve(K, N, R, curve_len)
        for b in budgets:
            if b < curve_len:
                assert np.array_equal(_u64(want[:, b]), _u64(_budget_reference(K, N, R, b)[1])), "the restated curve and budget_dp_rows differ"
        assert np.array_equal(_u64(curve.cpu().numpy()), _u64(want)), (K, budgets, curve_len)


@gpu
@pytest.mark.parametrize("side", ["lds", "workspace"])
def test_budget_dp_on_either_side_of_the_back_pointer_flip(side):
    """K = 150, N = 10: the last budget whose back-pointers fit the LDS beside the value rows and the first whose do not, through
    the single DP, the sweep, and the sweep with a curve of the same width."""
    _need_gpu()
    K, N, R = 150, 10, 3
    width = _budget_flip(K, N) + (side == "workspace")
    _dp_equals_reference(K, N, R, width - 1)
    _sweep_equals_reference(K, N, R, [0, width - 1], 0)
    _sweep_equals_reference(K, N, R, [0, width - 1], width)


@gpu
def test_budget_dp_at_the_widest_value_rows():
    """K = 1023, N = 10 at the last width whose two value rows fit the LDS.  Two rows in a workspace of exactly one slice between
    canaries: the second row is a second round of the one workgroup."""
    _need_gpu()
    K, N, R = 1023, 10, 2
    width = _budget_widest(K, N)
    slice_bytes = LP.budget_bp_row_bytes(K, width)
    ws = FP.guarded_workspace(slice_bytes, "cuda")
    _dp_equals_reference(K, N, R, width - 1, workspace=ws.view)
    ws.assert_outside_intact("budget_dp workspace")
    ws = FP.guarded_workspace(slice_bytes, "cuda")
    assert 5000 < width - 1
    _sweep_equals_reference(K, N, R, [5000, width - 1], 0, workspace=ws.view)
    ws.assert_outside_intact("budget_dp_sweep workspace")
    _sweep_equals_reference(K, N, R, [], width)                        # the curve-only pass: no back-pointers anywhere
    want = _budget_curve(K, N, R, width)
    for b in (5000, width - 1):
        assert np.array_equal(_u64(want[:, b]), _u64(_budget_reference(K, N, R, b)[1]))


@gpu
def test_budget_dp_one_step_past_the_widest_value_rows_is_refused():
    _need_gpu()
    from vbq_amd import _lib, _lib_budget, ops
    K, N, R = 1023, 10, 2
    budget = _budget_widest(K, N)                                      # width + 1 - 1
    fhat = torch.zeros((N + 1, R, K), dtype=torch.float64, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    g_bits, g_obj = FP.Guarded((R, K), torch.int32, "cuda"), FP.Guarded((R,), torch.float64, "cuda")
    h = _lib.lib()
    assert h.vbq_budget_dp_f64(ops._ptr(fhat), R, K, N, budget, g_bits.ptr, g_obj.ptr, None, ops._ptr(ws), ws.numel(),
                               ops._stream(fhat)) == UNSUPPORTED
    assert b"do not fit the LDS" in h.vbq_last_error()
    hb = _lib_budget.lib()
    s_bits, s_obj = FP.Guarded((1, R, K), torch.int32, "cuda"), FP.Guarded((1, R), torch.float64, "cuda")
    g_curve = FP.Guarded((R, budget + 1), torch.float64, "cuda")
    one = (ctypes.c_int32 * 1)(budget)
    assert hb.vbqb_budget_sweep_f64(ops._ptr(fhat), R, K, N, one, 1, s_bits.ptr, s_obj.ptr, None, 0, None, ops._ptr(ws), ws.numel(),
                                    ops._stream(fhat)) == UNSUPPORTED
    assert hb.vbqb_budget_sweep_f64(ops._ptr(fhat), R, K, N, None, 0, None, None, g_curve.ptr, budget + 1, None, None, 0,
                                    ops._stream(fhat)) == UNSUPPORTED
    torch.cuda.synchronize()
    for g in (g_bits, g_obj, s_bits, s_obj, g_curve):
        g.assert_untouched("refused budget DP")


# ====================================================================================================== the control
def test_control_a_wrong_plan_is_noticed(monkeypatch):
    """With the restated limits at 64 KiB (and the longest record halved) the regime assertion of a case of every kernel
    fails on the host, before anything is launched: no GPU is needed to see it."""
    for limit in ("BAG_LDS_LIMIT", "SCORES_LDS_LIMIT", "TOPK_LDS_LIMIT", "TOPK_LDS_TWO_PER_CU", "BUDGET_LDS_BYTES"):
        monkeypatch.setattr(LP, limit, 64 * 1024)
    monkeypatch.setattr(LP, "RECORDS_MAX_WORDS", 4096)
    failed = pytest.fail.Exception
    for name in RECORD_CASES:
        with pytest.raises(failed, match="not in the regime"):
            _record_shape(name)
    for name in BAG_CASES:
        with pytest.raises(failed, match="not in the regime"):
            _bag_shape(name, 256)
    for name in SCORES_CASES:
        if name != "dense_below":
            with pytest.raises(failed, match="not in the regime"):
                _scores_shape(name)
    for R, per_cu, at in TOPK_CASES:
        if per_cu == 1:
            with pytest.raises(failed, match="not in the regime"):
                _topk_dense_k(R, per_cu, at)
    for name in TOPK_RECORD_CASES:
        with pytest.raises(failed, match="not in the regime"):
            _topk_record_shape(name)
    with pytest.raises(failed, match="not in the regime"):
        _budget_flip(150, 10)
    with pytest.raises(failed, match="not in the regime"):
        _budget_widest(1023, 10)


def test_the_shapes_the_cases_derive():
    """The derived shapes with the sources as they are, for 256 CUs: what tests/test_launch_plans_host.py pins."""
    assert [_record_shape(n)[0] for n in RECORD_CASES] == [18724, 18724, 52428]
    assert [_bag_shape(n, 256) for n in BAG_CASES] == [
        (8193, 1, 0, 0), (20480, 1, 0, 0), (6432, 10, 21441, 1), (7599, 3, 22797, 7599), (16804, 10, 168040, 1),
        (16000, 10, 157216, 1), (16000, 10, 157217, 1)]
    assert [_scores_shape(n)[0] for n in SCORES_CASES] == [
        (2031, 1, 0, 0), (2032, 1, 0, 0), (5103, 1, 0, 0), (3549, 10, 35490, 1), (4413, 3, 13239, 4413)]
    assert [_topk_dense_k(*c)[0] for c in TOPK_CASES] == [63, 124, 125, 167, 208, 209, 259, 310, 311, 365, 418, 419, 521, 624]
    assert [_topk_record_shape(n) for n in TOPK_RECORD_CASES] == [
        (512, 10, 5120, 1), (514, 10, 5140, 1), (300, 10, 1000, 1), (350, 10, 1166, 1), (580, 3, 1740, 580)]
    assert _budget_flip(150, 10) == 985 and _budget_widest(1023, 10) == 10228
