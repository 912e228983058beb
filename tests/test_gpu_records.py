"""The record kernels (vbq_records.hip) against the NumPy restatement of the format (tests/records_reference.py), byte for
byte, on synthetic rank indices -- random lengths per row that add up to total_bits, random codes -- so that the parity tests do
not depend on the budget DP; then the surfaces built on them (vbq_amd.embeddings.compress_to_records / RecordEmbeddings /
decompress) against quantize_rows_to_budget, and what the kernels do with damaged records and rows outside the contract."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import records_reference as RR  # noqa: E402

gpu = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _table(rng, C, N):
    return np.sort(rng.normal(size=(C, 2 ** (N + 1) - 1)).astype(np.float32), axis=1)


def _status():
    return torch.zeros(1, dtype=torch.uint32, device="cuda")


def _pack(idx, total, N):
    from vbq_amd import ops
    st = _status()
    words = ops.records_pack(torch.from_numpy(idx).cuda(), total, N, status=st)
    assert words.dtype == torch.uint32 and words.is_cuda
    return words, int(st.cpu().item())


def _unpack(words, K, N, total, table, row_ids=None, **kw):
    from vbq_amd import ops
    st = _status()
    ids = None if row_ids is None else torch.from_numpy(np.asarray(row_ids, dtype=np.int64)).cuda()
    val, idx = ops.records_unpack(words, K, N, total, None if table is None else torch.from_numpy(table).cuda(), ids,
                                  want_values=table is not None, want_idx=True, status=st, **kw)
    return (None if val is None else val.cpu().numpy()), idx.cpu().numpy(), int(st.cpu().item())


def _round_trip(idx, N, total, rng, tables=(1, "K")):
    """Pack equals the restatement byte for byte; unpack gives the indices back and the code points they name."""
    R, K = idx.shape
    want = RR.pack(idx, N, total)
    words, st = _pack(idx, total, N)
    assert st == 0 and tuple(words.shape) == want.shape, (N, K, R, total)
    assert words.cpu().numpy().tobytes() == want.tobytes(), (N, K, R, total)
    for C in tables:
        table = _table(rng, K if C == "K" else 1, N)
        val, got, st = _unpack(words, K, N, total, table)
        assert st == 0 and got.dtype == np.uint16 and np.array_equal(got, idx), (N, K, R, total, C)
        cols = np.arange(K)[None, :] if C == "K" else 0
        assert val.dtype == np.float32 and val.tobytes() == table[cols, idx].tobytes(), (N, K, R, total, C)
    return words


def _budgets(K, N):
    """0, K * N, one value where K * W + total_bits is a multiple of 32 and one where it is not (where K * N has room)."""
    KW = K * N.bit_length()
    aligned = (-KW) % 32 or 32
    out = {0, K * N}
    if aligned <= K * N:
        out.add(aligned)
    for t in (aligned + 1, K * N // 2, 1):
        if 0 <= t <= K * N and (KW + t) % 32:
            out.add(t)
            break
    return sorted(out)


@gpu
@pytest.mark.parametrize("N", [1, 3, 10])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 130, 300])
def test_pack_and_unpack_equal_the_restatement(K, N):
    """K below, at and above one chunk of 64 coordinates and above two and four: the prefix sum's carry; R = 7: more than one
    workgroup.  The one code book is read from LDS at N = 1 and 3 from K = 63 on, through L2 otherwise, as are K code books."""
    _need_gpu()
    rng = np.random.default_rng(100 * K + N)
    for R in (1, 7):
        for total in _budgets(K, N):
            _round_trip(RR.random_indices(rng, R, K, N, total), N, total, rng)


@gpu
def test_rows_of_zero_bit_coordinates_and_a_code_across_a_word_boundary():
    _need_gpu()
    rng = np.random.default_rng(5)
    N, K, total = 10, 130, 50
    n = np.zeros((4, K), dtype=np.int64)
    n[0, :5] = 10                                            # every bit at the front, at the back, in the second chunk, spread
    n[1, -5:] = 10
    n[2, 64:69] = 10
    n[3, ::13] = 5
    assert (n.sum(axis=1) == total).all()
    j = rng.integers(0, 1 << 62, size=n.shape) & ((1 << n) - 1)
    _round_trip(RR.rank_of(n, j, N).astype(np.uint16), N, total, rng)
    # K * W = 28: the first code starts at bit 28 and its 10 bits end at bit 37, in the next word; all ones, then alternating
    N, K, total = 10, 7, 10
    for code in (0x3FF, 0x2AA, 0x155, 0x201):
        n = np.array([[10, 0, 0, 0, 0, 0, 0]])
        idx = RR.rank_of(n, np.array([[code, 0, 0, 0, 0, 0, 0]]), N).astype(np.uint16)
        words = _round_trip(idx, N, total, rng).cpu().numpy()
        assert words.shape == (1, 2) and words[0, 0] >> 28 == code & 0xF and words[0, 1] == code >> 4
    # and one that ends exactly at the boundary: K * W + 4 = 32
    _round_trip(RR.rank_of(np.array([[4, 0, 0, 0, 0, 0, 6]]), np.array([[0xF, 0, 0, 0, 0, 0, 0x3F]]), N).astype(np.uint16), N,
                total, rng)


@gpu
def test_row_ids():
    _need_gpu()
    rng = np.random.default_rng(6)
    N, K, R, total = 10, 65, 7, 301
    idx = RR.random_indices(rng, R, K, N, total)
    table = _table(rng, 1, N)
    words, _ = _pack(idx, total, N)
    for ids in ([], [3, 3, 0, 3], [6, 5, 4, 3, 2, 1, 0], [R - 1], list(rng.integers(0, R, 40))):
        val, got, st = _unpack(words, K, N, total, table, row_ids=ids)
        assert st == 0 and got.shape == (len(ids), K) and np.array_equal(got, idx[np.asarray(ids, dtype=np.int64)]), ids
        assert val.tobytes() == table[0, idx[np.asarray(ids, dtype=np.int64)]].tobytes(), ids
    # a row id the caller failed to check is refused, not read: zeros and bit 3
    val, got, st = _unpack(words, K, N, total, table, row_ids=[1, R, -1])
    assert st == 8 and np.array_equal(got[0], idx[1]) and not got[1:].any() and not val[1:].any()
    # neither output: the validating pass
    from vbq_amd import ops
    st = _status()
    assert ops.records_unpack(words, K, N, total, None, want_values=False, status=st) == (None, None)
    assert int(st.cpu().item()) == 0


@gpu
def test_many_rows_per_workgroup_and_the_table_in_lds_at_n10():
    """More rows than the grid has workgroups (16 per CU): the row loop, and -- from 4 T = 8188 coordinates per workgroup on -- the
    N = 10 code book staged in LDS.  Compared on the device."""
    _need_gpu()
    from vbq_amd import ops
    rng = np.random.default_rng(7)
    N, K, R, total = 10, 300, 32, 1234
    idx = RR.random_indices(rng, R, K, N, total)
    table = torch.from_numpy(_table(rng, 1, N)).cuda()
    n_out = 28 * 16 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    ids = torch.from_numpy(rng.integers(0, R, n_out)).cuda()
    big = torch.from_numpy(idx.astype(np.int64)).cuda()[ids]
    words = ops.records_pack(big.to(torch.uint16), total, N)                                  # n_out rows through the pack's loop
    assert torch.equal(words.view(torch.int32), torch.from_numpy(RR.pack(idx, N, total).view(np.int32)).cuda()[ids])
    st = _status()
    val, got = ops.records_unpack(words, K, N, total, table, want_idx=True, status=st)
    assert int(st.cpu().item()) == 0 and torch.equal(got.view(torch.int16).to(torch.int64) & 0xFFFF, big)
    assert torch.equal(val, table[0][big])
    sel = ids % 1000                                                                          # the same call by lookup
    val2, _ = ops.records_unpack(words, K, N, total, table, sel)
    assert torch.equal(val2, val[sel])


@gpu
def test_pack_refuses_rows_outside_the_contract():
    _need_gpu()
    rng = np.random.default_rng(8)
    N, K, R, total = 10, 70, 5, 222
    idx = RR.random_indices(rng, R, K, N, total)
    want = RR.pack(idx, N, total)
    for row, delta in ((2, +1), (4, -1)):                                                 # lengths that add up to total +/- 1
        bad = idx.copy()
        lev = RR.length_and_code(bad[row], N)[0]
        k = int(np.flatnonzero((lev > 0) & (lev < N))[-1])
        n, j = RR.length_and_code(bad[row, k], N)
        bad[row, k] = RR.rank_of(n + delta, j >> 1 if delta < 0 else j << 1, N)
        words, st = _pack(bad, total, N)
        w = words.cpu().numpy()
        assert st == 2 and not w[row].any() and np.array_equal(np.delete(w, row, 0), np.delete(want, row, 0))
    words, st = _pack(np.full((2, 9), 2046, np.uint16), 90, N)                            # every coordinate at N bits: fine
    assert st == 0
    words, st = _pack(np.full((2, 9), 2046, np.uint16), 89, N)                            # one bit over the budget
    assert st == 2 and not words.cpu().numpy().any()
    bad = RR.random_indices(rng, 3, 20, 3, 17)                                            # N = 3: T = 15
    want = RR.pack(bad, 3, 17)
    bad[1, 7] = 15
    words, st = _pack(bad, 17, 3)
    w = words.cpu().numpy()
    assert st & 1 and not w[1].any() and np.array_equal(w[[0, 2]], want[[0, 2]])
    bad[1, 7] = 65535
    assert _pack(bad, 17, 3)[1] & 1


def _latents(rng, R, K, per_column, N):
    import vbq_amd
    scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), K)) if per_column else np.array([1.0])
    tab = vbq_amd.gaussian_table(scale, N=N)                                                  # [K, T] / [1, T]
    mu = (scale * rng.standard_normal((R, K))).astype(np.float32)
    sg = np.clip(np.exp(-2 + 0.7 * rng.standard_normal((R, K))), 1e-4, 10).astype(np.float32)
    return mu, sg, (tab if per_column else tab[0])


@gpu
@pytest.mark.parametrize("per_column", [False, True])
@pytest.mark.parametrize("R,K,total", [(30, 12, 41), (60, 16, 64)])
def test_record_files_of_budget_rows(R, K, total, per_column):
    """compress_to_records -> RecordEmbeddings.tensor / rows / decompress give table_sorted[idx] of quantize_rows_to_budget bit
    for bit; the file is as long as records_nbytes says; the budget form takes the largest total_bits that fits."""
    _need_gpu()
    import vbq_amd
    from vbq_amd import bitstream as bs, embeddings as E, tables
    N = 10
    mu, sg, tab = _latents(np.random.default_rng(R + K), R, K, per_column, N)
    C = K if per_column else 1
    idx, num_bits, _ = vbq_amd.quantize_rows_to_budget(mu, sg, total, table=tab, N=N)
    idx = idx.cpu().numpy().astype(np.int64)
    srt = tables.level_major_to_sorted(np.asarray(tab, np.float32).reshape(C, -1))
    want = srt[np.arange(K)[None, :] if per_column else 0, idx]
    data = E.compress_to_records(mu, sg, total, tab, N=N)
    assert isinstance(data, bytes) and data[:4] == b"VBQr" and len(data) == bs.records_nbytes((R, K), N, total, C)
    h, table, off = bs.parse_records(data)
    assert h.shape == (R, K) and h.C == C and h.total_bits == total and table.tobytes() == srt.tobytes()
    assert np.frombuffer(data, "<u4", offset=off).tobytes() == RR.pack(idx, N, total).tobytes()
    emb = E.RecordEmbeddings(data)
    assert emb.shape == (R, K) and emb.total_bits == total and emb.bits_per_coordinate == 8.0 * len(data) / (R * K)
    t = emb.tensor()
    assert t.is_cuda and t.dtype == torch.float32 and t.cpu().numpy().tobytes() == want.tobytes()
    for ids in ([], [R - 1], [5, 5, 0], list(range(R - 1, -1, -1)), np.array([2, 7], np.int32), torch.tensor([1, 0])):
        got = emb.rows(ids).cpu().numpy()
        sel = np.asarray(ids, dtype=np.int64)
        assert got.shape == (len(sel), K) and got.tobytes() == want[sel].tobytes()
    with pytest.raises(IndexError, match=f"row {R} outside"):
        emb.rows([0, R])
    with pytest.raises(IndexError, match="row -1 outside"):
        emb.rows([-1])
    with pytest.raises(IndexError, match="integers"):
        emb.rows([0.5])
    with pytest.raises(ValueError, match="one-dimensional"):
        emb.rows([[0]])
    assert E.decompress(data).tobytes() == want.tobytes()
    assert E.decompress(data, return_np=False).is_cuda
    # a three-dimensional matrix: rows are the slices along axis 0
    d3 = E.compress_to_records(mu.reshape(R, 2, K // 2), sg.reshape(R, 2, K // 2), total, tab, N=N)
    assert d3[24:48] == np.array([R, 2, K // 2], "<u8").tobytes() and d3[48:] == data[40:]
    assert E.RecordEmbeddings(d3).rows([3]).shape == (1, 2, K // 2)
    # the byte budget
    for max_bytes in (len(data), len(data) - 1, bs.records_nbytes((R, K), N, 0, C), bs.records_nbytes((R, K), N, K * N, C) + 99):
        b = E.compress_to_records_budget(mu, sg, tab, max_bytes, N=N)
        tb = bs.parse_records(b)[0].total_bits
        assert len(b) <= max_bytes and tb == bs.records_total_bits_within((R, K), N, C, max_bytes)
        assert tb == K * N or bs.records_nbytes((R, K), N, tb + 1, C) > max_bytes
        i2, _, _ = vbq_amd.quantize_rows_to_budget(mu, sg, tb, table=tab, N=N)
        assert E.decompress(b).tobytes() == srt[np.arange(K)[None, :] if per_column else 0, i2.cpu().numpy().astype(np.int64)].tobytes()
    with pytest.raises(ValueError, match="smallest file"):
        E.compress_to_records_budget(mu, sg, tab, bs.records_nbytes((R, K), N, 0, C) - 1, N=N)
    # the rANS file still decodes through the same call
    if not per_column:
        cp = tables.sorted_to_level_major(srt[0]).astype(np.float64)
        e = E.compress_to_bytes(mu, sg, 1.0, cp)
        assert e[:4] == b"VBQe" and E.decompress(e).shape == (R, K)


@gpu
def test_damaged_records_raise_at_load_and_decode_to_zeros():
    """Damage applied to the bytes of a valid file: a length nibble above N, a length changed so that the sum is off, a padding
    bit set.  None of them can make the kernel read outside the record."""
    _need_gpu()
    import vbq_amd
    from vbq_amd import bitstream as bs, embeddings as E
    N, R, K, total = 10, 30, 12, 41                           # K * W + total = 89 bits: 3 words, 7 bits of padding
    mu, sg, tab = _latents(np.random.default_rng(9), R, K, False, N)
    data = E.compress_to_records(mu, sg, total, tab, N=N)
    h, table, off = bs.parse_records(data)
    good = np.frombuffer(data, "<u4", offset=off).reshape(R, h.record_words).copy()
    idx = RR.unpack(good, K, N, total)
    lengths = RR.length_and_code(idx, N)[0]
    row = 17
    k = int(np.flatnonzero(lengths[row] < N)[0])
    damage = {
        "a length field above N": (1, lambda w: w.__setitem__((row, 0), (w[row, 0] & ~np.uint32(0xF)) | np.uint32(0xD))),
        "lengths that do not add up": (2, lambda w: w.__setitem__((row, k // 8), w[row, k // 8] + (np.uint32(1) << np.uint32(4 * (k % 8))))),
        "non-zero padding": (4, lambda w: w.__setitem__((row, 2), w[row, 2] | np.uint32(1 << 31))),
    }
    for what, (bit, apply) in damage.items():
        w = good.copy()
        apply(w)
        assert not np.array_equal(w, good)
        bad = data[:off] + w.tobytes()
        assert bs.parse_records(bad)[0] == h                 # the host cannot see it
        with pytest.raises(vbq_amd.VBQError, match=what):
            E.RecordEmbeddings(bad)
        with pytest.raises(vbq_amd.VBQError, match=what):
            E.decompress(bad)
        val, got, st = _unpack(torch.from_numpy(w.view(np.int32)).cuda().view(torch.uint32), K, N, total, np.array(table))
        assert st & bit, (what, st)
        assert not got[row].any() and not val[row].any(), what
        assert np.array_equal(np.delete(got, row, 0), np.delete(idx, row, 0)), what
    # every length at 15 and every bit set: nothing but zeros comes back, whatever the record says
    w = np.full_like(good, 0xFFFFFFFF)
    val, got, st = _unpack(torch.from_numpy(w.view(np.int32)).cuda().view(torch.uint32), K, N, total, np.array(table))
    assert st & 1 and not got.any() and not val.any()
