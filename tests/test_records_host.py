"""The record file ("VBQr", vbq_amd.bitstream) on the host: the format's known answer through the NumPy restatement
(tests/records_reference.py), write -> parse, the closed-form file length and the budget rule built on it, one message of its
own for every malformed field, the other parsers' refusal of the magic, and the C entry points' argument checks, which need no
device."""
import math
import struct

import numpy as np
import pytest

import records_reference as RR
from vbq_amd import bitstream as bs


def _valid(shape=(5, 7), N=10, total_bits=23, per_column=False, seed=0):
    rng = np.random.default_rng(seed)
    K = math.prod(shape[1:])
    C = K if per_column else 1
    T = 2 ** (N + 1) - 1
    table = np.sort(rng.normal(size=(C, T)).astype(np.float32), axis=1)
    words = RR.pack(RR.random_indices(rng, shape[0], K, N, total_bits), N, total_bits)
    h = bs.RecordsHeader(N=N, shape=tuple(shape), C=C, total_bits=total_bits)
    return h, table, words, bs.write_records(h, table, words)


def _patch(data, offset, fmt, value):
    b = bytearray(data)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


def test_known_answer():
    """The example of the specification, written out: N = 3, K = 3, lengths (2, 0, 1), codes (2, -, 1), total_bits = 3."""
    idx = np.array([[9, 7, 11]])
    n, j = RR.length_and_code(idx[0], 3)
    assert n.tolist() == [2, 0, 1] and j.tolist() == [2, 0, 1]
    assert RR.rank_of([2, 0, 1], [2, 0, 1], 3).tolist() == [9, 7, 11]
    words = RR.pack(idx, 3, 3)
    assert words.shape == (1, 1) and words.tobytes() == bytes([0x92, 0x01, 0x00, 0x00])
    assert RR.unpack(np.frombuffer(bytes([0x92, 0x01, 0x00, 0x00]), "<u4").reshape(1, 1), 3, 3, 3).tolist() == [[9, 7, 11]]
    assert [N.bit_length() for N in (1, 3, 10)] == [1, 2, 4]


def test_reference_round_trip_and_refusals():
    from vbq_amd import tables
    rng = np.random.default_rng(1)
    for N, K, total in ((1, 5, 3), (3, 9, 13), (10, 70, 333), (10, 6, 0), (7, 6, 42)):
        idx = RR.random_indices(rng, 4, K, N, total)
        assert np.array_equal(tables.level_of_rank(N)[idx].sum(axis=1), np.full(4, total))
        words = RR.pack(idx, N, total)
        assert words.shape == (4, RR.record_words(K, N, total))
        assert np.array_equal(RR.unpack(words, K, N, total), idx)
    words = RR.pack(np.array([[9, 7, 11]]), 3, 3)
    for bad, what in ((words ^ 0x10, "add up"), (words | 0x80000000, "padding")):
        with pytest.raises(ValueError, match=what):
            RR.unpack(bad, 3, 3, 3)
    with pytest.raises(ValueError, match="length above N"):          # W = 4 bits hold up to 15, N = 10 allows up to 10
        RR.unpack(RR.pack(np.array([[1023, 1023]]), 10, 0) | 0xB, 2, 10, 0)


def test_write_then_parse():
    for shape, N, total, per_column in (((5, 7), 10, 23, False), ((5, 7), 10, 23, True), ((3,), 3, 2, False),
                                        ((2, 3, 4), 1, 12, True), ((4, 2, 64), 10, 0, False), ((1, 1), 10, 10, True)):
        h, table, words, data = _valid(shape, N, total, per_column)
        assert data[:4] == b"VBQr" and h.records_offset % 8 == 0 and len(data) % 4 == 0
        got, gt, off = bs.parse_records(data)
        assert got == h and got.n_rows == shape[0] and got.row_length == math.prod(shape[1:]) and got.n == math.prod(shape)
        assert got.record_words == RR.record_words(got.row_length, N, total) and got.length_bits == N.bit_length()
        assert gt.dtype == np.dtype("<f4") and gt.shape == table.shape and gt.tobytes() == table.tobytes()
        assert off == h.records_offset and np.array_equal(np.frombuffer(data, "<u4", offset=off).reshape(words.shape), words)
        assert bs.parse_records(bytearray(data))[0] == h and bs.parse_records(memoryview(data))[0] == h
    h, table, words, _ = _valid()
    with pytest.raises(ValueError, match="code points"):
        bs.write_records(h, table[:, :-1], words)
    with pytest.raises(ValueError, match="record words"):
        bs.write_records(h, table, words[:-1])
    with pytest.raises(ValueError, match="non-finite"):
        bs.write_records(h, np.where(np.arange(table.size) == 3, np.inf, table.reshape(-1)), words)
    with pytest.raises(ValueError, match="neither 1"):
        bs.write_records(bs.RecordsHeader(N=10, shape=(5, 7), C=2, total_bits=23), table, words)


def test_records_nbytes_is_the_length_of_the_file():
    for shape, N, total, per_column in (((5, 7), 10, 23, False), ((5, 7), 10, 23, True), ((5, 8), 10, 23, True),
                                        ((3,), 3, 2, False), ((2, 3, 4), 1, 12, True), ((4, 2, 64), 10, 0, False),
                                        ((6, 2), 4, 8, True), ((9, 33), 10, 4, False), ((9, 33), 10, 5, True)):
        h, table, _, data = _valid(shape, N, total, per_column)
        assert bs.records_nbytes(shape, N, total, h.C) == len(data), (shape, N, total, per_column)
        assert (h.C * h.T) % 2 == h.C % 2 and h.table_nbytes == 4 * h.C * h.T + 4 * (h.C % 2)      # odd and even C * T
    assert bs.records_nbytes((100_000, 100), 10, 300, 1) == 24 + 16 + 4 * 2047 + 4 + 100_000 * 4 * 22
    with pytest.raises(ValueError, match="total_bits"):
        bs.records_nbytes((5, 7), 10, 71, 1)
    with pytest.raises(ValueError, match="limit of 8192"):
        bs.records_nbytes((2, 70_000), 10, 0, 1)


def test_total_bits_within_is_the_largest_that_fits():
    for shape, N, C in (((5, 7), 10, 1), ((5, 7), 10, 7), ((100, 33), 3, 1), ((7, 300), 10, 300), ((3,), 1, 1)):
        K = math.prod(shape[1:])
        least, most = bs.records_nbytes(shape, N, 0, C), bs.records_nbytes(shape, N, K * N, C)
        for budget in sorted({least, least + 1, least + 4 * shape[0], (least + most) // 2, max(least, most - 1), most, most + 1000}):
            t = bs.records_total_bits_within(shape, N, C, budget)
            assert bs.records_nbytes(shape, N, t, C) <= budget
            assert t == K * N or bs.records_nbytes(shape, N, t + 1, C) > budget, (shape, N, C, budget)
        assert bs.records_total_bits_within(shape, N, C, most) == K * N
        with pytest.raises(ValueError, match=f"smallest file .* is {least} bytes"):
            bs.records_total_bits_within(shape, N, C, least - 1)
    with pytest.raises(TypeError):
        bs.records_total_bits_within((5, 7), 10, 1, 1e6)
    # the kernels' record limit caps the budget as well: K W = 4 * 60 000 bits leave 8192 * 32 - 240 000 bits for codes
    assert bs.records_total_bits_within((2, 60_000), 10, 1, 10 ** 9) == 8192 * 32 - 240_000


def test_every_malformed_field_has_a_message_of_its_own():
    h, table, words, data = _valid((5, 7), 10, 23, False)                 # C * T odd: 4 bytes of table padding
    assert h.table_nbytes == 4 * h.T + 4
    cases = [
        (b"VBQx" + data[4:], "not a VBQ record file"),
        (b"VBQe" + data[4:], "compressed embedding matrix"),
        (b"VBQb" + data[4:], "latent bitstream in segments"),
        (b"VBQc" + data[4:], "compact latent bitstream"),
        (_patch(data, 4, "<B", 2), "unknown record file version 2"),
        (_patch(data, 5, "<B", 0), r"N = 0 outside \[1, 10\]"),
        (_patch(data, 5, "<B", 11), r"N = 11 outside \[1, 10\]"),
        (_patch(data, 6, "<B", 0), "0 dimensions"),
        (_patch(data, 7, "<B", 1), "reserved header byte is 1"),
        (_patch(data, 20, "<I", 9), "reserved header word is 9"),
        (_patch(data, 8, "<I", 2), "C = 2 is neither 1 .* nor K = 7"),
        (_patch(data, 8, "<I", 0), "C = 0 is neither 1"),
        (_patch(data, 12, "<I", 71), r"total_bits 71 outside \[0, K\*N = 70\]"),
        (_patch(data, 16, "<I", h.record_words + 1), f"record_words is {h.record_words + 1}, .* need {h.record_words}"),
        (_patch(data, 24, "<Q", 0), "empty matrix shape"),
        (_patch(data, 24, "<Q", 2 ** 62), "too large"),
        (_patch(data, h.nbytes + 4 * 5, "<f", float("nan")), "non-finite code point"),
        (_patch(data, h.nbytes + 4 * 5, "<f", float("-inf")), "non-finite code point"),
        (_patch(data, h.nbytes + 4 * h.T + 1, "<B", 1), "padding after the code-point table is not zero"),
        (data[:10], "truncated: 10 bytes, the fixed header alone is 24"),
        (data[:30], "truncated in the matrix shape"),
        (data[:h.nbytes + 100], "truncated in the code-point table"),
        (data[:h.records_offset - 2], "truncated in the code-point table"),
        (data[:h.records_offset + 7], "truncated: .* records"),
        (data[:-1], "truncated: .* records"),
        (data + b"\0", "1 trailing bytes"),
        (b"", "truncated"),
    ]
    seen = set()
    for bad, msg in cases:
        with pytest.raises(ValueError, match=msg) as e:
            bs.parse_records(bad)
        seen.add(str(e.value))
    assert len(seen) >= len(cases) - 3                                    # (the two NaN/inf and two table truncations share one)
    # a record above the kernels' limit: a header that is consistent in itself, K W = 4 * 70 000 bits > 8192 words
    big = struct.pack("<4sBBBBIIII", b"VBQr", 1, 10, 2, 0, 1, 0, 8750, 0) + np.array([2, 70_000], "<u8").tobytes()
    with pytest.raises(ValueError, match="a record of 8750 words exceeds the limit of 8192"):
        bs.parse_records(big)
    for bad, _ in cases:                                                  # never struct.error or IndexError: checked above by
        try:                                                              # pytest.raises(ValueError); bytearray input as well
            bs.parse_records(bytearray(bad))
        except ValueError:
            pass


def test_the_other_parsers_reject_the_new_magic():
    _, _, _, data = _valid()
    for parse in (bs.parse, bs.parse_compact, bs.parse_latent, bs.parse_embeddings):
        with pytest.raises(ValueError, match="VBQr"):
            parse(data)


def test_entry_points_check_their_arguments_without_a_device():
    import ctypes as C
    from vbq_amd import _lib
    h = _lib.lib()
    for K, N, total in ((3, 3, 3), (100, 10, 300), (1, 1, 0), (1, 1, 1), (300, 10, 3000), (7, 5, 20), (64, 10, 384)):
        assert h.vbq_records_words(K, N, total) == RR.record_words(K, N, total) == bs.RecordsHeader(N, (1, K), 1, total).record_words
    for K, N, total in ((0, 10, 0), (5, 0, 0), (5, 11, 0), (5, 10, -1), (5, 10, 51)):
        assert h.vbq_records_words(K, N, total) == 0
    pack, unpack = h.vbq_records_pack_u16, h.vbq_records_unpack_f32
    assert pack(None, -1, 5, 10, 7, None, None, None) == -1 and b"bad sizes" in h.vbq_last_error()
    assert pack(None, 4, 0, 10, 0, None, None, None) == -1 and b"bad sizes" in h.vbq_last_error()
    assert pack(None, 4, 5, 11, 7, None, None, None) == -1 and b"bad sizes" in h.vbq_last_error()
    assert pack(None, 4, 5, 10, 51, None, None, None) == -1 and b"total_bits 51 outside" in h.vbq_last_error()
    assert pack(None, 4, 70_000, 10, 0, None, None, None) == -2 and b"exceeds the limit of 8192" in h.vbq_last_error()
    assert pack(None, 4, 5, 10, 7, None, None, None) == -1 and b"null pointer" in h.vbq_last_error()
    assert pack(None, 0, 5, 10, 7, None, None, None) == 0                                   # no rows: nothing to do
    assert unpack(None, 4, 5, 10, 51, None, 1, None, 0, None, None, None, None) == -1 and b"total_bits" in h.vbq_last_error()
    assert unpack(None, 4, 5, 10, 7, None, 2, None, 0, None, None, None, None) == -1 and b"neither 1 nor K" in h.vbq_last_error()
    assert unpack(None, 4, 5, 10, 7, None, 1, None, 0, None, None, None, None) == -1 and b"null pointer" in h.vbq_last_error()
    assert unpack(None, 4, 70_000, 10, 0, None, 1, None, 0, None, None, None, None) == -2
    assert unpack(None, 0, 5, 10, 7, None, 5, None, 0, None, None, None, None) == 0
    ids = (C.c_int64 * 1)(0)
    assert unpack(None, 4, 5, 10, 7, None, 1, ids, -1, None, None, None, None) == -1 and b"n_sel" in h.vbq_last_error()
    assert unpack(None, 4, 5, 10, 7, None, 1, ids, 0, None, None, None, None) == 0            # no row asked for
    # the Python layer: sizes are checked before anything touches a device
    from vbq_amd import embeddings, ops
    with pytest.raises(ValueError, match="no record"):
        ops.records_words(5, 10, 51)
    cp = np.zeros(2047)
    with pytest.raises(ValueError, match="total_bits 71 outside"):
        embeddings.compress_to_records(np.zeros((5, 7), np.float32), np.ones((5, 7), np.float32), 71, cp)
    with pytest.raises(ValueError, match="smallest file"):
        embeddings.compress_to_records_budget(np.zeros((5, 7), np.float32), np.ones((5, 7), np.float32), cp, 100)
    with pytest.raises(ValueError, match="empty matrix"):
        embeddings.compress_to_records(np.zeros((0, 7), np.float32), np.zeros((0, 7), np.float32), 0, cp)
