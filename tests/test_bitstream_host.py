"""vbq_amd.bitstream on the host: the container header writes and parses back, and every malformed file raises ValueError
with a message of its own (never struct.error / IndexError), before anything could reach the device."""
import math
import struct

import numpy as np
import pytest

from vbq_amd import bitstream as bs

SEG = 64


def _valid(shape=(2, 17, 23, 8), seg=SEG, lamb=0.125, seed=0):
    rng = np.random.default_rng(seed)
    C = shape[-1]
    nseg = (math.prod(shape) // C + seg - 1) // seg
    sizes = rng.integers(2, seg + 3, C * nseg).astype(np.uint32)
    payload = rng.integers(0, 65536, int(sizes.sum())).astype(np.uint16)
    h = bs.Header(N=10, C=C, shape=tuple(shape), lamb=lamb, segment=seg, digest=bytes(range(16)), n_words=int(sizes.sum()))
    return h, sizes, payload, bs.write(h, sizes, payload)


def _patch(data, offset, fmt, value):
    b = bytearray(data)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


def test_header_round_trip():
    for shape, seg in (((1, 32, 48, 256), 1024), ((2, 17, 23, 8), 64), ((1000, 1), 7), ((5,), 65533)):
        h, sizes, payload, data = _valid(shape, seg, lamb=2.0 ** -5.5)
        assert data[:4] == b"VBQb" and len(data) % 2 == 0 and h.nbytes % 8 == 0
        got, gs, off = bs.parse(data)
        assert got == h
        assert got.n_rows == math.prod(shape) // shape[-1] and got.nseg == -(-got.n_rows // seg)
        assert np.array_equal(gs, sizes) and gs.dtype == np.dtype("<u2")
        assert off == h.nbytes + 2 * h.n_sizes and len(data) == off + 2 * h.n_words
        assert np.array_equal(np.frombuffer(data, "<u2", offset=off), payload)
        assert bs.parse(bytearray(data))[0] == h and bs.parse(memoryview(data))[0] == h


def test_digest_covers_code_points_and_frequencies():
    rng = np.random.default_rng(3)
    tab = np.sort(rng.normal(size=(4, 2047)).astype(np.float32), axis=1)
    freq = np.full((4, 2047), 16, np.uint16)
    d = bs.digest(tab, freq)
    assert len(d) == 16 and d == bs.digest(tab.copy(), freq.copy())
    t2 = tab.copy()
    t2[1, 5] = np.nextafter(t2[1, 5], np.float32(np.inf))
    f2 = freq.copy()
    f2[3, 0] += 1
    f2[3, 1] -= 1
    assert len({d, bs.digest(t2, freq), bs.digest(tab, f2)}) == 3


def test_every_truncation_raises_value_error():
    h, _, _, data = _valid((2, 5, 7, 4), seg=16)
    for n in range(len(data)):
        with pytest.raises(ValueError):
            bs.parse(data[:n])


@pytest.mark.parametrize("case,match", [
    ("magic", "magic"), ("version", "version"), ("reserved", "reserved"), ("trailing", "trailing"),
    ("nan", "non-finite"), ("inf", "non-finite"), ("ndim0", "0 dimensions"), ("N0", "N = 0"), ("N11", "N = 11"),
    ("not_channel_last", "channel-last"), ("zero_dim", "empty"), ("nseg", "truncated|trailing"), ("C0", "zero channels"),
    ("segment0", "segment 0"), ("segment_big", "segment 65534"), ("size0", "segment size 0"), ("size1", "segment size 1"),
    ("size_big", f"segment size {SEG + 3}"), ("sum", "add up"), ("n_words", "add up|truncated|trailing"),
])
def test_malformed_headers(case, match):
    h, sizes, payload, data = _valid()
    sz = h.nbytes                                      # first size
    d = {
        "magic": lambda: b"VBQc" + data[4:],
        "version": lambda: _patch(data, 4, "<B", 2),
        "reserved": lambda: _patch(data, 7, "<B", 1),
        "trailing": lambda: data + b"\0\0",
        "nan": lambda: _patch(data, 16, "<d", float("nan")),
        "inf": lambda: _patch(data, 16, "<d", float("-inf")),
        "ndim0": lambda: _patch(data, 6, "<B", 0),
        "N0": lambda: _patch(data, 5, "<B", 0),
        "N11": lambda: _patch(data, 5, "<B", 11),
        "not_channel_last": lambda: _patch(data, 48 + 8 * 3, "<Q", 7),       # shape[-1] != C: product not a multiple of C
        "zero_dim": lambda: _patch(data, 48, "<Q", 0),
        "nseg": lambda: _patch(data, 48 + 8, "<Q", 40),                    # another row count: another number of segments
        "C0": lambda: _patch(data, 8, "<I", 0),
        "segment0": lambda: _patch(data, 12, "<I", 0),
        "segment_big": lambda: _patch(data, 12, "<I", 65534),
        "size0": lambda: _patch(data, sz + 2 * 5, "<H", 0),
        "size1": lambda: _patch(data, sz + 2 * 5, "<H", 1),
        "size_big": lambda: _patch(data, sz + 2 * 5, "<H", SEG + 3),
        "sum": lambda: _patch(_patch(data, sz, "<H", 2 if sizes[0] > 2 else 3), sz + 2, "<H", int(sizes[1])),
        "n_words": lambda: _patch(data, 24, "<Q", h.n_words - 1)[:-2],
    }[case]()
    with pytest.raises(ValueError, match=match):
        bs.parse(d)


def test_shape_not_a_multiple_of_c():
    h, sizes, payload, data = _valid()
    for bad in (bs.Header(N=10, C=8, shape=(3, 5), lamb=1.0, segment=SEG, digest=bytes(16), n_words=0),
                bs.Header(N=10, C=8, shape=(3, 8), lamb=float("inf"), segment=SEG, digest=bytes(16), n_words=0)):
        with pytest.raises(ValueError):
            bs.write(bad, [], [])
    with pytest.raises(ValueError, match="segment sizes"):
        bs.write(h, sizes[:-1], payload)
    with pytest.raises(ValueError, match="payload"):
        bs.write(h, sizes, payload[:-1].copy())
    with pytest.raises(ValueError, match="segment size"):
        s2 = sizes.copy()
        s2[0] = SEG + 3
        bs.write(h, s2, payload)


def test_pack_unpack_entry_points_validate_before_touching_the_device():
    from vbq_amd import _lib, build
    build.build_hip()
    h = _lib.lib()
    assert h.vbq_rans_pack_u16(None, None, 1, 10, 0, None, None, None, None) == -1 and b"bad sizes" in h.vbq_last_error()
    assert h.vbq_rans_pack_u16(None, None, 1, 10, 4, None, None, None, None) == -1 and b"d_total" in h.vbq_last_error()
    assert h.vbq_rans_unpack_u16(None, -1, None, 1, 10, 4, None, None, None, None, None) == -1
    assert h.vbq_rans_unpack_u16(None, 0, None, 1, 10, 4, None, None, None, None, None) == -1
    assert b"null pointer" in h.vbq_last_error()
    assert h.vbq_rans_unpack_u16(None, 3, None, 0, 10, 4, None, None, None, None, None) == -1
    assert b"d_payload" in h.vbq_last_error()


# ---------------------------------------------------------------------------------------------------------------------------
# The three formats pinned byte for byte, and every ValueError text of the two latent parsers pinned character for character.
# The digests, lengths and messages below were recorded from the implementation that wrote each format on its own (the commit
# before the latent formats were given one writer and one parser); they are constants, not recomputed.
# ---------------------------------------------------------------------------------------------------------------------------
import hashlib

_DIG = bytes(range(16))


def _pinned_segments():
    """VBQb, shape (3, 5, 4), C = 4, segment = 4: 4 streams of 15 symbols, 16 sizes at their lower bound 2."""
    sizes = np.full(16, 2)
    h = bs.Header(N=10, C=4, shape=(3, 5, 4), lamb=0.25, segment=4, digest=_DIG, n_words=32)
    return h, sizes, bs.write(h, sizes, np.arange(32))


def _pinned_compact():
    """VBQc of the same shape, part = 7: 9 parts (odd: the padding is there), the last one of 4 symbols; sizes at 128."""
    sizes = np.full(9, 128)
    h = bs.CompactHeader(N=10, C=4, shape=(3, 5, 4), lamb=0.25, part=7, digest=_DIG, n_words=9 * 128)
    return h, sizes, bs.write_compact(h, sizes, np.arange(9 * 128))


def _pinned_embeddings():
    """VBQe, shape (6, 5), segment = 10, K = 3: 3 segments at their lower bound 2."""
    table = np.zeros(3, dtype=bs.TABLE_DTYPE)
    table["rank"], table["freq"], table["value"] = [0, 1, 2], [16384, 8192, 8192], [-1.0, 0.0, 1.0]
    h = bs.EmbeddingHeader(N=10, shape=(6, 5), segment=10, beta=0.5, empirical_std=1.0, n_words=6, K=3)
    return h, table, bs.write_embeddings(h, table, np.full(3, 2), np.arange(6))


PINNED = {"segments": (168, "e9c15b5fb4f083132dd43322e6cb840b"), "compact": (2416, "9a35a3c8bc17720f5ce42f8c9a40d7ee"),
          "embeddings": (98, "7e40af1f4d2ec3cd840c708eed9c3fd2")}


@pytest.mark.parametrize("name,build", [("segments", _pinned_segments), ("compact", _pinned_compact),
                                        ("embeddings", _pinned_embeddings)])
def test_written_files_are_pinned_byte_for_byte(name, build):
    data = build()[-1]
    assert (len(data), hashlib.blake2b(data, digest_size=16).hexdigest()) == PINNED[name]


def _malformed(fmt, case):
    """One malformation of the pinned file of `fmt` ("segments" / "compact")."""
    h, sizes, data = _pinned_segments() if fmt == "segments" else _pinned_compact()
    compact = fmt == "compact"
    w = "<I" if compact else "<H"                                # a size
    at = lambda i: h.nbytes + struct.calcsize(w) * i
    return {
        "fixed": lambda: data[:47],
        "magic": lambda: b"VBQx" + data[4:],
        "other_magic": lambda: (b"VBQb" if compact else b"VBQc") + data[4:],
        "version": lambda: _patch(data, 4, "<B", 2),
        "reserved": lambda: _patch(data, 7, "<B", 1),
        "ndim0": lambda: _patch(data, 6, "<B", 0),
        "shape": lambda: data[:48 + 8 * 3 - 1],
        "unit": lambda: _patch(data, 12, "<I", 0),
        "unit_big": lambda: _patch(data, 12, "<I", (1 << 24) + 1 if compact else 65534),
        "tail": lambda: data[:-1],
        "trailing": lambda: data + b"\0\0",
        "size_small": lambda: _patch(data, at(1), w, 127 if compact else 1),
        "size_big": lambda: _patch(data, at(8), w, 133 if compact else 7),    # (the last part holds 4 symbols: 132 at most)
        "sum": lambda: _patch(data, at(0), w, 129 if compact else 3),
        "padding": lambda: _patch(data, at(9), "<I", 1 << 16),
    }[case]()


MESSAGES = {
    ("segments", "fixed"): 'truncated: 47 bytes, the fixed header alone is 48',
    ("segments", "magic"): "not a VBQ bitstream (magic b'VBQx')",
    ("segments", "other_magic"): "not a VBQ bitstream (magic b'VBQc')",
    ("segments", "version"): 'unknown bitstream version 2',
    ("segments", "reserved"): 'reserved header byte is 1, not 0',
    ("segments", "ndim0"): 'latent shape with 0 dimensions',
    ("segments", "shape"): 'truncated in the latent shape: 71 bytes, the header is 72',
    ("segments", "unit"): 'segment 0 outside [1, 65533]',
    ("segments", "unit_big"): 'segment 65534 outside [1, 65533]',
    ("segments", "tail"): 'truncated: 167 bytes, header, 16 segment sizes and 32 payload words need 168',
    ("segments", "trailing"): '2 trailing bytes after the payload',
    ("segments", "size_small"): 'segment size 1 at position 1 outside [2, 6]',
    ("segments", "size_big"): 'segment size 7 at position 8 outside [2, 6]',
    ("segments", "sum"): 'segment sizes add up to 33 words, the header says 32',
    ("compact", "fixed"): 'truncated: 47 bytes, the fixed header alone is 48',
    ("compact", "magic"): "not a compact VBQ bitstream (magic b'VBQx')",
    ("compact", "other_magic"): "a latent bitstream in segments (magic b'VBQb'), not a compact one",
    ("compact", "version"): 'unknown compact bitstream version 2',
    ("compact", "reserved"): 'reserved header byte is 1, not 0',
    ("compact", "ndim0"): 'latent shape with 0 dimensions',
    ("compact", "shape"): 'truncated in the latent shape: 71 bytes, the header is 72',
    ("compact", "unit"): 'part 0 outside [1, 16777216]',
    ("compact", "unit_big"): 'part 16777217 outside [1, 16777216]',
    ("compact", "tail"): 'truncated: 2415 bytes, header, 9 part sizes and 1152 payload words need 2416',
    ("compact", "trailing"): '2 trailing bytes after the payload',
    ("compact", "size_small"): 'part size 127 at position 1 outside [128, 135]',
    ("compact", "size_big"): 'part size 133 at position 8 outside [128, 132]',
    ("compact", "sum"): 'part sizes add up to 1153 words, the header says 1152',
    ("compact", "padding"): 'padding after the part sizes is not zero',
}


@pytest.mark.parametrize("fmt,case", sorted(MESSAGES))
def test_every_parse_message_is_pinned(fmt, case):
    with pytest.raises(ValueError) as e:
        (bs.parse if fmt == "segments" else bs.parse_compact)(_malformed(fmt, case))
    assert str(e.value) == MESSAGES[fmt, case]


def test_shared_tail_messages_of_the_embedding_file_and_the_writers_are_pinned():
    h, table, d = _pinned_embeddings()
    for bad, msg in ((d[:39], "truncated: 39 bytes, the fixed header alone is 40"),
                     (d[:55], "truncated in the matrix shape: 55 bytes, the header is 56"),
                     (d[:79], "truncated in the symbol table: 79 bytes, header and table need 80"),
                     (d[:-1], "truncated: 97 bytes, header, table, 3 segment sizes and 6 payload words need 98"),
                     (d + b"\0\0", "2 trailing bytes after the payload")):
        with pytest.raises(ValueError) as e:
            bs.parse_embeddings(bad)
        assert str(e.value) == msg
    hs, hc = _pinned_segments()[0], _pinned_compact()[0]
    for call, msg in ((lambda: bs.write_embeddings(h, table, np.full(2, 2), np.arange(6)), "2 segment sizes, the shape needs 3"),
                      (lambda: bs.write_embeddings(h, table, np.full(3, 2), np.arange(5)), "payload of 5 words, the header says 6"),
                      (lambda: bs.write(hs, np.full(15, 2), np.arange(32)), "15 segment sizes, the shape needs 16"),
                      (lambda: bs.write(hs, np.full(16, 2), np.arange(31)), "payload of 31 words, the header says 32"),
                      (lambda: bs.write_compact(hc, np.full(8, 128), np.arange(1152)), "8 part sizes, the shape needs 9"),
                      (lambda: bs.write_compact(hc, np.full(9, 128), np.arange(1151)), "payload of 1151 words, the header says 1152")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == msg


def test_parse_latent_reads_either_latent_file():
    for build, parse in ((_pinned_segments, bs.parse), (_pinned_compact, bs.parse_compact)):
        h, sizes, data = build()
        want, got = parse(data), bs.parse_latent(data)
        assert type(got[0]) is type(want[0]) and got[0] == want[0] == h
        assert got[1].dtype == want[1].dtype and np.array_equal(got[1], want[1]) and np.array_equal(got[1], sizes)
        assert got[2] == want[2]
        assert bs.parse_latent(bytearray(data))[0] == h and bs.parse_latent(memoryview(data))[0] == h
    for bad in (_pinned_embeddings()[-1], b"VBQe", b"", bytes(range(7, 107)), b"VBQx" + _pinned_segments()[-1][4:]):
        with pytest.raises(ValueError) as want:
            bs.parse(bad)
        with pytest.raises(ValueError) as got:
            bs.parse_latent(bad)
        assert str(got.value) == str(want.value)
