"""The compact latent file (magic b"VBQc") on the host: the NumPy coder of tests/interleaved_reference.py round-trips the
shapes of the GPU tests, write_compact / parse_compact are strict, the C-ABI checks its arguments without a device, and
the interleaved file of a 64 x 1536 tensor is shorter than the file in segments."""
import ctypes as C
import struct

import numpy as np
import pytest

import interleaved_reference as IR
from oracle import c_oracle as CO
from vbq_amd import bitstream as BS

DIG = bytes(range(16))


@pytest.mark.parametrize("N", [10, 3])
@pytest.mark.parametrize("S,n,part", IR.CASES)
def test_reference_round_trip(S, n, part, N):
    idx, freq, sizes, payload = IR.reference_case(S, n, part, N)
    total = S * n
    P = (total + part - 1) // part
    assert sizes.shape == (P,) and int(sizes.sum(dtype=np.int64)) == payload.size
    m = np.minimum(part, total - part * np.arange(P))
    assert np.all(sizes >= 128) and np.all(sizes <= m + 128)
    assert np.array_equal(IR.decode(sizes, payload, freq, n, part), idx)
    T = 2 ** (N + 1) - 1
    if n >= 3:
        assert idx.min() == 0 and idx.max() == T - 1
    if S >= 2:                                                   # the constant stream: one symbol holds most of its table
        assert len(np.unique(idx[1])) == 1 and freq[1, idx[1, 0]] == freq[1].max() > 2 * np.sort(freq[1])[-2]


def test_reference_rejects_damage():
    idx, freq, sizes, payload = IR.reference_case(3, 100, 1000, 10)
    with pytest.raises(ValueError):
        IR.decode(sizes, payload[:-1], freq, 100, 1000)
    p = payload.copy()
    p[0] ^= 1
    with pytest.raises(ValueError):
        IR.decode(sizes, p, freq, 100, 1000)


def _file(shape=(3, 100, 4), part=500, N=10, seed=3):
    """A valid compact file of random indices: (bytes, header, sizes, payload)."""
    Cn = shape[-1]
    B = int(np.prod(shape)) // Cn
    idx, freq = IR.make_case(Cn, B, N, seed)
    sizes, payload = IR.encode(idx, freq, part)
    h = BS.CompactHeader(N=N, C=Cn, shape=shape, lamb=0.25, part=part, digest=DIG, n_words=payload.size)
    return BS.write_compact(h, sizes, payload), h, sizes, payload


@pytest.mark.parametrize("shape,part", [((3, 100, 4), 500), ((3, 100, 4), 1200), ((7, 4), 5), ((2, 3, 5, 2), 1 << 24)])
def test_write_parse_round_trip_and_length(shape, part):
    data, h, sizes, payload = _file(shape, part)
    h2, s2, off = BS.parse_compact(data)
    assert h2 == h and s2.dtype == np.dtype("<u4") and np.array_equal(s2, sizes)
    assert off % 8 == 0                                          # the payload starts 8-byte aligned, whatever the parity of P
    assert off == h.nbytes + h.sizes_nbytes == 48 + 8 * len(shape) + 4 * (h.n_parts + (h.n_parts & 1))
    assert np.array_equal(np.frombuffer(data, "<u2", offset=off), payload)
    assert len(data) == BS.compact_nbytes(shape, shape[-1], part, payload.size)
    if h.n_parts & 1:
        assert data[off - 4: off] == bytes(4)


def test_cross_format_rejection():
    data, h, sizes, payload = _file()
    with pytest.raises(ValueError, match="not a VBQ bitstream"):
        BS.parse(data)
    old = BS.write(BS.Header(N=10, C=4, shape=(2, 4), lamb=1.0, segment=16, digest=DIG, n_words=8), [2] * 4, [0, 1] * 4)
    assert BS.parse(old)[0].segment == 16
    with pytest.raises(ValueError, match="VBQb"):
        BS.parse_compact(old)
    with pytest.raises(ValueError, match="not a compact VBQ bitstream"):
        BS.parse_compact(b"VBQe" + data[4:])


def _patched(data, offset, raw):
    d = bytearray(data)
    d[offset: offset + len(raw)] = raw
    return bytes(d)


def test_parse_compact_rejects_every_field():
    data, h, sizes, payload = _file((3, 100, 4), 500)            # P = 3 (odd): a padded size block
    P, hlen = h.n_parts, h.nbytes
    assert P == 3
    bad = [
        (_patched(data, 0, b"VBQx"), "magic"),
        (_patched(data, 4, b"\x02"), "version 2"),
        (_patched(data, 7, b"\x01"), "reserved"),
        (_patched(data, 5, b"\x0b"), "N = 11"),
        (_patched(data, 5, b"\x00"), "N = 0"),
        (_patched(data, 6, b"\x00"), "0 dimensions"),
        (_patched(data, 8, struct.pack("<I", 0)), "zero channels"),
        (_patched(data, 8, struct.pack("<I", 5)), "channel-last"),
        (_patched(data, 12, struct.pack("<I", 0)), r"part 0 outside \[1, 16777216\]"),
        (_patched(data, 12, struct.pack("<I", (1 << 24) + 1)), r"part 16777217 outside \[1, 16777216\]"),
        (_patched(data, 16, struct.pack("<d", float("nan"))), "non-finite lambda"),
        (_patched(data, 24, struct.pack("<Q", h.n_words + 1)), "truncated"),
        (_patched(data, 24, struct.pack("<Q", h.n_words - 1)), "trailing"),
        (_patched(data, 48, struct.pack("<Q", 0)), "empty latent shape"),
        (data + b"\x00\x00", "2 trailing bytes"),
        (_patched(data, hlen + 4, struct.pack("<I", 127)), r"part size 127 at position 1 outside \[128, 628\]"),
        (_patched(data, hlen + 4, struct.pack("<I", 629)), r"part size 629 at position 1 outside \[128, 628\]"),
        (_patched(data, hlen + 8, struct.pack("<I", 200 + 128 + 1)), r"part size 329 at position 2 outside \[128, 328\]"),
        (_patched(data, hlen + 4 * P, b"\x01\x00\x00\x00"), "padding"),
    ]
    a, b = int(sizes[0]), int(sizes[1])
    if a > 128 and b < 628:                                      # in range, one word moved: the sum no longer matches
        bad.append((_patched(data, hlen, struct.pack("<I", a - 1)), "add up to"))
    else:
        pytest.fail("the draw leaves no room to move a word between two parts")
    for d, msg in bad:
        with pytest.raises(ValueError, match=msg):
            BS.parse_compact(d)
    # truncation at every boundary: inside the fixed header, the shape, the sizes, the padding, the payload
    off = hlen + h.sizes_nbytes
    for cut in (0, 3, 47, 48, hlen - 1, hlen, hlen + 4 * P - 1, hlen + 4 * P, off - 1, off, off + 1, len(data) - 1):
        with pytest.raises(ValueError, match="truncated"):
            BS.parse_compact(data[:cut])
    assert BS.parse_compact(data)[0] == h


def test_write_compact_validates():
    data, h, sizes, payload = _file()
    import dataclasses
    for change, msg in ((dict(part=0), "part 0"), (dict(part=(1 << 24) + 1), "part"), (dict(N=11), "N = 11"),
                        (dict(n_words=h.n_words + 1), "add up to"), (dict(digest=b"x"), "digest"),
                        (dict(shape=(3, 100, 5)), "channel-last")):
        with pytest.raises(ValueError, match=msg):
            BS.write_compact(dataclasses.replace(h, **change), sizes, payload)
    with pytest.raises(ValueError, match="part sizes, the shape needs"):
        BS.write_compact(h, sizes[:-1], payload)
    with pytest.raises(ValueError, match="payload of"):
        BS.write_compact(h, sizes, payload[:-1])
    s = sizes.copy()
    s[0], s[1] = 127, s[1] + (s[0] - 127)
    with pytest.raises(ValueError, match="part size 127"):
        BS.write_compact(h, s, payload)
    with pytest.raises(ValueError, match="part 0"):
        BS.compact_nbytes((3, 100, 4), 4, 0, 10)


def test_entry_points_validate_without_a_device():
    from vbq_amd import _lib
    h = _lib.lib()
    one = C.c_void_p(8)                                          # a non-null pointer that is never followed
    for bad in (dict(n_streams=-1), dict(n=-1), dict(N=0), dict(N=11), dict(part=0), dict(part=(1 << 24) + 1)):
        a = dict(n_streams=2, n=10, N=10, part=64)
        a.update(bad)
        assert h.vbq_rans_il_sizes_u16(one, a["n_streams"], a["n"], a["N"], a["part"], one, one, None) == -1
        assert b"vbq_rans_il_sizes_u16: bad sizes" in h.vbq_last_error()
        assert h.vbq_rans_il_encode_u16(one, a["n_streams"], a["n"], a["N"], a["part"], one, one, one, one, 200, None) == -1
        assert b"vbq_rans_il_encode_u16: bad sizes" in h.vbq_last_error()
        assert h.vbq_rans_il_decode_u16(one, 200, one, one, a["n_streams"], a["n"], a["N"], a["part"], one, one, None, None) == -1
        assert b"vbq_rans_il_decode_u16: bad sizes" in h.vbq_last_error()
    assert h.vbq_rans_il_encode_u16(one, 2, 10, 10, 64, one, one, one, one, -1, None) == -1
    assert h.vbq_rans_il_decode_u16(one, -1, one, one, 2, 10, 10, 64, one, one, None, None) == -1
    assert h.vbq_rans_il_sizes_u16(one, 1 << 40, 1 << 40, 10, 64, one, one, None) == -1 and b"too many" in h.vbq_last_error()
    assert h.vbq_rans_il_sizes_u16(one, 1 << 30, 4, 10, 1, one, one, None) == -1 and b"parts are too many" in h.vbq_last_error()
    # null pointers
    assert h.vbq_rans_il_sizes_u16(None, 2, 10, 10, 64, one, one, None) == -1 and b"null pointer" in h.vbq_last_error()
    assert h.vbq_rans_il_sizes_u16(one, 2, 10, 10, 64, None, one, None) == -1
    assert h.vbq_rans_il_sizes_u16(one, 2, 10, 10, 64, one, None, None) == -1
    for k in range(5):
        p = [one] * 5
        p[k] = None
        assert h.vbq_rans_il_encode_u16(p[0], 2, 10, 10, 64, p[1], p[2], p[3], p[4], 200, None) == -1
        assert b"null pointer" in h.vbq_last_error()
    for k in range(5):
        p = [one] * 5
        p[k] = None
        assert h.vbq_rans_il_decode_u16(p[0], 200, p[1], p[2], 2, 10, 10, 64, p[3], p[4], None, None) == -1
        assert b"null" in h.vbq_last_error()
    # nothing to code: fine without any pointer
    assert h.vbq_rans_il_sizes_u16(None, 0, 10, 10, 64, None, None, None) == 0
    assert h.vbq_rans_il_encode_u16(None, 2, 0, 10, 64, None, None, None, None, 0, None) == 0
    assert h.vbq_rans_il_decode_u16(None, 0, None, None, 0, 0, 10, 64, None, None, None, None) == 0
    assert h.vbq_abi_version() == 5


def _streams(rng, S, n, spread, T):
    """The draw of tests/test_gpu_bitstream.py."""
    idx = np.empty((S, n), np.uint16)
    for s in range(S):
        v = np.rint(rng.normal(rng.integers(200, 1800), spread[s % len(spread)], n)).astype(np.int64)
        idx[s] = np.clip(v, 0, T - 1)
    return idx


def test_interleaved_file_is_shorter_than_the_file_in_segments():
    """C = 64 channels of B = 1536 latents, three of four channels near-dead: one part of C * B symbols against segments of
    1024.  The claim is a condition on file lengths, both computed on the host: the segment file from the C checker's words,
    the interleaved file from the NumPy coder."""
    from vbq_amd.coder import ideal_bits, quantize_frequencies
    Cn, B, T = 64, 1536, 2047
    idx = _streams(np.random.default_rng(64 * 7 + 1024), Cn, B, [0.05, 0.05, 0.05, 0.6], T)
    counts = np.stack([np.bincount(r, minlength=T) for r in idx])
    freq = quantize_frequencies(counts)
    shape = (B, Cn)
    _, s_seg = CO.rans_encode(idx, freq, 1024)
    seg_bytes = BS.latent_nbytes(shape, Cn, 1024, int(s_seg.sum(dtype=np.int64)))
    sizes, payload = IR.encode(idx, freq, Cn * B)
    il = BS.write_compact(BS.CompactHeader(N=10, C=Cn, shape=shape, lamb=1.0, part=Cn * B, digest=DIG, n_words=payload.size),
                          sizes, payload)
    assert np.array_equal(IR.decode(sizes, payload, freq, B, Cn * B), idx)
    entropy = ideal_bits(counts, freq) / 8
    print(f"cross-entropy {entropy:.0f} B, segments {seg_bytes} B (+{seg_bytes - entropy:.0f}), "
          f"interleaved {len(il)} B (+{len(il) - entropy:.0f})")
    assert len(il) < seg_bytes
