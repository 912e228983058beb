"""The lambda-map file (vbq_amd.bitstream, magic b"VBQm") and the class-mapped coder's reference on the host: the reference
round-trips and is pinned to the C checker, write_mapped / parse_mapped round-trip and reject every malformed field, and the
new entry points check their arguments without a device."""
import struct

import numpy as np
import pytest

import mapped_reference as MR
from oracle import c_oracle as CO
from vbq_amd import bitstream as bs


@pytest.mark.parametrize("N", [10, 4])
@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_reference_round_trips(P, N):
    n = 203
    for name in MR.maps(P, n):
        planes, freq, cls, idx, words, sizes = MR.reference_case(P, n, N, name)
        assert sizes.min() >= 2 and sizes.max() <= MR.SEG + 2
        assert np.array_equal(MR.sizes(idx, cls, freq, MR.SEG), sizes)
        back, status = MR.decode(words, sizes, cls, freq, n, MR.SEG)
        assert status == 0 and np.array_equal(back, idx), (P, N, name)


@pytest.mark.parametrize("N,n,seg", [(10, 1003, 64), (10, 1024, 64), (4, 500, 7), (10, 300, 1000)])
def test_reference_with_one_class_is_the_c_checker(N, n, seg):
    planes, freq = MR.make_planes(1, n, N)
    cls = np.zeros(n, np.uint8)
    words, sizes = MR.encode(planes[0], cls, freq, seg)
    w_ref, s_ref = CO.rans_encode(planes[0], freq[0], seg)
    assert np.array_equal(sizes, s_ref)
    keep = np.arange(seg + 2)[None, None, :] < s_ref[..., None].astype(np.int64)
    assert np.array_equal(words[keep], w_ref[keep])
    assert np.array_equal(CO.rans_decode(words, sizes, freq[0], n, seg), planes[0])
    # and class p of a larger palette, all symbols in it: the checker with that class's table
    planes, freq = MR.make_planes(3, n, N)
    words, sizes = MR.encode(planes[2], np.full(n, 2, np.uint8), freq, seg)
    w_ref, s_ref = CO.rans_encode(planes[2], freq[2], seg)
    keep = np.arange(seg + 2)[None, None, :] < s_ref[..., None].astype(np.int64)
    assert np.array_equal(sizes, s_ref) and np.array_equal(words[keep], w_ref[keep])


def test_reference_decoder_reports_damage():
    n, N, P = 203, 10, 3
    planes, freq, cls, idx, words, sizes = MR.reference_case(P, n, N, "checker")
    c2 = cls.copy()
    c2[70] = P                                                   # segment 1
    back, status = MR.decode(words, sizes, c2, freq, n, MR.SEG)
    assert status == 64 and not back[:, 64:128].any() and np.array_equal(back[:, :64], idx[:, :64])
    s2 = sizes.copy()
    s2[0, 0] = 1
    assert MR.decode(words, s2, cls, freq, n, MR.SEG)[1] == 1
    f2 = freq.copy()
    f2[1, 2, 5] += 1
    back, status = MR.decode(words, sizes, cls, f2, n, MR.SEG)
    assert status == 8 and not back[2].any() and np.array_equal(back[:2], idx[:2])


def test_class_block_packing():
    rng = np.random.default_rng(3)
    for B in (1, 3, 4, 5, 31, 32, 33, 210):
        cls = rng.integers(0, 4, B).astype(np.uint8)
        block = MR.pack_classes(cls)
        assert len(block) % 8 == 0 and len(block) == 8 * ((B + 31) // 32)
        assert bs.pack_classes(cls) == block
        assert np.array_equal(bs.unpack_classes(block, B), cls) and np.array_equal(MR.unpack_classes(block, B), cls)
    assert MR.pack_classes([1, 2, 3, 0, 3])[:2] == bytes([1 | 2 << 2 | 3 << 4, 3])


def _file(shape, P, segment=4, seed=0):
    rng = np.random.default_rng(seed)
    C = shape[-1]
    B = int(np.prod(shape)) // C
    nseg = (B + segment - 1) // segment
    cls = rng.integers(0, P, shape[:-1]).astype(np.int64)
    if B >= P:
        cls.reshape(-1)[:P] = np.arange(P)                       # every class occurs
    sizes = rng.integers(2, segment + 3, C * nseg)
    payload = rng.integers(0, 65536, int(sizes.sum())).astype(np.uint16)
    h = bs.MappedHeader(N=10, C=C, shape=tuple(shape), segment=segment, lambs=tuple(2.0 ** -(p + 1) for p in range(P)),
                        digests=tuple(bytes([p + 1] * 16) for p in range(P)), n_words=int(sizes.sum()))
    return h, cls, sizes, payload


@pytest.mark.parametrize("shape", [(3,), (7, 3), (5, 7, 3), (2, 5, 7, 3), (33, 1)])
@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_write_parse_round_trip_and_length(shape, P):
    h, cls, sizes, payload = _file(shape, P)
    data = bs.write_mapped(h, cls, sizes, payload)
    h2, c2, s2, off = bs.parse_mapped(data)
    assert h2 == h and h2.P == P
    assert c2.dtype == np.uint8 and np.array_equal(c2, cls.reshape(-1))
    assert s2.dtype == np.dtype("<u2") and np.array_equal(s2, sizes)
    assert data[off:] == payload.tobytes() and off % 8 == (2 * sizes.size) % 8
    assert bs.mapped_nbytes(shape, shape[-1], h.segment, h.n_words, P) == len(data)
    assert h2.sizes_offset % 8 == 0 and data[:4] == b"VBQm"
    B = int(np.prod(shape)) // shape[-1]
    assert data[h2.nbytes: h2.sizes_offset] == MR.pack_classes(cls.reshape(-1))
    assert h2.n_rows == B and h2.total_nbytes == len(data)


def test_parse_latent_and_the_other_parsers_reject_the_new_magic():
    h, cls, sizes, payload = _file((2, 5, 7, 3), 3)
    data = bs.write_mapped(h, cls, sizes, payload)
    for parser in (bs.parse_latent, bs.parse, bs.parse_compact, bs.parse_embeddings, bs.parse_records):
        with pytest.raises(ValueError, match="VBQm"):
            parser(data)
    one = bs.write(bs.Header(N=10, C=3, shape=(4, 3), lamb=1.0, digest=bytes(16), n_words=6, segment=4), [2, 2, 2], np.zeros(6, np.uint16))
    with pytest.raises(ValueError, match="at one lambda"):
        bs.parse_mapped(one)
    with pytest.raises(ValueError, match="not a VBQ lambda-map bitstream"):
        bs.parse_mapped(b"XXXX" + bytes(60))


def _patched(data, offset, raw):
    d = bytearray(data)
    d[offset: offset + len(raw)] = raw
    return bytes(d)


def test_every_malformed_field_is_a_value_error():
    shape, P = (2, 5, 7, 3), 3                                   # B = 70: 18 class bytes, padded to 24
    h, cls, sizes, payload = _file(shape, P)
    data = bs.write_mapped(h, cls, sizes, payload)
    hp = bs.parse_mapped(data)[0]
    lam0, dig0, shp0, cls0, siz0 = 24, 24 + 8 * P, 24 + 24 * P, hp.nbytes, hp.sizes_offset
    u8, u32, u64, f64 = (lambda v: bytes([v])), (lambda v: struct.pack("<I", v)), (lambda v: struct.pack("<Q", v)), \
        (lambda v: struct.pack("<d", v))
    cases = [
        (0, b"VBQx", "not a VBQ lambda-map"),
        (4, u8(2), "version 2"),
        (5, u8(0), "N = 0"), (5, u8(11), "N = 11"),
        (6, u8(0), "0 dimensions"),
        (7, u8(0), "P = 0"), (7, u8(5), "P = 5"),
        (8, u32(0), "zero channels"), (8, u32(4), "not channel-last"),
        (12, u32(0), "segment 0"), (12, u32(65534), "segment 65534"),
        (16, u64(h.n_words + 1), "truncated"), (16, u64(h.n_words - 1), "trailing"),
        (lam0 + 8, f64(float("nan")), "non-finite lambda"), (lam0 + 8, f64(float("inf")), "non-finite lambda"),
        (lam0 + 16, f64(h.lambs[0]), "repeated lambda"),
        (shp0, u64(0), "empty latent shape"), (shp0 + 24, u64(5), "not channel-last"),
        (shp0, u64(2 ** 62), "too large"),
        (cls0, u8(data[cls0] | 3), "class 3 at position 0 is not below P = 3"),
        (cls0 + 17, u8(data[cls0 + 17] | 3 << 2), "class 3 at position 69"),
        (cls0 + 17, u8(data[cls0 + 17] | 1 << 4), "padding bits"),          # position 70: the first that does not exist
        (cls0 + 23, u8(0x40), "padding bits"),
        (siz0, struct.pack("<H", 1), "segment size 1 at position 0"), (siz0 + 2, struct.pack("<H", 7), "segment size 7 at position 1"),
    ]
    for off, raw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            bs.parse_mapped(_patched(data, off, raw))
    # sizes in range that no longer add up
    s2 = sizes.copy()
    s2[0] = s2[0] + 1 if s2[0] < h.segment + 2 else s2[0] - 1
    with pytest.raises(ValueError, match="add up"):
        bs.parse_mapped(_patched(data, siz0, struct.pack("<H", int(s2[0]))))
    # a digest is opaque: any 16 bytes parse
    assert bs.parse_mapped(_patched(data, dig0, bytes(range(16))))[0].digests[0] == bytes(range(16))
    for cut in (0, 3, 23, 24, lam0 + 9, dig0 + 5, shp0 + 31, cls0 + 3, siz0 + 1, len(data) - 2, len(data) - 1):
        with pytest.raises(ValueError, match="truncated"):
            bs.parse_mapped(data[:cut])
    with pytest.raises(ValueError, match="trailing"):
        bs.parse_mapped(data + b"\0\0")
    assert bs.parse_mapped(bytearray(data))[0] == h and bs.parse_mapped(memoryview(data))[0] == h


def test_writer_validates_as_the_parser():
    h, cls, sizes, payload = _file((2, 5, 7, 3), 3)
    import dataclasses
    for change, msg in (({"lambs": h.lambs[:2]}, "digests for 2 lambdas"), ({"lambs": (), "digests": ()}, "P = 0"),
                        ({"lambs": (1.0, 2.0, 1.0)}, "repeated lambda"), ({"lambs": (1.0, 2.0, float("nan"))}, "non-finite"),
                        ({"digests": (bytes(16), bytes(16), bytes(15))}, "16 bytes"), ({"segment": 0}, "segment 0"),
                        ({"shape": (2, 5, 7, 4)}, "channel-last"), ({"n_words": h.n_words + 1}, "add up"),
                        ({"lambs": (1.0, 2.0, 3.0, 4.0, 5.0), "digests": (bytes(16),) * 5}, "P = 5")):
        with pytest.raises(ValueError, match=msg):
            bs.write_mapped(dataclasses.replace(h, **change), cls, sizes, payload)
    bad = cls.copy()
    bad.reshape(-1)[9] = 3
    with pytest.raises(ValueError, match="class 3 at position 9"):
        bs.write_mapped(h, bad, sizes, payload)
    bad.reshape(-1)[9] = -1
    with pytest.raises(ValueError, match="negative class"):
        bs.write_mapped(h, bad, sizes, payload)
    bad.reshape(-1)[9] = 259                                     # (no wrap-around to class 3)
    with pytest.raises(ValueError, match="not below P"):
        bs.write_mapped(h, bad, sizes, payload)
    with pytest.raises(ValueError, match="69 classes"):
        bs.write_mapped(h, cls.reshape(-1)[:-1], sizes, payload)
    with pytest.raises(ValueError, match="integers"):
        bs.write_mapped(h, cls.astype(np.float32), sizes, payload)
    with pytest.raises(ValueError, match="segment sizes"):
        bs.write_mapped(h, cls, sizes[:-1], payload)
    with pytest.raises(ValueError, match="payload of"):
        bs.write_mapped(h, cls, sizes, payload[:-1])
    for P in (0, 5):
        with pytest.raises(ValueError, match="classes outside"):
            bs.mapped_nbytes((2, 5, 7, 3), 3, 4, 10, P)
    with pytest.raises(ValueError, match="channel-last"):
        bs.mapped_nbytes((2, 5, 7, 3), 4, 4, 10, 2)


def test_mapped_file_of_one_class_is_the_latent_file_plus_a_closed_form():
    """The same sizes and payload in both containers: the lambda-map file is longer by 24 P - 24 bytes of header (8 + 16 per
    lambda against the one lambda and digest of 24 bytes) and the class block."""
    for shape, seg in (((2, 5, 7, 3), 4), ((1, 32, 48, 8), 64)):
        C = shape[-1]
        B = int(np.prod(shape)) // C
        for P in (1, 2, 4):
            for n_words in (2 * C * ((B + seg - 1) // seg), 12345):
                extra = bs.mapped_nbytes(shape, C, seg, n_words, P) - bs.latent_nbytes(shape, C, seg, n_words)
                assert extra == 24 * (P - 1) + 8 * ((B + 31) // 32)


def test_new_entry_points_check_arguments_without_a_device():
    import ctypes as C
    from vbq_amd import _lib
    h = _lib.lib()
    one = C.c_void_p(8)                                          # a non-null pointer that is never followed: every call fails before device work
    enc, siz, dec = h.vbq_rans_map_encode_u16, h.vbq_rans_map_sizes_u16, h.vbq_rans_map_decode_u16
    for P in (0, 5, -1):
        assert enc(one, 1, one, P, 3, 100, 10, 64, one, one, one, None) == -1 and b"n_classes" in h.vbq_last_error()
        assert siz(one, 1, one, P, 3, 100, 10, 64, one, one, None) == -1 and b"n_classes" in h.vbq_last_error()
        assert dec(one, one, one, P, 3, 100, 10, 64, one, one, None, None) == -1 and b"n_classes" in h.vbq_last_error()
    for planes, P in ((2, 3), (0, 2), (4, 3), (3, 1)):
        assert enc(one, planes, one, P, 3, 100, 10, 64, one, one, one, None) == -1 and b"n_planes" in h.vbq_last_error()
        assert siz(one, planes, one, P, 3, 100, 10, 64, one, one, None) == -1 and b"n_planes" in h.vbq_last_error()
    for S, n, N, seg in ((-1, 100, 10, 64), (3, -1, 10, 64), (3, 100, 0, 64), (3, 100, 11, 64), (3, 100, 10, 0), (3, 100, 10, 65534),
                         (65536, 100, 10, 64)):
        assert enc(one, 1, one, 2, S, n, N, seg, one, one, one, None) == -1 and b"bad sizes" in h.vbq_last_error()
        assert siz(one, 2, one, 2, S, n, N, seg, one, one, None) == -1 and b"bad sizes" in h.vbq_last_error()
        assert dec(one, one, one, 2, S, n, N, seg, one, one, None, None) == -1 and b"bad sizes" in h.vbq_last_error()
    for k in range(5):                                           # each pointer of the encoder in turn
        a = [one] * 5
        a[k] = None
        assert enc(a[0], 2, a[1], 2, 3, 100, 10, 64, a[2], a[3], a[4], None) == -1 and b"null pointer" in h.vbq_last_error()
    for k in range(4):
        a = [one] * 4
        a[k] = None
        assert siz(a[0], 2, a[1], 2, 3, 100, 10, 64, a[2], a[3], None) == -1 and b"null pointer" in h.vbq_last_error()
    for k in range(5):                                           # (d_status may be null)
        a = [one] * 5
        a[k] = None
        assert dec(a[0], a[1], a[2], 2, 3, 100, 10, 64, a[3], a[4], None, None) == -1 and b"null pointer" in h.vbq_last_error()
    # nothing to do: 0, whatever the pointers
    assert enc(None, 2, None, 2, 0, 100, 10, 64, None, None, None, None) == 0
    assert enc(None, 2, None, 2, 3, 0, 10, 64, None, None, None, None) == 0
    assert siz(None, 1, None, 4, 3, 0, 10, 64, None, None, None) == 0
    assert dec(None, None, None, 4, 0, 5, 10, 64, None, None, None, None) == 0


def test_mapped_codec_checks_shapes_on_the_host():
    from vbq_amd.coder import MappedRansCodec
    planes, freq = MR.make_planes(3, 100, 4)
    codec = MappedRansCodec(freq, N=4, segment=64)
    assert (codec.P, codec.S, codec.n_streams) == (3, 3, 3)
    with pytest.raises(ValueError, match=r"freq must be \[P, S, 31\]"):
        MappedRansCodec(freq[0], N=4)
    with pytest.raises(ValueError, match="freq must be"):
        MappedRansCodec(np.concatenate([freq, freq[:2]]), N=4)
    f2 = freq.copy()
    f2[2, 1, 0] += 1
    with pytest.raises(ValueError, match="sum to 2\\*\\*15"):
        MappedRansCodec(f2, N=4)
    with pytest.raises(ValueError, match="no interleaved layout"):
        codec._parts(10, 64)
