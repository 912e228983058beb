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
