"""The compressed-embedding byte format ("VBQe", vbq_amd.bitstream) and its frequency table on the host: the header writes
and parses back, every malformed file raises ValueError with a message of its own, coder.exact_frequencies keeps its
invariants, and the notebook fixtures coded with the C checker round-trip through the format bit for bit within
entropy + 48 bits per segment."""
import math
import struct

import numpy as np
import pytest

from vbq_amd import bitstream as bs
from vbq_amd import coder, tables

SEG = 24


def _table(rng, N=10, K=37):
    T = 2 ** (N + 1) - 1
    K = min(K, T - 1)
    ranks = np.sort(rng.choice(T, K, replace=False))
    counts = np.zeros(T, np.int64)
    counts[ranks] = rng.integers(1, 1000, K)
    freq = coder.exact_frequencies(counts)
    r = np.flatnonzero(freq)
    t = np.empty(r.size, bs.TABLE_DTYPE)
    t["rank"], t["freq"] = r, freq[r]
    t["value"] = np.sort(rng.normal(size=r.size).astype(np.float32))
    return t


def _valid(shape=(13, 7), seg=SEG, beta=17.0, seed=0, N=10):
    rng = np.random.default_rng(seed)
    t = _table(rng, N=N)
    nseg = (math.prod(shape) + seg - 1) // seg
    sizes = rng.integers(2, seg + 3, nseg).astype(np.uint32)
    payload = rng.integers(0, 65536, int(sizes.sum())).astype(np.uint16)
    h = bs.EmbeddingHeader(N=N, shape=tuple(shape), segment=seg, beta=beta, empirical_std=1.25, n_words=int(sizes.sum()),
                           K=t.size)
    return h, t, sizes, payload, bs.write_embeddings(h, t, sizes, payload)


def _patch(data, offset, fmt, value):
    b = bytearray(data)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


def test_header_round_trip():
    for shape, seg, N in (((13, 7), SEG, 10), ((100, 300), 900, 10), ((5,), 65533, 3), ((2, 3, 4, 5), 1, 1), ((1,), 7, 10)):
        h, t, sizes, payload, data = _valid(shape, seg, beta=2.0 ** -5.5, N=N)
        assert data[:4] == b"VBQe" and len(data) % 2 == 0 and h.nbytes % 8 == 0
        got, gt, gs, off = bs.parse_embeddings(data)
        assert got == h and got.n == math.prod(shape) and got.nseg == -(-got.n // seg)
        assert got.row_length == math.prod(shape[1:])
        assert gt.tobytes() == t.tobytes() and gt.dtype == bs.TABLE_DTYPE
        assert np.array_equal(gs, sizes) and gs.dtype == np.dtype("<u2")
        assert off == h.nbytes + 2 * h.nseg and len(data) == off + 2 * h.n_words
        assert np.array_equal(np.frombuffer(data, "<u2", offset=off), payload)
        assert bs.parse_embeddings(bytearray(data))[0] == h and bs.parse_embeddings(memoryview(data))[0] == h


def test_every_truncation_raises_value_error():
    data = _valid((5, 3), seg=4)[-1]
    for n in range(len(data)):
        with pytest.raises(ValueError):
            bs.parse_embeddings(data[:n])


def test_cross_magic_rejection():
    emb = _valid()[-1]
    with pytest.raises(ValueError, match="magic"):
        bs.parse(emb)
    h = bs.Header(N=10, C=2, shape=(3, 2), lamb=0.5, segment=4, digest=bytes(16), n_words=4)
    lat = bs.write(h, [2, 2], [1, 2, 3, 4])
    with pytest.raises(ValueError, match="latent bitstream"):
        bs.parse_embeddings(lat)
    assert bs.parse(lat)[0] == h                           # the latent format itself is untouched


def _table_patch(data, h, i, field, value):
    off = 40 + 8 * len(h.shape) + 8 * i + {"rank": 0, "freq": 2, "value": 4}[field]
    return _patch(data, off, {"rank": "<H", "freq": "<H", "value": "<f"}[field], value)


@pytest.mark.parametrize("case,match", [
    ("magic", "magic"), ("version", "version"), ("reserved", "reserved"), ("trailing", "trailing"), ("N0", "N = 0"),
    ("N11", "N = 11"), ("ndim0", "0 dimensions"), ("ndim_big", "65 dimensions"), ("zero_dim", "empty"),
    ("segment0", "segment 0"), ("segment_big", "segment 65534"), ("beta_nan", "beta"), ("beta_inf", "beta"),
    ("beta_neg", "beta"), ("K_small", "K = 1"), ("K_big", "K = 2048"), ("rank_order", "strictly increasing"),
    ("rank_repeat", "strictly increasing"), ("rank_T", "rank 2047"), ("rank_T_small_N", "rank 15"), ("freq0", "frequency 0"),
    ("freq_big", "above 32767"), ("freq_sum", "sum to"), ("value_nan", "non-finite"), ("value_inf", "non-finite"),
    ("value_order", "decrease"), ("size0", "segment size 0"), ("size1", "segment size 1"),
    ("size_big", f"segment size {SEG + 3}"), ("sum", "add up"), ("n_words", "add up|truncated|trailing"),
    ("nseg", "truncated|trailing"),
])
def test_malformed_files(case, match):
    h, t, sizes, payload, data = _valid()
    if case == "rank_T_small_N":
        h, t, sizes, payload, data = _valid(N=3)
    sz = h.nbytes                                          # first segment size
    last = h.K - 1
    d = {
        "magic": lambda: b"VBQx" + data[4:],
        "version": lambda: _patch(data, 4, "<B", 2),
        "reserved": lambda: _patch(data, 6, "<H", 1),
        "trailing": lambda: data + b"\0\0",
        "N0": lambda: _patch(data, 5, "<B", 0),
        "N11": lambda: _patch(data, 5, "<B", 11),
        "ndim0": lambda: _patch(data, 36, "<I", 0),
        "ndim_big": lambda: _patch(data, 36, "<I", 65),
        "zero_dim": lambda: _patch(data, 40, "<Q", 0),
        "segment0": lambda: _patch(data, 8, "<I", 0),
        "segment_big": lambda: _patch(data, 8, "<I", 65534),
        "beta_nan": lambda: _patch(data, 16, "<d", float("nan")),
        "beta_inf": lambda: _patch(data, 16, "<d", float("inf")),
        "beta_neg": lambda: _patch(data, 16, "<d", -1.0),
        "K_small": lambda: _patch(data, 12, "<I", 1),
        "K_big": lambda: _patch(data, 12, "<I", 2048),
        "rank_order": lambda: _table_patch(data, h, 1, "rank", int(t["rank"][0])),
        "rank_repeat": lambda: _table_patch(data, h, last, "rank", int(t["rank"][last - 1])),
        "rank_T": lambda: _table_patch(data, h, last, "rank", 2047),
        "rank_T_small_N": lambda: _table_patch(data, h, last, "rank", 15),
        "freq0": lambda: _table_patch(_table_patch(data, h, 0, "freq", 0), h, 1, "freq", int(t["freq"][1] + t["freq"][0])),
        "freq_big": lambda: _table_patch(data, h, 0, "freq", 32768),
        "freq_sum": lambda: _table_patch(data, h, 0, "freq", int(t["freq"][0]) + 1),
        "value_nan": lambda: _table_patch(data, h, 3, "value", float("nan")),
        "value_inf": lambda: _table_patch(data, h, last, "value", float("inf")),
        "value_order": lambda: _table_patch(data, h, 0, "value", float(t["value"][1]) + 1.0),
        "size0": lambda: _patch(data, sz + 2 * 2, "<H", 0),
        "size1": lambda: _patch(data, sz + 2 * 2, "<H", 1),
        "size_big": lambda: _patch(data, sz + 2 * 2, "<H", SEG + 3),
        "sum": lambda: _patch(_patch(data, sz, "<H", 2 if sizes[0] > 2 else 3), sz + 2, "<H", int(sizes[1])),
        "n_words": lambda: _patch(data, 24, "<Q", h.n_words - 1)[:-2],
        "nseg": lambda: _patch(data, 40, "<Q", 40),        # another row count: another number of segments
    }[case]()
    with pytest.raises(ValueError, match=match):
        bs.parse_embeddings(d)


def test_write_validates_as_parse_does():
    h, t, sizes, payload, _ = _valid()
    with pytest.raises(ValueError, match="segment sizes"):
        bs.write_embeddings(h, t, sizes[:-1], payload)
    with pytest.raises(ValueError, match="payload"):
        bs.write_embeddings(h, t, sizes, payload[:-1].copy())
    with pytest.raises(ValueError, match="table must be"):
        bs.write_embeddings(h, t[:-1], sizes, payload)
    t2 = t.copy()
    t2["value"][0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        bs.write_embeddings(h, t2, sizes, payload)
    for bad in ((0, 3), ()):
        with pytest.raises(ValueError):
            bs.write_embeddings(bs.EmbeddingHeader(N=10, shape=bad, segment=SEG, beta=1.0, empirical_std=1.0, n_words=0,
                                                   K=t.size), t, [], [])


# ---------------------------------------------------------------------------------------------- coder.exact_frequencies
def _check_exact(counts, f):
    c = np.asarray(counts)
    assert f.dtype == np.uint16 and f.shape == c.shape
    f = f.astype(np.int64)
    assert f.sum() == 2 ** 15 and f.max() <= 2 ** 15 - 1
    used = np.flatnonzero(c)
    assert np.all(f[used] >= 1)
    if used.size > 1:
        assert np.array_equal(f > 0, c > 0)                # zeros kept
    else:
        assert np.count_nonzero(f) == 2


def test_exact_frequencies_invariants():
    rng = np.random.default_rng(5)
    T = 2047
    cases = [rng.integers(0, 3, T) * rng.integers(0, 10 ** 6, T),          # sparse, wide range
             np.ones(T, np.int64),                                        # all 2047 symbols used
             rng.integers(1, 100, T),
             np.r_[10 ** 12, np.ones(T - 1, np.int64)],                   # floors of 1 overshoot: surplus taken back
             np.bincount(rng.integers(0, 5, 1000), minlength=T)]
    for c in cases:
        f = coder.exact_frequencies(c)
        _check_exact(c, f)
        assert np.array_equal(f, coder.exact_frequencies(c.copy()))       # deterministic
        assert np.array_equal(f, coder.exact_frequencies(c.astype(np.float64)))
    f = coder.exact_frequencies(np.ones(T, np.int64))
    assert f.min() == 16 and f.max() == 17                               # 32768 = 2047 * 16 + 16: largest remainders first


def test_exact_frequencies_single_symbol():
    T = 2047
    for s, nb in ((0, 1), (1023, 1024), (T - 1, T - 2)):
        c = np.zeros(T, np.int64)
        c[s] = 21000
        f = coder.exact_frequencies(c)
        _check_exact(c, f)
        assert f[s] == 2 ** 15 - 1 and f[nb] == 1
    f = coder.exact_frequencies(np.array([0, 0, 5]))
    assert list(f) == [0, 1, 32767]
    for bad in (np.zeros(T), np.array([1]), np.array([-1, 3])):
        with pytest.raises(ValueError):
            coder.exact_frequencies(bad)


def test_codec_accepts_zero_entries_only_when_asked():
    f = coder.exact_frequencies(np.r_[np.zeros(2040, np.int64), np.arange(1, 8)])
    with pytest.raises(ValueError):
        coder.RansCodec(f, N=10)
    coder.RansCodec(f, N=10, allow_zero=True)
    big = np.zeros(2047, np.uint16)
    big[3] = 2 ** 15 - 1 + 1
    with pytest.raises(ValueError):
        coder.RansCodec(big, N=10, allow_zero=True)


# ---------------------------------------------------------------------------- the notebook fixtures through the C checker
@pytest.mark.parametrize("fixture", ["g7_notebook.npz", "g13_notebook_chain.npz"])
def test_fixtures_round_trip_through_the_format(golden, fixture):
    from oracle import c_oracle
    from vbq_amd import embeddings
    g = golden(fixture)
    cp = g["codepoints"]
    srt = tables.level_major_to_sorted(cp).astype(np.float32)
    shape = g["means"].shape
    seg = embeddings.default_segment(shape[1])
    assert seg % shape[1] == 0
    for beta, opt, ent in zip(g["betas"], g["optima"], g["entropy"]):
        ranks = np.searchsorted(srt, opt.ravel())
        freq = coder.exact_frequencies(np.bincount(ranks, minlength=cp.size))
        words, sizes = c_oracle.rans_encode(ranks[None].astype(np.uint16), freq[None], seg)
        keep = np.arange(seg + 2)[None, None, :] < sizes[..., None]
        payload = words[keep]
        r = np.flatnonzero(freq)
        table = np.empty(r.size, bs.TABLE_DTYPE)
        table["rank"], table["freq"], table["value"] = r, freq[r], srt[r]
        h = bs.EmbeddingHeader(N=10, shape=shape, segment=seg, beta=float(beta), empirical_std=float(g["empirical_std"]),
                               n_words=int(payload.size), K=r.size)
        data = bs.write_embeddings(h, table, sizes, payload)
        got, t, sz, off = bs.parse_embeddings(data)
        assert got == h
        pw = np.frombuffer(data, "<u2", offset=off)
        nseg = got.nseg
        offs = np.concatenate([[0], np.cumsum(sz.astype(np.int64))])
        padded = np.zeros((1, nseg, seg + 2), np.uint16)
        for j in range(nseg):
            padded[0, j, :sz[j]] = pw[offs[j]:offs[j + 1]]
        dense = np.zeros(cp.size, np.uint16)
        dense[t["rank"]] = t["freq"]
        dec = c_oracle.rans_decode(padded, sz.astype(np.uint32)[None], dense[None], got.n, seg)[0]
        vals = np.zeros(cp.size, np.float32)
        vals[t["rank"]] = t["value"]
        assert np.array_equal(vals[dec].view(np.uint32), opt.ravel().view(np.uint32)), beta
        assert 16 * got.n_words <= ent + 48 * nseg, (beta, 16 * got.n_words, ent)


def test_new_entry_points_validate_before_touching_the_device():
    from vbq_amd import _lib, build
    build.build_hip()
    h = _lib.lib()
    o = h.vbq_rans_segment_offsets_u16
    assert o(None, -1, 4, 0, None, None, None) == -1 and b"bad sizes" in h.vbq_last_error()
    assert o(None, 3, 0, 0, None, None, None) == -1 and b"bad sizes" in h.vbq_last_error()
    assert o(None, 3, 65534, 0, None, None, None) == -1
    assert o(None, 3, 4, -1, None, None, None) == -1
    assert o(None, 3, 4, 6, None, None, None) == -1 and b"null pointer" in h.vbq_last_error()
    d = h.vbq_rans_decode_values_f32
    # (payload, n_words, sizes, offsets, n, seg, N, freq, values, segments, n_sel, out, status, stream)
    assert d(None, 0, None, None, 10, 0, 10, None, None, None, 0, None, None, None) == -1 and b"bad sizes" in h.vbq_last_error()
    assert d(None, 0, None, None, 10, 65534, 10, None, None, None, 0, None, None, None) == -1
    assert d(None, 0, None, None, -1, 4, 10, None, None, None, 0, None, None, None) == -1
    assert d(None, -1, None, None, 10, 4, 10, None, None, None, 0, None, None, None) == -1
    assert d(None, 0, None, None, 10, 4, 0, None, None, None, 0, None, None, None) == -1
    assert d(None, 0, None, None, 10, 4, 11, None, None, None, 0, None, None, None) == -1
    assert d(None, 0, None, None, 10, 4, 10, None, None, None, -1, None, None, None) == -1 and b"n_sel" in h.vbq_last_error()
    assert d(None, 0, None, None, 10, 4, 10, None, None, None, 0, None, None, None) == -1 and b"null pointer" in h.vbq_last_error()
    assert d(None, 0, None, None, 0, 4, 10, None, None, None, 0, None, None, None) == 0        # nothing to decode
