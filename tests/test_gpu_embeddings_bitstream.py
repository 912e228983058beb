"""Compressed word embeddings on the GPU: vbq_rans_segment_offsets_u16 / vbq_rans_decode_values_f32 against the C checker,
embeddings.compress_to_bytes / decompress / CompressedEmbeddings against compress_coordinates and the notebook fixtures, bit
for bit, and damaged input that raises instead of returning data."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import c_oracle as CO

pytestmark = pytest.mark.gpu
N = 10
T = 2 ** (N + 1) - 1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------- the C-ABI level
def _symbols(rng, kind, n):
    if kind == "skewed":
        return np.clip(np.rint(rng.normal(1023, 3.0, n)), 0, T - 1).astype(np.uint16)
    if kind == "uniform":
        return rng.integers(0, T, n).astype(np.uint16)
    if kind == "zeros":                                           # a sparse support: most table entries are 0
        support = np.sort(rng.choice(T, 100, replace=False))
        return support[rng.integers(0, 100, n) ** 2 // 100].astype(np.uint16)
    return np.full(n, int(rng.integers(0, T)), np.uint16)        # a single symbol (its neighbour gets frequency 1)


def _encode_checker(sym, seg):
    from vbq_amd.coder import exact_frequencies
    freq = exact_frequencies(np.bincount(sym, minlength=T))
    words, sizes = CO.rans_encode(sym[None], freq[None], seg)
    keep = np.arange(seg + 2)[None, None, :] < sizes[..., None].astype(np.int64)
    return freq, words[keep], sizes.reshape(-1).astype(np.uint16)


class _Stream:
    """One packed stream on the device, with its offsets from vbq_rans_segment_offsets_u16."""

    def __init__(self, payload, sizes, n, seg, freq, values):
        from vbq_amd import _lib, ops
        self.lib, self.ops = _lib.lib(), ops
        self.n, self.seg = n, seg
        self.nseg = (n + seg - 1) // seg
        self.payload = torch.from_numpy(np.ascontiguousarray(payload, np.uint16)).cuda()
        self.sizes = torch.from_numpy(np.ascontiguousarray(sizes, np.uint16)).cuda()
        self.freq = torch.from_numpy(np.ascontiguousarray(freq, np.uint16)).cuda()
        self.values = torch.from_numpy(np.ascontiguousarray(values, np.float32)).cuda()
        self.offsets = torch.empty(self.nseg, dtype=torch.int64, device="cuda")
        st = torch.zeros(1, dtype=torch.uint32, device="cuda")
        p = ops._ptr
        assert self.lib.vbq_rans_segment_offsets_u16(p(self.sizes), self.nseg, seg, self.payload.numel(), p(self.offsets),
                                                     p(st), ops._stream(self.sizes)) == 0
        self.offsets_status = int(st.cpu().item())

    def decode(self, segments=None):
        p = self.ops._ptr
        st = torch.zeros(1, dtype=torch.uint32, device="cuda")
        if segments is None:
            segs, out = None, torch.full((self.n,), np.nan, dtype=torch.float32, device="cuda")
        else:
            segs = torch.from_numpy(np.asarray(segments, np.int64)).cuda()
            out = torch.full((segs.numel() * self.seg,), np.nan, dtype=torch.float32, device="cuda")
        r = self.lib.vbq_rans_decode_values_f32(p(self.payload), self.payload.numel(), p(self.sizes), p(self.offsets), self.n,
                                                self.seg, N, p(self.freq), p(self.values), p(segs),
                                                0 if segs is None else segs.numel(), p(out), p(st), self.ops._stream(out))
        assert r == 0, self.lib.vbq_last_error()
        return out.cpu().numpy(), int(st.cpu().item())


CASES = [(seg, n) for seg in (1, 3, 8, 1000, 1024, 4096) for n in ({1: 1}.get(seg, seg // 2), 3 * seg, 3 * seg + 1)]


@pytest.mark.parametrize("kind", ["skewed", "uniform", "zeros", "single"])
@pytest.mark.parametrize("seg,n", CASES)
def test_decode_values_matches_the_checker(kind, seg, n):
    rng = np.random.default_rng(seg * 31 + n + len(kind))
    sym = _symbols(rng, kind, n)
    freq, payload, sizes = _encode_checker(sym, seg)
    values = rng.normal(size=T).astype(np.float32)
    values[::7] = -0.0                                            # the sign of zero survives
    s = _Stream(payload, sizes, n, seg, freq, values)
    assert s.offsets_status == 0
    assert np.array_equal(s.offsets.cpu().numpy(), np.concatenate([[0], np.cumsum(sizes.astype(np.int64))[:-1]]))
    want = values[sym]                                           # == checker decode + table lookup
    padded = np.zeros((1, s.nseg, seg + 2), np.uint16)
    offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    for j in range(s.nseg):
        padded[0, j, :sizes[j]] = payload[offs[j]:offs[j + 1]]
    assert np.array_equal(CO.rans_decode(padded, sizes[None].astype(np.uint32), freq[None], n, seg)[0], sym)

    full, st = s.decode()
    assert st == 0 and np.array_equal(_u32(full), _u32(want))

    sel = np.concatenate([rng.permutation(s.nseg), rng.integers(0, s.nseg, 5), [s.nseg - 1, 0]])
    got, st = s.decode(sel)
    assert st == 0
    for i, g in enumerate(sel):
        a, b = g * seg, min(n, (g + 1) * seg)
        assert np.array_equal(_u32(got[i * seg:i * seg + (b - a)]), _u32(want[a:b])), (i, g)
        if b - a < seg:                                           # the last segment writes only its valid length
            assert np.all(np.isnan(got[i * seg + (b - a):(i + 1) * seg]))


def test_decode_values_rejects_damage_at_the_abi_level():
    rng = np.random.default_rng(11)
    seg, n = 64, 64 * 20 + 5
    sym = _symbols(rng, "skewed", n)
    freq, payload, sizes = _encode_checker(sym, seg)
    values = np.arange(T, dtype=np.float32) + 1.0
    ok = _Stream(payload, sizes, n, seg, freq, values)
    # segment ids outside [0, nseg): bit 5 (32), zeros in their slots, the valid ones still decode
    got, st = ok.decode([3, -1, ok.nseg, 2 ** 40, 0])
    assert st == 32
    assert np.all(got[seg:4 * seg] == 0) and np.array_equal(_u32(got[:seg]), _u32(values[sym[3 * seg:4 * seg]]))
    assert np.array_equal(_u32(got[4 * seg:]), _u32(values[sym[:seg]]))
    # a size out of range: bit 0 from the offsets and the decoder, that segment decodes to zeros
    bad = sizes.copy()
    bad[4] = seg + 3
    s = _Stream(payload, bad, n, seg, freq, values)
    assert s.offsets_status & 1
    full, st = s.decode()
    assert st & 1 and np.all(full[4 * seg:5 * seg] == 0)
    # sizes that overrun the payload: bit 4 (16) from the offsets, bit 0 for the segments past the end
    over = sizes.copy()
    over[-3:] = seg + 2
    s = _Stream(payload, over, n, seg, freq, values)
    assert s.offsets_status & 16
    full, st = s.decode()
    assert st & 1 and np.all(full[-5:] == 0)
    # a flipped payload word: bit 1 or 2
    flip = payload.copy()
    flip[len(flip) // 2] ^= 0x1234
    s = _Stream(flip, sizes, n, seg, freq, values)
    assert s.offsets_status == 0
    assert s.decode()[1] & 6
    # an invalid table: bit 3, zeros
    f2 = freq.copy()
    f2[int(np.argmax(f2))] += 1
    s = _Stream(payload, sizes, n, seg, f2, values)
    full, st = s.decode()
    assert st & 8 and np.all(full == 0)


# ---------------------------------------------------------------------------------------------------------- the Python API
@pytest.mark.parametrize("fixture", ["g7_notebook.npz", "g13_notebook_chain.npz"])
def test_fixtures_round_trip(golden, fixture):
    from vbq_amd import bitstream as bs, embeddings, tables
    from vbq_amd.coder import exact_frequencies
    g = golden(fixture)
    cp = g["codepoints"]
    srt = tables.level_major_to_sorted(cp).astype(np.float32)
    for beta, opt in zip(g["betas"], g["optima"]):
        data = embeddings.compress_to_bytes(g["means"], g["stds"], beta, cp)
        q = embeddings.decompress(data)
        assert q.shape == g["means"].shape and q.dtype == np.float32
        assert np.array_equal(_u32(q), _u32(opt)), beta
        ref = np.asarray(embeddings.compress_coordinates(g["means"], g["stds"], beta, codepoints=cp))
        assert np.array_equal(_u32(q), _u32(ref)), beta
        # the payload and sizes are the C checker's encoding, byte for byte
        h, table, sizes, off = bs.parse_embeddings(data)
        assert h.beta == beta and h.segment == embeddings.default_segment(g["means"].shape[1])
        ranks = np.searchsorted(srt, opt.ravel())
        freq = exact_frequencies(np.bincount(ranks, minlength=T))
        words, s_ref = CO.rans_encode(ranks[None].astype(np.uint16), freq[None], h.segment)
        keep = np.arange(h.segment + 2)[None, None, :] < s_ref[..., None].astype(np.int64)
        assert np.array_equal(sizes, s_ref.reshape(-1))
        assert data[off:] == words[keep].tobytes()
        assert np.array_equal(table["rank"], np.flatnonzero(freq)) and np.array_equal(table["freq"], freq[freq > 0])
        ce = embeddings.CompressedEmbeddings(data)
        assert ce.shape == g["means"].shape and ce.beta == beta and ce.nbytes == len(data)
        assert ce.bits_per_coordinate == 8 * len(data) / g["means"].size


@pytest.mark.parametrize("segment", [None, 1000, 5])
def test_rows_equal_the_decoded_matrix(golden, segment):
    from vbq_amd import embeddings
    g = golden("g13_notebook_chain.npz")
    data = embeddings.compress_to_bytes(g["means"], g["stds"], 17.0, g["codepoints"], segment=segment)
    ce = embeddings.CompressedEmbeddings(data)
    full = embeddings.decompress(data)
    assert np.array_equal(_u32(ce.tensor().cpu().numpy()), _u32(full))
    V = full.shape[0]
    rng = np.random.default_rng(3)
    for ids in (rng.integers(0, V, 64), [0], [V - 1], [V - 1, 0, 5, 5, 5, V - 1], rng.permutation(V), np.arange(V)[::-1]):
        got = ce.rows(ids)
        assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (len(ids), full.shape[1])
        assert np.array_equal(_u32(got.cpu().numpy()), _u32(full[np.asarray(ids)]))
    assert tuple(ce.rows(torch.tensor([2, 1])).shape) == (2, full.shape[1])
    assert tuple(ce.rows([]).shape) == (0, full.shape[1])
    for bad in ([V], [-1], [0, V + 5]):
        with pytest.raises(IndexError):
            ce.rows(bad)


def test_three_dimensional_rows(golden):
    from vbq_amd import embeddings
    g = golden("g7_notebook.npz")
    means, stds = g["means"].reshape(250, 3, 4), g["stds"].reshape(250, 3, 4)
    data = embeddings.compress_to_bytes(means, stds, 1.0, g["codepoints"])
    ce = embeddings.CompressedEmbeddings(data)
    full = embeddings.decompress(data)
    assert full.shape == (250, 3, 4) and np.array_equal(_u32(full.reshape(250, 12)), _u32(g["optima"][2]))
    assert np.array_equal(_u32(ce.rows([249, 0, 7]).cpu().numpy()), _u32(full[[249, 0, 7]]))


def test_damaged_input_raises(golden):
    from vbq_amd import _lib, bitstream as bs, embeddings
    g = golden("g13_notebook_chain.npz")
    data = embeddings.compress_to_bytes(g["means"], g["stds"], 0.6, g["codepoints"])
    h, _, sizes, off = bs.parse_embeddings(data)
    # a flipped payload word: the load succeeds (sizes are fine), every decode raises
    b = bytearray(data)
    b[off + 2 * (h.n_words // 2)] ^= 0x5A
    ce = embeddings.CompressedEmbeddings(bytes(b))
    with pytest.raises(_lib.VBQError, match="rANS"):
        ce.tensor()
    with pytest.raises(_lib.VBQError):
        embeddings.decompress(bytes(b))
    seg_of_flip = int(np.searchsorted(np.cumsum(sizes.astype(np.int64)), h.n_words // 2, side="right"))
    with pytest.raises(_lib.VBQError):
        ce.rows([seg_of_flip * h.segment // h.row_length])
    # the host check rejects a size out of range before any upload
    with pytest.raises(ValueError, match="segment size"):
        embeddings.CompressedEmbeddings(data[:h.nbytes] + struct_u16(h.segment + 3) + data[h.nbytes + 2:])
    # damage on the device after loading: a size out of range, a segment that overruns the payload
    ce = embeddings.CompressedEmbeddings(data)
    ce._sizes.view(torch.int16)[1] = h.segment + 3
    with pytest.raises(_lib.VBQError, match="size out of range"):
        ce.rows([h.segment // h.row_length])
    ce = embeddings.CompressedEmbeddings(data)
    ce._offsets[-1] = h.n_words
    with pytest.raises(_lib.VBQError, match="size out of range"):
        ce.tensor()
    with pytest.raises(_lib.VBQError):
        ce.rows([h.shape[0] - 1])
    assert np.array_equal(_u32(ce.rows([0]).cpu().numpy()), _u32(g["optima"][1][:1]))   # the rest still decodes


def struct_u16(v):
    return int(v).to_bytes(2, "little")


def test_large_synthetic_matrix(golden):
    """100 000 x 100 at one beta: exact round trip, and the file stays within entropy + 48 bits per segment + the table
    and the header."""
    from vbq_amd import bitstream as bs, embeddings
    g = golden("g13_notebook_chain.npz")
    cp = g["codepoints"]
    rng = np.random.default_rng(7)
    V, D = 100_000, 100
    means = (rng.standard_t(5, size=(V, D)) * float(g["empirical_std"]) * 0.8).astype(np.float32)
    stds = rng.uniform(0.05, 0.6, size=(V, D)).astype(np.float32)
    beta = 17.0
    data = embeddings.compress_to_bytes(means, stds, beta, cp)
    q = embeddings.decompress(data)
    ref = np.asarray(embeddings.compress_coordinates(means, stds, beta, codepoints=cp))
    assert np.array_equal(_u32(q), _u32(ref))
    h, _, _, _ = bs.parse_embeddings(data)
    idx, _ = embeddings.compress_coordinates_sweep(means, stds, [beta], cp, want_values=False)
    ent = embeddings.entropy_from_indices(idx)[0]
    header_bits = 8 * (40 + 8 * len(h.shape))
    assert h.segment == 1000 and h.nseg == 10_000
    assert 8 * len(data) <= ent + 48 * h.nseg + 64 * h.K + header_bits, (8 * len(data), ent)
    ce = embeddings.CompressedEmbeddings(data)
    ids = rng.integers(0, V, 4096)
    assert np.array_equal(_u32(ce.rows(ids).cpu().numpy()), _u32(ref[ids]))
