"""The segment decoders' rules for untrusted input, status bit by status bit -- vbq_rans_decode_u16 and
vbq_rans_decode_values_f32 launched once per hand-damaged stream, their EXACT status word and output against the reference
decoder of tests/mapped_reference.py at a palette of one class -- and the layout edges every segment kernel shares (a single
short segment, no 8-symbol steps, 8-symbol steps only, a second workgroup with one live lane) against the C checker."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mapped_reference as MR  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402

pytestmark = pytest.mark.gpu
S, n, SEG = 2, 70, 32                                            # three segments per stream: 32, 32 and 6 symbols
NSEG = 3
G = 1                                                            # the damaged segment: segment 1 of stream 1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _u32(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_CASES = {}


def _case(N):
    """(idx [S, n], freq [S, T], words [S, NSEG, SEG + 2], sizes u32 [S, NSEG], values f32 [T]) of one bit depth, encoded by
    the reference once and shared read-only."""
    if N not in _CASES:
        from vbq_amd.coder import quantize_frequencies
        T = 2 ** (N + 1) - 1
        rng = np.random.default_rng(500 + N)
        idx = np.clip(np.rint(rng.normal(T // 2, T / 8.0, (S, n))), 0, T - 1).astype(np.uint16)
        freq = quantize_frequencies(np.stack([np.bincount(r, minlength=T) for r in idx]))
        words, sizes = MR.encode(idx, np.zeros(n, np.uint8), freq[None], SEG)
        assert 5 <= sizes[1, G] <= SEG + 1                       # words to remove, and room for one more
        values = (np.arange(T, dtype=np.float32) + 0.5) * np.float32(-1.25)     # values[0] != 0
        for a in (idx, freq, words, sizes, values):
            a.setflags(write=False)
        _CASES[N] = idx, freq, words, sizes, values
    return _CASES[N]


def _reference(words, sizes, freq):
    return MR.decode(words, sizes, np.zeros(n, np.uint8), freq[None], n, SEG)


def _decode(words, sizes, freq, N):
    """One launch of vbq_rans_decode_u16 -> (idx u16 [S, n], status)."""
    from vbq_amd import _lib, ops
    d = [torch.from_numpy(np.array(a)).cuda() for a in (words, sizes.astype(np.uint32), freq)]
    idx = torch.full((S, n), 0x7fff, dtype=torch.int16, device="cuda").view(torch.uint16)
    status = torch.zeros(1, dtype=torch.uint32, device="cuda")
    r = _lib.lib().vbq_rans_decode_u16(ops._ptr(d[0]), ops._ptr(d[1]), S, n, N, SEG, ops._ptr(d[2]), ops._ptr(idx),
                                       ops._ptr(status), ops._stream(idx))
    assert r == 0, _lib.lib().vbq_last_error()
    return _u16(idx), int(status.cpu().item())


def _damages(words, sizes):
    """name -> (words, sizes, the status bit) with segment G of stream 1 damaged."""
    k = int(sizes[1, G])
    out = {}
    for name, size in (("size 1", 1), ("size seg + 3", SEG + 3)):
        s2 = sizes.copy()
        s2[1, G] = size
        out[name] = words.copy(), s2, 1
    for name, drop in (("one word removed", 1), ("every renormalisation word removed", k - 2)):
        w2, s2 = words.copy(), sizes.copy()
        w2[1, G] = 0
        w2[1, G, : k - drop] = words[1, G, drop:k]
        s2[1, G] = k - drop
        out[name] = w2, s2, 2
    w2, s2 = words.copy(), sizes.copy()
    w2[1, G, 1: k + 1] = words[1, G, :k]
    w2[1, G, 0] = 0x1234
    s2[1, G] = k + 1
    out["one word prepended"] = w2, s2, 4
    return out


@pytest.mark.parametrize("N", [10, 4])
def test_segment_decoder_status_bits(N):
    idx, freq, words, sizes, _ = _case(N)
    got, st = _decode(words, sizes, freq, N)
    assert st == 0 and np.array_equal(got, idx)
    a, b = G * SEG, (G + 1) * SEG
    rest = np.ones((S, n), bool)
    rest[1, a:b] = False
    for name, (w2, s2, bit) in _damages(words, sizes).items():
        want, st_ref = _reference(w2, s2, freq)
        got, st = _decode(w2, s2, freq, N)
        assert st_ref == bit and st == bit, (name, st, st_ref)
        assert np.array_equal(got, want), name
        assert np.array_equal(got[rest], idx[rest]), name
        if bit == 1:
            assert not got[1, a:b].any()
        if bit == 2:                                             # the segment's head up to the starving symbol, then zeros
            m = int(np.flatnonzero(got[1, a:b] != idx[1, a:b])[0])
            assert 0 < m < SEG and not got[1, a + m: b].any()
        if bit == 4:
            assert np.array_equal(got, idx)
    f2 = freq.copy()                                             # a row that sums to 2^15 - 1: every segment of its stream
    f2[1, int(np.argmax(f2[1]))] -= 1
    want, st_ref = _reference(words, sizes, f2)
    got, st = _decode(words, sizes, f2, N)
    assert st_ref == 8 and st == 8 and np.array_equal(got, want)
    assert not got[1].any() and np.array_equal(got[0], idx[0])


class _Packed:
    """One stream's segments as a contiguous payload on the device (a size outside [2, seg + 2] contributes no word, as
    vbq_rans_segment_offsets_u16 counts it) and one launch of vbq_rans_decode_values_f32 over it."""

    def __init__(self, words, sizes, freq, values, N):
        from vbq_amd import _lib, ops
        self.lib, self.ops, self.N = _lib.lib(), ops, N
        keep = [words[g, : sizes[g]] for g in range(NSEG) if 2 <= sizes[g] <= SEG + 2]
        self.payload = torch.from_numpy(np.concatenate(keep).astype(np.uint16)).cuda()
        self.sizes = torch.from_numpy(sizes.astype(np.uint16)).cuda()
        self.freq = torch.from_numpy(np.array(freq)).cuda()
        self.values = torch.from_numpy(np.array(values)).cuda()
        self.offsets = torch.empty(NSEG, dtype=torch.int64, device="cuda")
        st = torch.zeros(1, dtype=torch.uint32, device="cuda")
        p = ops._ptr
        assert self.lib.vbq_rans_segment_offsets_u16(p(self.sizes), NSEG, SEG, self.payload.numel(), p(self.offsets), p(st),
                                                     ops._stream(self.sizes)) == 0

    def decode(self, segments=None):
        p = self.ops._ptr
        st = torch.zeros(1, dtype=torch.uint32, device="cuda")
        segs = None if segments is None else torch.from_numpy(np.asarray(segments, np.int64)).cuda()
        count = NSEG if segs is None else segs.numel()
        out = torch.full((n if segs is None else count * SEG,), np.nan, dtype=torch.float32, device="cuda")
        r = self.lib.vbq_rans_decode_values_f32(p(self.payload), self.payload.numel(), p(self.sizes), p(self.offsets), n, SEG,
                                                self.N, p(self.freq), p(self.values), p(segs), 0 if segs is None else count,
                                                p(out), p(st), self.ops._stream(out))
        assert r == 0, self.lib.vbq_last_error()
        return out.cpu().numpy(), int(st.cpu().item())


def _values_of(want_idx, values, zeroed=()):
    """The reference's indices through the rank -> value table; a segment the decoder rejects outright (bits 0, 3, 5) is 0.0,
    not the value of symbol 0."""
    want = values[want_idx].copy()
    for g in zeroed:
        want[g * SEG: (g + 1) * SEG] = 0.0
    return want


@pytest.mark.parametrize("N", [10, 4])
def test_value_decoder_status_bits(N):
    idx, freq, words, sizes, values = _case(N)
    s = 1                                                        # the stream the damages are in
    ok = _Packed(words[s], sizes[s], freq[s], values, N)
    got, st = ok.decode()
    assert st == 0 and np.array_equal(_bits(got), _bits(values[idx[s]]))
    a, b = G * SEG, (G + 1) * SEG
    for name, (w2, s2, bit) in _damages(words, sizes).items():
        want_idx, st_ref = _reference(w2, s2, freq)
        want = _values_of(want_idx[s], values, zeroed=[G] if bit == 1 else [])
        got, st = _Packed(w2[s], s2[s], freq[s], values, N).decode()
        assert st_ref == bit and st == bit, (name, st, st_ref)
        assert np.array_equal(_bits(got), _bits(want)), name
        if bit == 2:                                             # after the starving symbol: the value of symbol 0
            m = int(np.flatnonzero(want_idx[s, a:b] != idx[s, a:b])[0])
            assert 0 < m < SEG and np.all(got[a + m: b] == values[0])
    f2 = freq.copy()
    f2[s, int(np.argmax(f2[s]))] -= 1
    assert _reference(words, sizes, f2)[1] == 8
    got, st = _Packed(words[s], sizes[s], f2[s], values, N).decode()
    assert st == 8 and np.array_equal(_bits(got), _bits(np.zeros(n, np.float32)))

    n_words = ok.payload.numel()                                 # an offset whose words would end past the payload: bit 0
    for off in (n_words - int(sizes[s, G]) + 1, n_words + 5, -1):
        bad = _Packed(words[s], sizes[s], freq[s], values, N)
        bad.offsets[G] = off
        got, st = bad.decode()
        assert st == 1 and np.array_equal(_bits(got), _bits(_values_of(idx[s], values, zeroed=[G]))), off
    got, st = ok.decode([0, NSEG, 2])                            # a listed segment id of nseg: bit 5, zeros in its slot
    assert st == 32
    assert np.array_equal(_bits(got[:SEG]), _bits(values[idx[s, :SEG]]))
    assert np.array_equal(_bits(got[SEG: 2 * SEG]), _bits(np.zeros(SEG)))
    tail = n - 2 * SEG                                           # the short last segment writes only its length
    assert np.array_equal(_bits(got[2 * SEG: 2 * SEG + tail]), _bits(values[idx[s, 2 * SEG:]]))
    assert np.all(np.isnan(got[2 * SEG + tail:]))


# ---------------------------------------------------------------------------------------- layout edges, against the C checker
def _valid(words, sizes):
    return words[np.arange(words.shape[-1])[None, None, :] < sizes[..., None].astype(np.int64)]


@pytest.mark.parametrize("n_,seg", [(5, 32), (1003, 64), (1024, 64), (520, 8)])
def test_layout_edges_match_the_checker(n_, seg):
    """n = 5: one short segment; 1003 / 64: no 8-symbol steps and a short last segment; 1024 / 64: 8-symbol steps only; 520 / 8:
    65 segments, so the second workgroup along x holds a single live lane.  The plain coder and the mapped coder (a uniform map
    per class, which must give the plain coder's words, and a map that changes at every symbol) on the same three streams."""
    from vbq_amd.coder import MappedRansCodec, RansCodec
    N, P = 10, 2
    planes, freq = MR.make_planes(P, n_, N)                      # [P, 3, n], [P, 3, T]
    nseg = (n_ + seg - 1) // seg
    mapped = MappedRansCodec(freq.copy(), N=N, segment=seg)
    for p in range(P):
        w_ref, s_ref = CO.rans_encode(planes[p], freq[p], seg)
        assert np.array_equal(CO.rans_decode(w_ref, s_ref, freq[p], n_, seg), planes[p])
        codec = RansCodec(freq[p].copy(), N=N, segment=seg)
        d_idx = torch.from_numpy(planes[p].copy()).cuda()
        cls = np.full(n_, p, np.uint8)
        for words, sizes in (codec.encode(d_idx), mapped.encode(torch.from_numpy(planes.copy()).cuda(), cls)):
            assert words.shape == (MR.S, nseg, seg + 2)
            assert np.array_equal(_u32(sizes), s_ref) and np.array_equal(_valid(_u16(words), s_ref), _valid(w_ref, s_ref))
        assert np.array_equal(_u32(codec.sizes(d_idx)), s_ref) and np.array_equal(_u32(mapped.sizes(d_idx, cls)), s_ref)
        d_w, d_s = torch.from_numpy(w_ref).cuda(), torch.from_numpy(s_ref).cuda()
        assert np.array_equal(_u16(codec.decode(d_w, d_s, n_)), planes[p])
        assert np.array_equal(_u16(mapped.decode(d_w, d_s, cls, n_)), planes[p])
    cls = (np.arange(n_) % P).astype(np.uint8)
    idx = MR.select(planes, cls)
    w_ref, s_ref = MR.encode(idx, cls, freq, seg)
    words, sizes = mapped.encode(torch.from_numpy(planes.copy()).cuda(), cls)
    assert np.array_equal(_u32(sizes), s_ref) and np.array_equal(_valid(_u16(words), s_ref), _valid(w_ref, s_ref))
    assert np.array_equal(_u32(mapped.sizes(torch.from_numpy(idx.copy()).cuda(), cls)), s_ref)
    assert np.array_equal(_u16(mapped.decode(words, sizes, cls, n_)), idx)
