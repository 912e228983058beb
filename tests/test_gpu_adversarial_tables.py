"""Every rANS coder kernel on frequency tables that do not fit the data (tests/adversarial_tables.py): spikes, runs of
frequency-1 symbols, the ramp of all small divisors and tables with zeros, coding data drawn without a look at them -- segments of
two words and segments close to seg + 2, parts in which nearly every lane takes a word at every step, encoder states close to
f 2^17 at f = 32766 and 32767.  Every comparison is bit for bit with a reference that shares no code with the kernels: the C
checker, tests/interleaved_reference.py, tests/mapped_reference.py; tests/test_adversarial_tables_host.py proves on those
references that the cases reach what is claimed.  Nothing here is damaged input: what is decoded was made by a reference or by the
encoder under test after it was compared with one.  Last, one quantizer whose entropy models were fitted on narrow latents, used
on latents spread over the whole grid."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import adversarial_tables as AT  # noqa: E402
import interleaved_reference as IR  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402

pytestmark = pytest.mark.gpu


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


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                  # (a copy: the shared arrays are read-only)


def _valid(words, sizes):
    return words[np.arange(words.shape[-1])[None, None, :] < sizes[..., None].astype(np.int64)]


# ------------------------------------------------------------------------------------------------------------ the segment coder
def _values_decode(words, sizes, freq, values, n, seg, N, segments=None):
    """One stream's valid words as a payload, vbq_rans_segment_offsets_u16 over its sizes, then one launch of
    vbq_rans_decode_values_f32 (every segment, or the listed ones) -> (out, [status of the offsets, status of the decode])."""
    from vbq_amd import _lib, ops
    lib, p = _lib.lib(), ops._ptr
    nseg = sizes.size
    payload = _dev(np.concatenate([words[g, : sizes[g]] for g in range(nseg)]).astype(np.uint16))
    d_sizes, d_freq, d_values = _dev(sizes.astype(np.uint16)), _dev(freq), _dev(values)
    offsets = torch.empty(nseg, dtype=torch.int64, device="cuda")
    st = torch.zeros(2, dtype=torch.uint32, device="cuda")
    r = lib.vbq_rans_segment_offsets_u16(p(d_sizes), nseg, seg, payload.numel(), p(offsets), p(st[0:1]), ops._stream(payload))
    assert r == 0, lib.vbq_last_error()
    segs = None if segments is None else _dev(np.asarray(segments, np.int64))
    count = nseg if segs is None else segs.numel()
    out = torch.full((n if segs is None else count * seg,), np.nan, dtype=torch.float32, device="cuda")
    r = lib.vbq_rans_decode_values_f32(p(payload), payload.numel(), p(d_sizes), p(offsets), n, seg, N, p(d_freq), p(d_values),
                                       p(segs), 0 if segs is None else count, p(out), p(st[1:2]), ops._stream(out))
    assert r == 0, lib.vbq_last_error()
    want_off = np.cumsum(sizes.astype(np.int64)) - sizes
    assert np.array_equal(offsets.cpu().numpy(), want_off)
    return out.cpu().numpy(), _u32(st).tolist()


def _check_segment_coder(idx, freq, n, seg, N, value_streams):
    """All five checks of the segment coder on streams idx [S, n] with rows freq [S, T] (zeros allowed)."""
    from vbq_amd.coder import RansCodec
    T = freq.shape[1]
    w_ref, s_ref = CO.rans_encode(idx, freq, seg)
    codec = RansCodec(np.array(freq), N=N, segment=seg, allow_zero=True)
    d_idx = _dev(idx)
    words, sizes = codec.encode(d_idx)                           # vbq_rans_encode_u16
    got_s, got_w = _u32(sizes), _u16(words)
    diff = np.argwhere(got_s != s_ref)
    assert diff.size == 0, ("first size that differs (stream, segment)", diff[0], got_s[tuple(diff[0])], s_ref[tuple(diff[0])])
    assert np.array_equal(_valid(got_w, s_ref), _valid(w_ref, s_ref))
    assert np.array_equal(_u32(codec.sizes(d_idx)), s_ref)        # vbq_rans_sizes_u16, entry by entry
    back = codec.decode(_dev(w_ref), _dev(s_ref), n)             # vbq_rans_decode_u16 on the checker's words: status 0
    assert np.array_equal(_u16(back), idx)
    blob = codec.pack(words, sizes)
    assert len(blob) * 8 == codec.compressed_bits(sizes) == 16 * int(s_ref.sum(dtype=np.int64))
    assert blob == _valid(w_ref, s_ref).tobytes()
    payload, total, _ = codec.pack_device(words, sizes)
    n_words = int(total.view(torch.int64).cpu().item())
    assert _u16(payload[:n_words]).tobytes() == blob
    back = codec.decode_packed(_dev(np.frombuffer(blob, np.uint16)), _dev(s_ref.astype(np.uint16)), n)
    assert np.array_equal(_u16(back), idx)
    values = ((np.arange(T, dtype=np.float32) + 0.5) * np.float32(-1.25))
    nseg = s_ref.shape[1]
    listed = [nseg - 1, 0, nseg // 2, 0]                         # any order, a repeat, the short last segment
    for s in value_streams:
        out, st = _values_decode(w_ref[s], s_ref[s], freq[s], values, n, seg, N)
        assert st == [0, 0], (s, st)
        assert np.array_equal(_bits(out), _bits(values[idx[s]])), s
        out, st = _values_decode(w_ref[s], s_ref[s], freq[s], values, n, seg, N, listed)
        assert st == [0, 0], (s, st)
        for i, g in enumerate(listed):
            a, b = g * seg, min(n, (g + 1) * seg)
            assert np.array_equal(_bits(out[i * seg: i * seg + b - a]), _bits(values[idx[s, a:b]])), (s, g)
            assert np.all(np.isnan(out[i * seg + b - a: (i + 1) * seg]))


@pytest.mark.parametrize("N", AT.BIT_DEPTHS)
@pytest.mark.parametrize("n,seg", AT.SEGMENT_SHAPES)
def test_segment_coder_matches_the_checker(n, seg, N):
    names, idx, freq = AT.streams(N, n, zero=True)
    assert len(AT.pick(names, "zero")) == 15
    _check_segment_coder(idx, freq, n, seg, N, range(len(names)))


def test_the_largest_segment_of_frequency_one_symbols():
    """65533 symbols of frequency 1 in one lane: 61439 words, close to the seg + 2 = 65535 of the buffer and of the file's u16
    size field; the second segment holds 5 symbols."""
    n, seg = AT.LARGEST_SEGMENT
    idx, freq = AT.rare_stream(10, n)
    _check_segment_coder(idx, freq, n, seg, 10, [0])


# -------------------------------------------------------------------------------------------------------- the interleaved coder
@pytest.mark.parametrize("N", AT.BIT_DEPTHS)
@pytest.mark.parametrize("n,part", AT.IL_SHAPES + [AT.IL_CROSSING])
def test_interleaved_coder_matches_the_numpy_coder(n, part, N):
    from vbq_amd.coder import RansCodec
    names, idx, freq = AT.streams(N, n)
    sizes_ref, payload_ref = IR.encode(idx, freq, part)
    codec = RansCodec(np.array(freq), N=N, segment=None)
    d_idx = _dev(idx)
    got = _u32(codec.sizes_interleaved(d_idx, part))
    diff = np.flatnonzero(got != sizes_ref)
    assert diff.size == 0, ("first part whose size differs", diff[0], got[diff[0]], sizes_ref[diff[0]])
    sizes, payload = codec.encode_interleaved(d_idx, part)
    assert np.array_equal(sizes, sizes_ref)
    diff = np.flatnonzero(payload != payload_ref)
    assert diff.size == 0, ("first word that differs", diff[0])
    back = codec.decode_interleaved(_dev(payload_ref), _dev(sizes_ref), n, part)          # status 0, or it raises
    assert back.shape == idx.shape and np.array_equal(_u16(back), idx)


# ------------------------------------------------------------------------------------------------------------- the mapped coder
@pytest.mark.parametrize("N", AT.BIT_DEPTHS)
@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("n", [1003, 1024])
def test_mapped_coder_matches_the_python_coder(n, P, N):
    from vbq_amd.coder import MappedRansCodec, RansCodec
    seg = AT.MAPPED_SEG
    for name in AT.MAPPED_MAPS:
        planes, freq, cls, idx, w_ref, s_ref = AT.mapped_case(P, n, N, name)
        mapped = MappedRansCodec(np.array(freq), N=N, segment=seg)
        d_planes = _dev(planes)
        words, sizes = mapped.encode(d_planes, cls)
        assert np.array_equal(_u32(sizes), s_ref), name
        assert np.array_equal(_valid(_u16(words), s_ref), _valid(w_ref, s_ref)), name
        assert np.array_equal(_u32(mapped.sizes(d_planes, cls)), s_ref), name
        assert np.array_equal(_u32(mapped.sizes(_dev(idx), cls)), s_ref), name
        assert np.array_equal(_u16(mapped.decode(_dev(w_ref), _dev(s_ref), cls, n)), idx), name
    # a uniform map: word for word vbq_rans_encode_u16 with that class's rows (and the checker)
    for p in range(P):
        w_ref, s_ref = CO.rans_encode(planes[p], freq[p], seg)
        uniform = np.full(n, p, np.uint8)
        plain = RansCodec(np.array(freq[p]), N=N, segment=seg).encode(_dev(planes[p]))
        for words, sizes in (mapped.encode(d_planes, uniform), plain):
            assert np.array_equal(_u32(sizes), s_ref), p
            assert np.array_equal(_valid(_u16(words), s_ref), _valid(w_ref, s_ref)), p
        assert np.array_equal(_u32(mapped.sizes(d_planes, uniform)), s_ref), p
        assert np.array_equal(_u16(mapped.decode(_dev(w_ref), _dev(s_ref), uniform, n)), planes[p]), p


# --------------------------------------------------------------------------------------------------------------- end to end
C, NB, SHAPE = 32, 10, (1, 16, 16, 32)
LAMBS = [2.0 ** -6, 2.0 ** -2, 1.0]
SEG, PART = 64, 1000
FIT_AT = 0.3141                                                  # where the validation latents sit, as a fraction of the grid


class _UniformGrid:
    """Code points evenly spaced over [-2 scale, 2 scale] in every channel: which level a solve ends on depends on the
    posterior's width and on lambda, not on where on the grid the mean lies."""

    def __init__(self, scale):
        self.scale = scale

    def inverse_cdf(self, xi):
        return 4.0 * self.scale * (xi - 0.5)


@pytest.fixture(scope="module")
def mismatched():
    """(quantizer, three latents, compress_latents of each at LAMBS).  The entropy models were built from narrow validation
    latents: means within a few hundredths of the channel's scale of one place on the grid, so the tables are near-spikes
    there; 40000 rows, so that add-one smoothing leaves a symbol that never occurred at frequency 1 of 2^15.  The latents that
    are coded have means spread evenly over the whole grid.  Both have posterior widths of a tenth of the scale, and the place
    of the fit is no short binary fraction (no coarse code point sits on it), so fit and use end on the same levels and the
    bit-length model fits: raw_num_bits is the level, at most 10 bits, plus a bit or two for saying which -- while all but the
    few symbols near the place of the fit are coded with frequency 1, at 15 bits.  Shared, never changed."""
    from vbq_amd import ChannelwisePriorCDFQuantizer
    rng = np.random.default_rng(2024)
    scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), C))
    q = ChannelwisePriorCDFQuantizer(C, NB)
    q.build_code_points(_UniformGrid(scale))

    def widths(shape):
        return (2 * (np.log(0.1 * scale) + 0.3 * rng.standard_normal(shape))).astype(np.float32)
    fit_m = (4.0 * scale * (FIT_AT - 0.5) + 0.04 * scale * rng.standard_normal((40000, C))).astype(np.float32)
    q.build_entropy_models_from_latents(fit_m, widths((40000, C)), LAMBS, add_n_smoothing=1, spread="logvar")
    lat = []
    for shape in (SHAPE, (2, 5, 7, C), (1, 16, 16, C)):
        lat.append(((scale * rng.uniform(-1.9, 1.9, shape)).astype(np.float32), widths(shape)))
    refs = []
    for m, lv in lat:
        ref = q.compress_latents(m, lv, LAMBS)
        refs.append({k: {l: np.array(ref[k][l]) for l in LAMBS} for k in ("Z_hat", "raw_num_bits")})
    return q, lat, refs


def _mismatch_is_real(data, raw_num_bits):
    """The issue's yardstick, for every file these tests make: longer than 1.5 times the latents' raw_num_bits / 8 of
    compress_latents.  A file whose tables fitted would be shorter than raw_num_bits / 8."""
    raw = float(np.asarray(raw_num_bits).astype(np.float64).sum()) / 8
    assert len(data) > 1.5 * raw, (len(data), raw)


def test_files_of_out_of_distribution_latents(mismatched):
    from vbq_amd import bitstream
    q, lat, refs = mismatched
    (m, lv), ref = lat[0], refs[0]
    for lamb in LAMBS:
        for layout in ("segments", "interleaved"):
            data = q.compress_latents_to_bytes(m, lv, lamb, segment=SEG, layout=layout, part=PART)
            assert np.array_equal(_bits(q.decompress_latents(data)), _bits(ref["Z_hat"][lamb])), (lamb, layout)
            assert len(data) == q.coded_nbytes(m, lv, [lamb], segment=SEG, layout=layout, part=PART)[lamb]
            _mismatch_is_real(data, ref["raw_num_bits"][lamb])
            if layout == "segments":
                assert bitstream.latent_nbytes(SHAPE, C, SEG, bitstream.parse(data)[0].n_words) == len(data)
    cls = (np.arange(16)[:, None] + np.arange(16)[None, :])[None] // 3 % 2
    for pair in ([LAMBS[0], LAMBS[2]], [LAMBS[1], LAMBS[0]]):
        data = q.compress_latents_to_bytes_mapped(m, lv, pair, cls, segment=SEG)
        want = np.where(cls[..., None] == 0, ref["Z_hat"][pair[0]], ref["Z_hat"][pair[1]])
        assert np.array_equal(_bits(q.decompress_latents(data)), _bits(want)), pair
        assert len(data) == q.coded_nbytes_mapped(m, lv, pair, cls, segment=SEG), pair
        _mismatch_is_real(data, np.where(cls[..., None] == 0, ref["raw_num_bits"][pair[0]], ref["raw_num_bits"][pair[1]]))


def test_batches_of_out_of_distribution_latents_equal_the_loop(mismatched):
    q, lat, refs = mismatched
    lambs = [LAMBS[1], LAMBS[0], LAMBS[2]]
    loop = [q.compress_latents_to_bytes(m, lv, lamb, segment=SEG) for (m, lv), lamb in zip(lat, lambs)]
    assert q.compress_latents_to_bytes_batch(lat, lambs, segment=SEG) == loop
    compact = [q.compress_latents_to_bytes(m, lv, lamb, layout="interleaved", part=PART) for (m, lv), lamb in zip(lat, lambs)]
    assert q.compress_latents_to_compact_batch(lat, lambs, part=PART) == compact
    for files in (loop, compact):
        for data, ref, lamb in zip(files, refs, lambs):
            _mismatch_is_real(data, ref["raw_num_bits"][lamb])
    one = [q.coded_nbytes(m, lv, LAMBS, segment=SEG) for m, lv in lat]
    got = q.coded_nbytes_batch(lat, LAMBS, segment=SEG)
    assert [list(g.items()) for g in got] == [list(w.items()) for w in one]


def test_budget_takes_the_smallest_lambda_that_fits(mismatched):
    from vbq_amd import bitstream
    q, lat, refs = mismatched
    m, lv = lat[0]
    nb = q.coded_nbytes(m, lv, LAMBS, segment=SEG)
    assert len(set(nb.values())) == len(LAMBS)
    for budget in sorted(nb.values()) + [min(nb.values()) + 1, max(nb.values()) - 1]:
        data = q.compress_latents_to_budget(m, lv, budget, LAMBS, segment=SEG)
        want = min(l for l in LAMBS if nb[l] <= budget)
        assert bitstream.parse(data)[0].lamb == want and len(data) == nb[want] <= budget
        assert data == q.compress_latents_to_bytes(m, lv, want, segment=SEG)
        _mismatch_is_real(data, refs[0]["raw_num_bits"][want])
    with pytest.raises(ValueError):
        q.compress_latents_to_budget(m, lv, min(nb.values()) - 1, LAMBS, segment=SEG)
