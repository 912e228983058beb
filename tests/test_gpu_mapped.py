"""The class-mapped coder on the GPU (vbq_rans_map_*_u16, coder.MappedRansCodec) against tests/mapped_reference.py -- sizes,
words and decoded indices, identical -- and against the segment coder for a map of one class; its rejection of damaged input by
status bit; and the quantizer's lambda-map files (magic b"VBQm") against compress_latents, bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mapped_reference as MR  # noqa: E402

pytestmark = pytest.mark.gpu
N = 10
LAMBS = [2.0 ** -6, 2.0 ** -2, 2.0, 16.0]
S, SEG = MR.S, MR.SEG


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _u32(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _valid(words, sizes):
    return words[np.arange(words.shape[-1])[None, None, :] < sizes[..., None].astype(np.int64)]


@pytest.mark.parametrize("N_", [10, 4])
@pytest.mark.parametrize("n", [1003, 1024])                      # 1003: no 8-symbol steps and a short last segment; 1024: 8-symbol steps
@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_kernels_match_the_reference_and_the_segment_coder(P, n, N_):
    from vbq_amd.coder import MappedRansCodec, RansCodec
    for name in MR.maps(P, n):
        planes, freq, cls, idx, w_ref, s_ref = MR.reference_case(P, n, N_, name)
        codec = MappedRansCodec(freq.copy(), N=N_, segment=SEG)
        d_planes, d_idx = torch.from_numpy(planes.copy()).cuda(), torch.from_numpy(idx.copy()).cuda()
        d_cls = torch.from_numpy(cls.copy()).cuda()
        words, sizes = codec.encode(d_planes, d_cls)
        assert words.shape == (S, (n + SEG - 1) // SEG, SEG + 2) and sizes.dtype == torch.uint32
        assert np.array_equal(_u32(sizes), s_ref), (P, n, N_, name)
        assert np.array_equal(_valid(_u16(words), s_ref), _valid(w_ref, s_ref)), (P, n, N_, name)
        assert np.array_equal(_u32(codec.sizes(d_planes, d_cls)), s_ref)
        assert np.array_equal(_u32(codec.sizes(d_idx, cls)), s_ref)                 # (classes as a host array)
        w1, s1 = codec.encode(d_idx, d_cls)                                        # the pre-selected [S, n] input
        assert torch.equal(s1.view(torch.int32), sizes.view(torch.int32))
        assert np.array_equal(_valid(_u16(w1), s_ref), _valid(_u16(words), s_ref))
        back = codec.decode(words, sizes, d_cls, n)
        assert back.shape == (S, n) and np.array_equal(_u16(back), idx)
        sz_h, pay_h = codec.encode_packed(d_planes, d_cls)
        assert np.array_equal(sz_h, s_ref) and pay_h.tobytes() == _valid(w_ref, s_ref).tobytes()
        got = codec.decode_packed(torch.from_numpy(pay_h.copy()).cuda(), torch.from_numpy(sz_h.astype(np.uint16).reshape(-1)).cuda(),
                                  cls, n)
        assert np.array_equal(_u16(got), idx)
        if name.startswith("uniform"):
            p = int(name[len("uniform"):])
            w0, s0 = RansCodec(freq[p].copy(), N=N_, segment=SEG).encode(d_planes[p])
            assert torch.equal(s0.view(torch.int32), sizes.view(torch.int32))
            assert np.array_equal(_valid(_u16(w0), s_ref), _valid(_u16(words), s_ref))


def test_codec_rejects_bad_calls_on_the_host():
    from vbq_amd.coder import MappedRansCodec
    planes, freq, cls, idx, _, _ = MR.reference_case(3, 1003, N, "checker")
    codec = MappedRansCodec(freq.copy(), N=N, segment=SEG)
    d_planes = torch.from_numpy(planes.copy()).cuda()
    bad = cls.copy()
    bad[500] = 3
    for c in (bad, torch.from_numpy(bad).cuda(), cls.astype(np.int64) - 1):
        with pytest.raises(ValueError, match="class outside"):
            codec.encode(d_planes, c)
    with pytest.raises(ValueError, match="1002 classes"):
        codec.sizes(d_planes, cls[:-1])
    with pytest.raises(ValueError, match="integers"):
        codec.encode(d_planes, cls.astype(np.float32))
    with pytest.raises(ValueError, match="idx must be"):
        codec.encode(d_planes[:2], cls)
    words, sizes = codec.encode(d_planes, cls)
    with pytest.raises(ValueError, match="expected words"):
        codec.decode(words[:, :-1], sizes, cls, 1003)
    # the refusals both codecs word alike, in full
    import re
    from vbq_amd.coder import RansCodec
    plain = RansCodec(freq[0].copy(), N=N, segment=SEG)
    shape = "expected words [3, 16, 66] and sizes [3, 16] for 1003 symbols per stream, got (3, 15, 66) and (3, 16)"
    for call in (lambda: codec.decode(words[:, :-1], sizes, cls, 1003), lambda: plain.decode(words[:, :-1], sizes, 1003)):
        with pytest.raises(ValueError, match="^" + re.escape(shape) + "$"):
            call()
    with pytest.raises(ValueError, match="^" + re.escape(shape.replace("(3, 16)", "(3, 15)")) + "$"):
        plain.decode(words[:, :-1], sizes[:, :-1], 1003)
    for call in (plain.encode, plain.sizes, plain.encode_packed):
        with pytest.raises(ValueError, match="^2 index streams but 3 frequency rows$"):
            call(d_planes[0, :2])
    no_seg = RansCodec(freq[0].copy(), N=N, segment=None)
    text = "^this codec was made without a segment: it serves the interleaved layout only$"
    for call in (lambda: no_seg.encode(d_planes[0]), lambda: no_seg.sizes(d_planes[0]), lambda: no_seg.encode_packed(d_planes[0]),
                 lambda: no_seg.decode(words, sizes, 1003)):
        with pytest.raises(ValueError, match=text):
            call()
    for call in (lambda: codec.sizes_interleaved(d_planes, 4096), lambda: codec.encode_interleaved(d_planes, 4096),
                 lambda: codec.decode_interleaved(words.reshape(-1), sizes.reshape(-1), 1003, 4096)):
        with pytest.raises(ValueError, match="^the class-mapped coder has no interleaved layout$"):
            call()


def _raw_decode(codec, words, sizes, cls, n):
    """One launch of the decoder without the host's VBQError: (idx u16 [S, n] as NumPy, the status word)."""
    idx = torch.full((S, n), 0x7fff, dtype=torch.int16, device="cuda").view(torch.uint16)
    status = torch.zeros(1, dtype=torch.uint32, device="cuda")
    codec._map_decode(words, sizes, torch.from_numpy(np.ascontiguousarray(cls)).cuda(), n, idx, status)
    return _u16(idx), int(status.cpu().item())


def test_damaged_input_sets_the_status_bits():
    """Each case damages one thing, runs the decoder once and compares its output and status with the reference decoder's.  The
    kernel compares a class with P before it selects a table, keeps every word read below the segment's size (itself checked
    against seg + 2) and every table walk below T."""
    from vbq_amd import _lib
    from vbq_amd.coder import MappedRansCodec
    P, n = 3, 1003
    T = 2 ** (N + 1) - 1
    planes, freq, cls, idx, w_ref, s_ref = MR.reference_case(P, n, N, "checker")
    codec = MappedRansCodec(freq.copy(), N=N, segment=SEG)
    words, sizes = torch.from_numpy(w_ref.copy()).cuda(), torch.from_numpy(s_ref.copy()).cuda()
    got, st = _raw_decode(codec, words, sizes, cls, n)
    assert st == 0 and np.array_equal(got, idx)

    c2 = cls.copy()                                              # a class byte set to P, in segment 3
    c2[3 * SEG + 10] = P
    want, st_ref = MR.decode(w_ref, s_ref, c2, freq, n, SEG)
    got, st = _raw_decode(codec, words, sizes, c2, n)
    assert st_ref == 64 and st == 64 and np.array_equal(got, want)
    assert not got[:, 3 * SEG: 4 * SEG].any() and np.array_equal(got[:, : 3 * SEG], idx[:, : 3 * SEG])
    with pytest.raises(_lib.VBQError, match="class outside the palette"):
        codec.decode(words, sizes, c2, n)
    c2[3 * SEG + 10] = 255
    assert _raw_decode(codec, words, sizes, c2, n)[1] == 64

    s2 = s_ref.copy()                                            # a truncated segment: fewer words than it needs
    g = int(np.argmax(s_ref[1]))
    assert s_ref[1, g] > 4
    s2[1, g] = 2
    want, st_ref = MR.decode(w_ref, s2, cls, freq, n, SEG)
    got, st = _raw_decode(codec, words, torch.from_numpy(s2).cuda(), cls, n)
    assert st_ref == 2 and st == 2
    keep = np.ones((S, n), bool)
    keep[1, g * SEG: (g + 1) * SEG] = False
    assert np.array_equal(got[keep], idx[keep]) and got.max() < T
    with pytest.raises(_lib.VBQError, match="ran out of words"):
        codec.decode(words, torch.from_numpy(s2).cuda(), cls, n)

    w2 = w_ref.copy()                                            # a flipped payload word
    w2[2, 5, 1] ^= 0x5a5a
    want, st_ref = MR.decode(w2, s_ref, cls, freq, n, SEG)
    got, st = _raw_decode(codec, torch.from_numpy(w2).cuda(), sizes, cls, n)
    assert st == st_ref and st in (0, 2, 4)
    assert (st & 4) or not np.array_equal(got[2, 5 * SEG: 6 * SEG], idx[2, 5 * SEG: 6 * SEG])
    assert got.max() < T
    if not st & 2:
        assert np.array_equal(got, want)

    for bad_size in (0, 1, SEG + 3, 0xffffffff):                 # a size out of range: bit 0, zeros
        s3 = s_ref.copy()
        s3[0, 2] = bad_size
        got, st = _raw_decode(codec, words, torch.from_numpy(s3).cuda(), cls, n)
        assert st == 1 and not got[0, 2 * SEG: 3 * SEG].any()

    f2 = freq.copy()                                             # one class's table of one stream does not sum to 2^15: bit 3
    f2[2, 1, 7] += 1
    other = MappedRansCodec(freq.copy(), N=N, segment=SEG)
    other._freq_dev = torch.from_numpy(f2.reshape(-1, T)).cuda()
    got, st = _raw_decode(other, words, sizes, cls, n)
    assert st == 8 and not got[1].any() and np.array_equal(got[[0, 2]], idx[[0, 2]])


# ---------------------------------------------------------------------------------------------------------------- quantizer
C = 3
SHAPE = (2, 5, 7, C)


def _quantizer(seed):
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), C))
    q = ChannelwisePriorCDFQuantizer(C, N)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), scale))
    return q, scale, rng


def _latents(rng, scale, shape):
    m = (scale * rng.standard_normal(shape)).astype(np.float32)
    lv = (2 * (-2 + 0.7 * rng.standard_normal(shape))).astype(np.float32)
    return m, lv


@pytest.fixture(scope="module")
def built():
    """(quantizer with models for LAMBS, latents, a random map over the four lambdas, compress_latents of all four)."""
    q, scale, rng = _quantizer(31)
    fit_m, fit_lv = _latents(rng, scale, (4000, C))
    q.build_entropy_models_from_latents(fit_m, fit_lv, LAMBS, add_n_smoothing=1, spread="logvar")
    m, lv = _latents(rng, scale, SHAPE)
    classes = rng.integers(0, 4, SHAPE[:-1])
    ref = q.compress_latents(m, lv, LAMBS)
    ref = {k: {l: np.array(ref[k][l]) for l in LAMBS} for k in ("Z_hat", "num_bits")}
    return q, scale, rng, m, lv, classes, ref


def test_mapped_file_round_trips_bit_for_bit(built):
    from vbq_amd import bitstream
    q, _, _, m, lv, classes, ref = built
    for lambs, cls in ((LAMBS, classes), (LAMBS[::-1], classes), (LAMBS[1:3], classes % 2), ([LAMBS[2]], classes * 0),
                       (LAMBS[:3], np.where(classes == 1, 2, classes % 3))):
        for seg in (16, 1024):
            data = q.compress_latents_to_bytes_mapped(m, lv, lambs, cls, segment=seg)
            mapped = q.compress_latents_mapped(m, lv, lambs, cls)
            z = q.decompress_latents(data)
            assert z.shape == SHAPE and z.dtype == np.float32
            assert np.array_equal(z, mapped["Z_hat"])
            for name in ("Z_hat", "num_bits"):
                want = np.stack([ref[name][l] for l in lambs])[cls, np.arange(SHAPE[0])[:, None, None],
                                                                np.arange(SHAPE[1])[None, :, None], np.arange(SHAPE[2])[None, None, :]]
                assert mapped[name].shape == SHAPE and np.array_equal(mapped[name], want), (name, lambs)
            assert q.coded_nbytes_mapped(m, lv, lambs, cls, segment=seg) == len(data)
            h, c2, sizes, off = bitstream.parse_mapped(data)
            assert h.lambs == tuple(lambs) and h.shape == SHAPE and h.segment == seg and np.array_equal(c2, cls.reshape(-1))
            assert bitstream.mapped_nbytes(SHAPE, C, seg, h.n_words, len(lambs)) == len(data)
    zt = q.decompress_latents(data, return_np=False)
    assert isinstance(zt, torch.Tensor) and zt.is_cuda and np.array_equal(zt.cpu().numpy(), z)
    dev = q.compress_latents_mapped(m, lv, lambs, torch.from_numpy(cls).cuda(), return_np=False)
    assert dev["Z_hat"].is_cuda and np.array_equal(dev["Z_hat"].cpu().numpy(), mapped["Z_hat"])
    assert np.array_equal(dev["num_bits"].cpu().numpy(), mapped["num_bits"])


def test_uniform_map_is_the_one_lambda_file_in_another_container(built):
    from vbq_amd import bitstream
    q, _, _, m, lv, classes, _ = built
    for seg in (16, 1024):
        for p, lamb in enumerate(LAMBS):
            one = q.compress_latents_to_bytes(m, lv, lamb, segment=seg)
            data = q.compress_latents_to_bytes_mapped(m, lv, LAMBS, np.full(SHAPE[:-1], p), segment=seg)
            h1, s1, off1 = bitstream.parse(one)
            h, _, s, off = bitstream.parse_mapped(data)
            assert np.array_equal(s, s1) and data[off:] == one[off1:] and h.n_words == h1.n_words
            assert h.digests[p] == h1.digest and h.lambs[p] == h1.lamb
            assert len(data) - len(one) == bitstream.mapped_nbytes(SHAPE, C, seg, h.n_words, 4) - bitstream.latent_nbytes(SHAPE, C, seg, h.n_words)
            assert np.array_equal(q.decompress_latents(data), q.decompress_latents(one))


def test_other_files_still_decode_and_foreign_models_are_refused(built):
    q, scale, rng, m, lv, classes, ref = built
    for layout in ("segments", "interleaved"):
        data = q.compress_latents_to_bytes(m, lv, LAMBS[1], layout=layout, segment=16, part=64)
        assert data[:4] == (b"VBQb" if layout == "segments" else b"VBQc")
        assert np.array_equal(q.decompress_latents(data), ref["Z_hat"][LAMBS[1]])
    data = q.compress_latents_to_bytes_mapped(m, lv, LAMBS, classes, segment=16)
    q2, scale2, rng2 = _quantizer(31)                            # the same code points and the same models ...
    fit_m, fit_lv = _latents(rng2, scale2, (4000, C))
    q2.build_entropy_models_from_latents(fit_m, fit_lv, LAMBS, add_n_smoothing=1, spread="logvar")
    assert np.array_equal(q2.decompress_latents(data), q.decompress_latents(data))
    counts = np.array(q2._code_counts[LAMBS[2]])                 # ... until the model of ONE palette lambda differs
    counts[1, 1000] += 50
    q2._code_counts[LAMBS[2]] = counts
    for slot in ("_coder_tables", "_coder_stacks", "_coder_maps"):
        q2._dev_cache.pop(slot, None)
    with pytest.raises(ValueError, match="different quantizer or entropy model"):
        q2.decompress_latents(data)
    q3, _, _ = _quantizer(31)                                    # every model fitted on other data
    fit_m, fit_lv = _latents(np.random.default_rng(77), scale * 2, (4000, C))
    q3.build_entropy_models_from_latents(fit_m, fit_lv, LAMBS, add_n_smoothing=1, spread="logvar")
    with pytest.raises(ValueError, match="different quantizer or entropy model"):
        q3.decompress_latents(data)


def test_damaged_files(built):
    from vbq_amd import _lib, bitstream
    q, _, _, m, lv, classes, _ = built
    cls = classes % 3
    data = q.compress_latents_to_bytes_mapped(m, lv, LAMBS[:3], cls, segment=16)
    h, _, _, off = bitstream.parse_mapped(data)
    d = bytearray(data)
    d[h.nbytes] |= 3                                             # class 3 with P = 3: stopped by the parser, before the device
    with pytest.raises(ValueError, match="not below P = 3"):
        q.decompress_latents(bytes(d))
    d = bytearray(data)
    d[h.nbytes] = (d[h.nbytes] & ~3) | ((d[h.nbytes] & 3) + 1) % 3   # another VALID class at position 0: the payload no longer fits it
    z = None
    try:
        z = q.decompress_latents(bytes(d))
    except _lib.VBQError:
        pass
    assert z is None or not np.array_equal(z, q.decompress_latents(data))
    flipped = bytearray(data)
    flipped[off + 2 * (h.n_words // 2) + 1] ^= 0x5a
    with pytest.raises(_lib.VBQError):
        q.decompress_latents(bytes(flipped))
    with pytest.raises(ValueError, match="truncated"):
        q.decompress_latents(data[:-2])
    d = bytearray(data)
    d[24:32] = np.float64(0.123).tobytes()
    with pytest.raises(KeyError):
        q.decompress_latents(bytes(d))


def test_errors(built):
    from vbq_amd import ChannelwisePriorCDFQuantizer
    q, _, _, m, lv, classes, _ = built
    calls = (q.compress_latents_mapped, q.compress_latents_to_bytes_mapped, q.coded_nbytes_mapped)
    for call in calls:
        with pytest.raises(ValueError, match="palette of 0"):
            call(m, lv, [], classes * 0)
        with pytest.raises(ValueError, match="palette of 5"):
            call(m, lv, LAMBS + [LAMBS[0]], classes)
        with pytest.raises(ValueError, match="repeated lambda"):
            call(m, lv, [LAMBS[0], LAMBS[1], LAMBS[0]], classes % 3)
        with pytest.raises(KeyError):
            call(m, lv, [LAMBS[0], 0.123], classes % 2)
        with pytest.raises(ValueError, match="classes of shape"):
            call(m, lv, LAMBS, classes[0])
        with pytest.raises(ValueError, match="classes of shape"):
            call(m, lv, LAMBS, np.broadcast_to(classes[..., None], SHAPE))
        with pytest.raises(ValueError, match="class outside"):
            call(m, lv, LAMBS[:3], classes)
        with pytest.raises(ValueError, match="class outside"):
            call(m, lv, LAMBS, classes - 1)
        with pytest.raises(ValueError, match="integers"):
            call(m, lv, LAMBS, classes.astype(np.float32))
    with pytest.raises(ValueError, match="segment 0"):
        q.compress_latents_to_bytes_mapped(m, lv, LAMBS, classes, segment=0)
    q11 = ChannelwisePriorCDFQuantizer(C, 11)
    with pytest.raises(ValueError, match="at most 10"):
        q11.compress_latents_to_bytes_mapped(m, lv, LAMBS, classes)


class ToyVAE:
    """Deterministic torch VAE on the device, as tests/test_gpu_bitstream.py uses: 16x average pool + a 1x1 map to C channels
    (means), a constant log-variance; a 1x1 map back to 3 channels + nearest 16x upsampling.  NHWC, channel-last latents."""

    def __init__(self, C, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.enc = (torch.randn(3, C, generator=g) * 2.0).cuda()
        self.dec = (torch.randn(C, 3, generator=g) * 0.1).cuda()

    def encode(self, X):
        X = torch.as_tensor(X).cuda().float()
        pooled = torch.nn.functional.avg_pool2d(X.permute(0, 3, 1, 2), 16).permute(0, 2, 3, 1)
        means = (pooled @ self.enc).contiguous()
        return means, torch.full_like(means, -3.0)

    def decode(self, Z):
        Z = torch.as_tensor(Z).cuda().contiguous()
        y = (Z @ self.dec + 0.5).permute(0, 3, 1, 2)
        return torch.nn.functional.interpolate(y, scale_factor=16, mode="nearest").permute(0, 2, 3, 1).contiguous()


def test_image_level_round_trip():
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    vae = ToyVAE(C)
    X = torch.from_numpy(np.random.default_rng(11).random((2, 64, 96, 3)).astype(np.float32)).cuda()
    q = ChannelwisePriorCDFQuantizer(C, N)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), np.full(C, 1.0)))
    q.build_entropy_models(X, vae, LAMBS, add_n_smoothing=1)
    classes = np.random.default_rng(12).integers(0, 4, (2, 4, 6))          # latent resolution
    data = q.compress_to_bytes_mapped(X, vae, LAMBS, classes, segment=16)
    means, logvars = vae.encode(X)
    assert data == q.compress_latents_to_bytes_mapped(means, logvars, LAMBS, classes, segment=16)
    Z = q.compress_latents_mapped(means, logvars, LAMBS, classes, return_np=False)["Z_hat"]
    for clip in (True, False):
        want = vae.decode(Z)
        want = (want.clamp(0, 1) if clip else want).cpu().numpy()
        got = q.decompress(data, vae, clip=clip)
        assert got.shape == tuple(X.shape) and np.array_equal(got, want)
