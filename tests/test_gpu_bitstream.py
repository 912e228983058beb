"""Byte strings on the GPU: vbq_rans_pack_u16 / vbq_rans_unpack_u16 against the host packer and the C checker, and the
quantizer's compress_latents_to_bytes / decompress_latents / compress_to_bytes / decompress against compress_latents /
compress, bit for bit."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import c_oracle as CO

pytestmark = pytest.mark.gpu
N = 10
T = 2 ** (N + 1) - 1
LAMBS = [2.0 ** -6, 2.0 ** -2, 2.0, 16.0]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _streams(rng, S, n, spread):
    idx = np.empty((S, n), np.uint16)
    for s in range(S):
        v = np.rint(rng.normal(rng.integers(200, 1800), spread[s % len(spread)], n)).astype(np.int64)
        idx[s] = np.clip(v, 0, T - 1)
    return idx


@pytest.mark.parametrize("S,n,seg", [(5, 3000, 1024), (3, 36864, 1024), (2, 1000, 7), (64, 2048, 256), (1, 2_000_000, 16)])
def test_pack_unpack_match_host_pack_and_checker(S, n, seg):
    from vbq_amd.coder import RansCodec, quantize_frequencies
    rng = np.random.default_rng(S * 7 + seg)
    idx = _streams(rng, S, n, [0.2, 2.0, 25.0, 300.0])
    freq = quantize_frequencies(np.stack([np.bincount(r, minlength=T) for r in idx]))
    codec = RansCodec(freq, N=N, segment=seg)
    d_idx = torch.from_numpy(idx).cuda()
    words, sizes = codec.encode(d_idx)
    w_ref, s_ref = CO.rans_encode(idx, freq, seg)
    assert np.array_equal(sizes.cpu().numpy(), s_ref)
    keep = np.arange(seg + 2)[None, None, :] < s_ref[..., None].astype(np.int64)
    assert np.array_equal(words.cpu().numpy()[keep], w_ref[keep])

    payload, total, offsets = codec.pack_device(words, sizes)
    s64 = s_ref.astype(np.int64)
    assert int(total.cpu().numpy()[0]) == int(s64.sum())
    assert np.array_equal(offsets.cpu().numpy().reshape(-1), np.concatenate([[0], np.cumsum(s64.reshape(-1))[:-1]]))
    got = payload[: int(s64.sum())].cpu().numpy().tobytes()
    assert got == codec.pack(words, sizes)                                       # byte for byte the host packer
    assert got == w_ref[keep].tobytes()                                          # and the checker's words

    sizes16 = torch.from_numpy(s_ref.astype(np.uint16).reshape(-1)).cuda()
    w2, s2, status = codec.unpack_device(payload[: int(s64.sum())], sizes16, n)
    assert int(status.cpu().item()) == 0
    assert np.array_equal(s2.cpu().numpy(), s_ref)
    assert np.array_equal(w2.cpu().numpy()[keep], w_ref[keep])
    back = codec.decode(w2, s2, n)
    assert torch.equal(back.view(torch.int16), d_idx.view(torch.int16))
    assert torch.equal(codec.decode_packed(payload[: int(s64.sum())], sizes16, n).view(torch.int16), d_idx.view(torch.int16))
    sz_h, pay_h = codec.encode_packed(d_idx)                                     # encode + pack, two copies back
    assert np.array_equal(sz_h, s_ref) and pay_h.tobytes() == got


def test_unpack_rejects_sizes_that_overrun_the_payload():
    """One direct C-ABI call: sizes in range but adding up past n_words, and one out of range.  The kernel reads nothing past
    n_words (every segment that would is left zero-sized), sets the status bits and returns normally."""
    from vbq_amd import _lib
    seg, n, n_words = 16, 64, 10                                      # 4 segments of at most 18 words, 10 payload words
    payload = torch.arange(n_words, dtype=torch.int16, device="cuda").view(torch.uint16)
    sizes_in = torch.tensor([18, 18, 0, 18], dtype=torch.int16, device="cuda").view(torch.uint16)
    words = torch.zeros((4, seg + 2), dtype=torch.uint16, device="cuda")
    sizes = torch.full((4,), 7, dtype=torch.int32, device="cuda").view(torch.uint32)
    offsets = torch.empty(4, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.uint32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    r = _lib.lib().vbq_rans_unpack_u16(p(payload), n_words, p(sizes_in), 1, n, seg, p(words), p(sizes), p(offsets), p(status),
                                       None)
    torch.cuda.synchronize()
    assert r == 0
    assert int(status.cpu().item()) == 1 | 16
    assert sizes.view(torch.int32).cpu().tolist() == [0, 0, 0, 0]
    assert int(words.view(torch.int16).abs().sum().item()) == 0                # nothing placed
    # the same words with sizes that fit: placed, no status
    sizes_in = torch.tensor([4, 2, 2, 2], dtype=torch.int16, device="cuda").view(torch.uint16)
    status.zero_()
    r = _lib.lib().vbq_rans_unpack_u16(p(payload), n_words, p(sizes_in), 1, n, seg, p(words), p(sizes), p(offsets), p(status),
                                       None)
    torch.cuda.synchronize()
    assert r == 0 and int(status.cpu().item()) == 0
    assert sizes.view(torch.int32).cpu().tolist() == [4, 2, 2, 2] and offsets.cpu().tolist() == [0, 4, 6, 8]
    w = words.view(torch.int16).cpu().numpy()
    assert w[0, :4].tolist() == [0, 1, 2, 3] and w[1, :2].tolist() == [4, 5] and w[3, :2].tolist() == [8, 9]


def _gaussian_quantizer(C, seed):
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


@pytest.mark.parametrize("C", [32, 256])
def test_latents_round_trip_bit_identical_and_rate(C):
    from vbq_amd import bitstream
    q, scale, rng = _gaussian_quantizer(C, C)
    for shape in ((1, 32, 48, C), (2, 17, 23, C)):
        m, lv = _latents(rng, scale, shape)
        q.build_entropy_models_from_latents(m.reshape(-1, C), lv.reshape(-1, C), LAMBS, add_n_smoothing=1, spread="logvar")
        for seg in (64, 1024):
            for lamb in LAMBS:
                data = q.compress_latents_to_bytes(m, lv, lamb, segment=seg)
                ref = q.compress_latents(m, lv, [lamb])
                z = q.decompress_latents(data)
                assert z.shape == shape and z.dtype == np.float32
                assert np.array_equal(z, np.asarray(ref["Z_hat"][lamb]))
                zt = q.decompress_latents(data, return_np=False)
                assert isinstance(zt, torch.Tensor) and zt.is_cuda and np.array_equal(zt.cpu().numpy(), z)
                h, sizes, _ = bitstream.parse(data)
                assert h.shape == shape and h.lamb == lamb and h.segment == seg and h.C == C and h.N == N
                est = float(np.sum(np.asarray(ref["num_bits"][lamb], dtype=np.float64)))
                bits = 16 * h.n_words
                assert 0.98 * est <= bits <= 1.02 * est + 40 * sizes.size, (C, shape, seg, lamb, bits, est)


def test_repeated_code_points_round_trip():
    from scipy.stats import norm
    from vbq_amd import ChannelwisePriorCDFQuantizer

    class Coarse:
        def inverse_cdf(self, xi):
            return np.round(norm.ppf(xi) * np.array([24.0, 64.0])) / np.array([24.0, 64.0])
    q = ChannelwisePriorCDFQuantizer(2, N)
    q.build_code_points(Coarse())
    assert not q._strict
    rng = np.random.default_rng(21)
    shape = (1, 40, 50, 2)
    m = rng.normal(0, 1.1, shape).astype(np.float32)
    lv = (2 * rng.normal(-2, 0.7, shape)).astype(np.float32)
    lambs = [0.01, 0.3, 4.0]
    q.build_entropy_models_from_latents(m.reshape(-1, 2), lv.reshape(-1, 2), lambs, add_n_smoothing=1, spread="logvar")
    for lamb in lambs:
        for seg in (64, 1024):
            z = q.decompress_latents(q.compress_latents_to_bytes(m, lv, lamb, segment=seg))
            assert np.array_equal(z, np.asarray(q.compress_latents(m, lv, [lamb])["Z_hat"][lamb]))


def test_save_load_and_foreign_models(tmp_path):
    from vbq_amd import ChannelwisePriorCDFQuantizer
    C = 32
    q, scale, rng = _gaussian_quantizer(C, 5)
    m, lv = _latents(rng, scale, (1, 32, 48, C))
    q.build_entropy_models_from_latents(m.reshape(-1, C), lv.reshape(-1, C), LAMBS, add_n_smoothing=1, spread="logvar")
    data = {lamb: q.compress_latents_to_bytes(m, lv, lamb) for lamb in LAMBS}
    want = {lamb: q.decompress_latents(data[lamb]) for lamb in LAMBS}
    q.save(tmp_path / "q.npz")
    q2 = ChannelwisePriorCDFQuantizer.load(tmp_path / "q.npz")
    for lamb in LAMBS:
        assert np.array_equal(q2.decompress_latents(data[lamb]), want[lamb])
        assert q2.compress_latents_to_bytes(m, lv, lamb) == data[lamb]
    m3, lv3 = _latents(rng, scale * 2, (1, 32, 48, C))                 # same code points, models fitted on other data
    q.build_entropy_models_from_latents(m3.reshape(-1, C), lv3.reshape(-1, C), LAMBS, add_n_smoothing=1, spread="logvar")
    for lamb in LAMBS:
        with pytest.raises(ValueError, match="different quantizer or entropy model"):
            q.decompress_latents(data[lamb])
    assert np.array_equal(q.decompress_latents(q.compress_latents_to_bytes(m, lv, LAMBS[1])),
                          np.asarray(q.compress_latents(m, lv, [LAMBS[1]])["Z_hat"][LAMBS[1]]))


def test_damaged_files():
    from vbq_amd import _lib, bitstream
    C, seg = 32, 64
    q, scale, rng = _gaussian_quantizer(C, 7)
    m, lv = _latents(rng, scale, (1, 32, 48, C))
    q.build_entropy_models_from_latents(m.reshape(-1, C), lv.reshape(-1, C), LAMBS, add_n_smoothing=1, spread="logvar")
    data = q.compress_latents_to_bytes(m, lv, LAMBS[1], segment=seg)
    h, sizes, off = bitstream.parse(data)
    flipped = bytearray(data)
    flipped[off + 2 * (h.n_words // 2) + 1] ^= 0x5a
    with pytest.raises(_lib.VBQError):
        q.decompress_latents(bytes(flipped))
    for bad in (0, 1, seg + 3):
        d = bytearray(data)
        d[h.nbytes + 6: h.nbytes + 8] = np.uint16(bad).tobytes()
        with pytest.raises(ValueError, match="segment size"):
            q.decompress_latents(bytes(d))
    with pytest.raises(ValueError, match="truncated"):
        q.decompress_latents(data[:-2])
    assert np.array_equal(q.decompress_latents(data), np.asarray(q.compress_latents(m, lv, [LAMBS[1]])["Z_hat"][LAMBS[1]]))


class ToyVAE:
    """Deterministic torch VAE on the device: 16x average pool + a 1x1 map to C channels (means), a constant log-variance;
    a 1x1 map back to 3 channels + nearest 16x upsampling.  NHWC in and out, channel-last latents."""

    def __init__(self, C, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.enc = (torch.randn(3, C, generator=g) * 2.0).cuda()
        self.dec = (torch.randn(C, 3, generator=g) * 0.1).cuda()
        self.C = C

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
    C = 32
    vae = ToyVAE(C)
    X = torch.from_numpy(np.random.default_rng(11).random((2, 64, 96, 3)).astype(np.float32)).cuda()
    q = ChannelwisePriorCDFQuantizer(C, N)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), np.full(C, 1.0)))
    q.build_entropy_models(X, vae, LAMBS, add_n_smoothing=1)
    for lamb in LAMBS:
        data = q.compress_to_bytes(X, vae, lamb)
        got = q.decompress(data, vae)
        want = np.asarray(q.compress(X, vae, [lamb])["X_hat"][lamb])
        assert got.shape == tuple(X.shape) and np.array_equal(got, want)
        assert np.array_equal(q.decompress(data, vae, clip=False), np.asarray(q.compress(X, vae, [lamb], clip=False)["X_hat"][lamb]))


def test_errors():
    from vbq_amd import ChannelwisePriorCDFQuantizer, bitstream
    C = 32
    q, scale, rng = _gaussian_quantizer(C, 9)
    m, lv = _latents(rng, scale, (1, 8, 8, C))
    q.build_entropy_models_from_latents(m.reshape(-1, C), lv.reshape(-1, C), LAMBS, add_n_smoothing=1, spread="logvar")
    with pytest.raises(KeyError):
        q.compress_latents_to_bytes(m, lv, 0.123)
    data = bytearray(q.compress_latents_to_bytes(m, lv, LAMBS[0]))
    data[16:24] = np.float64(0.123).tobytes()
    with pytest.raises(KeyError):
        q.decompress_latents(bytes(data))
    with pytest.raises(ValueError):
        q.compress_latents_to_bytes(m[..., :-1], lv[..., :-1], LAMBS[0])
    q11 = ChannelwisePriorCDFQuantizer(C, 11)
    with pytest.raises(ValueError, match="at most 10"):
        q11.compress_latents_to_bytes(m, lv, LAMBS[0])
    with pytest.raises(ValueError, match="at most 10"):
        q11.decompress_latents(bytes(data))
    assert bitstream.parse(bytes(data))[0].lamb == 0.123
