"""The wave-interleaved coder on the GPU (vbq_rans_il_*_u16, RansCodec.*_interleaved) against the NumPy coder of
tests/interleaved_reference.py -- sizes, payload bytes and decoded indices, identical -- its rejection of damaged input by
status bit, and the quantizer's layout="interleaved" files (magic b"VBQc") against compress_latents, bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import interleaved_reference as IR  # noqa: E402

pytestmark = pytest.mark.gpu
LAMBS = [2.0 ** -6, 2.0 ** -2, 2.0, 16.0]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("N", [10, 3])
@pytest.mark.parametrize("S,n,part", IR.CASES)
def test_kernels_match_the_numpy_coder(S, n, part, N):
    from vbq_amd.coder import RansCodec
    idx, freq, sizes_ref, payload_ref = IR.reference_case(S, n, part, N)
    codec = RansCodec(freq.copy(), N=N)
    d_idx = torch.from_numpy(idx.copy()).cuda()
    only_sizes = codec.sizes_interleaved(d_idx, part)
    assert only_sizes.dtype == torch.uint32 and only_sizes.is_cuda
    assert np.array_equal(only_sizes.view(torch.int32).cpu().numpy().view(np.uint32), sizes_ref)
    sizes, payload = codec.encode_interleaved(d_idx, part)
    assert sizes.dtype == np.uint32 and payload.dtype == np.uint16
    assert np.array_equal(sizes, sizes_ref)
    assert payload.tobytes() == payload_ref.tobytes()
    back = codec.decode_interleaved(torch.from_numpy(payload_ref.copy()).cuda(), torch.from_numpy(sizes_ref.copy()).cuda(), n, part)
    assert back.shape == (S, n) and np.array_equal(_u16(back), idx)


# ---- rejection: deterministic damage of one valid stream of 61 parts of (at most) 64 symbols ----
RS, RN, RPART, RNB = 5, 777, 64, 10


def _raw_decode(codec, payload, sizes, n=RN, part=RPART):
    """(status, indices [S, n]) of one decoder launch on host arrays, without the exception."""
    d_pay = torch.from_numpy(np.ascontiguousarray(payload, np.uint16)).cuda()
    d_sz = torch.from_numpy(np.ascontiguousarray(sizes, np.uint32)).cuda()
    out = torch.full((codec.freq_host.shape[0], n), 7, dtype=torch.int16, device="cuda").view(torch.uint16)
    status = torch.zeros(1, dtype=torch.uint32, device="cuda")
    codec._decode_interleaved(d_pay, d_sz, n, part, out, status)
    return int(status.cpu().item()), _u16(out)


def _expect(idx, zero_parts, part=RPART):
    want = idx.reshape(-1).copy()
    for p in zero_parts:
        want[p * part: (p + 1) * part] = 0
    return want.reshape(idx.shape)


def _check_rejected(codec, payload, sizes, idx, zero_parts, status_is):
    from vbq_amd._lib import VBQError
    st, got = _raw_decode(codec, payload, sizes)
    assert status_is(st), st
    assert np.array_equal(got, _expect(idx, zero_parts))         # zeros for the rejected parts, every other part decoded
    with pytest.raises(VBQError, match="rANS bitstream rejected"):
        codec.decode_interleaved(torch.from_numpy(np.ascontiguousarray(payload, np.uint16)).cuda(),
                                 torch.from_numpy(np.ascontiguousarray(sizes, np.uint32)).cuda(), RN, RPART)


@pytest.fixture(scope="module")
def stream():
    from vbq_amd.coder import RansCodec
    idx, freq, sizes, payload = IR.reference_case(RS, RN, RPART, RNB)
    offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    return RansCodec(freq.copy(), N=RNB), idx, freq, sizes, payload, offs


def test_rejects_a_part_size_of_127(stream):
    codec, idx, freq, sizes, payload, offs = stream
    k = 2
    s = sizes.copy()
    s[k] = 127
    cut = int(sizes[k]) - 127                                    # drop the part's last words: the sum still matches
    pay = np.concatenate([payload[: offs[k + 1] - cut], payload[offs[k + 1]:]])
    _check_rejected(codec, pay, s, idx, [k], lambda st: st == 1)


def test_rejects_a_part_size_of_m_plus_129(stream):
    codec, idx, freq, sizes, payload, offs = stream
    k = 3
    s = sizes.copy()
    s[k] = RPART + 129
    pay = np.concatenate([payload[: offs[k + 1]], np.zeros(RPART + 129 - int(sizes[k]), np.uint16), payload[offs[k + 1]:]])
    _check_rejected(codec, pay, s, idx, [k], lambda st: st == 1)
    # the same damage on the shorter last part: its own limit is m + 128 with m = 45
    P = sizes.size
    m = RS * RN - (P - 1) * RPART
    assert 0 < m < RPART
    s = sizes.copy()
    s[P - 1] = m + 129
    pay = np.concatenate([payload, np.zeros(m + 129 - int(sizes[P - 1]), np.uint16)])
    _check_rejected(codec, pay, s, idx, [P - 1], lambda st: st == 1)


def test_rejects_a_word_moved_between_two_parts(stream):
    codec, idx, freq, sizes, payload, offs = stream
    k = next(p for p in range(sizes.size - 2) if sizes[p] > 128 and sizes[p + 1] < RPART + 128)
    s = sizes.copy()
    s[k] -= 1                                                    # words owed at the end of part k ...
    s[k + 1] += 1                                                # ... and part k + 1 starts a word early: left over / wrong state
    _check_rejected(codec, payload, s, idx, [k, k + 1], lambda st: st & 6 and not st & ~6)


def test_rejects_a_payload_one_word_short(stream):
    codec, idx, freq, sizes, payload, offs = stream
    _check_rejected(codec, payload[:-1], sizes, idx, [sizes.size - 1], lambda st: st == 16)


def test_rejects_a_frequency_row_summing_to_one_less(stream):
    from vbq_amd.coder import RansCodec
    _, idx, freq, sizes, payload, offs = stream
    codec = RansCodec(freq.copy(), N=RNB)                        # (its own: the damaged table below is installed by hand)
    f = freq.copy()
    j = int(np.argmax(f[2]))
    f[2, j] -= 1
    assert int(f[2].sum()) == (1 << 15) - 1
    codec._freq_dev = torch.from_numpy(f).cuda()
    hit = [p for p in range(sizes.size) if p * RPART < 3 * RN and (p + 1) * RPART > 2 * RN]   # the parts that hold stream 2
    _check_rejected(codec, payload, sizes, idx, hit, lambda st: st == 8)


def test_the_process_runs_on(stream):
    """After every rejection above: the same codec still decodes the valid stream."""
    codec, idx, freq, sizes, payload, offs = stream
    st, got = _raw_decode(codec, payload, sizes)
    assert st == 0 and np.array_equal(got, idx)


# ---- the quantizer ----
C = 64
SHAPE = (1, 48, 32, C)


@pytest.fixture(scope="module")
def quant():
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    rng = np.random.default_rng(C)
    scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), C))
    q = ChannelwisePriorCDFQuantizer(C, 10)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), scale))
    m = (scale * rng.standard_normal(SHAPE)).astype(np.float32)
    lv = (2 * (-2 + 0.7 * rng.standard_normal(SHAPE))).astype(np.float32)
    q.build_entropy_models_from_latents(m.reshape(-1, C), lv.reshape(-1, C), LAMBS, add_n_smoothing=1, spread="logvar")
    ref = q.compress_latents(m, lv, LAMBS)
    zhat = {lamb: np.asarray(ref["Z_hat"][lamb]).copy() for lamb in LAMBS}
    files = {(lamb, part): q.compress_latents_to_bytes(m, lv, lamb, layout="interleaved", part=part)
             for lamb in LAMBS for part in (1 << 17, 1000)}
    return q, m, lv, zhat, files


@pytest.mark.parametrize("part", [1 << 17, 1000])
def test_round_trip_is_bit_identical_to_compress_latents(quant, part):
    from vbq_amd import bitstream
    q, m, lv, zhat, files = quant
    for lamb in LAMBS:
        data = files[lamb, part]
        assert data[:4] == b"VBQc"
        h, sizes, _ = bitstream.parse_compact(data)
        assert h.shape == SHAPE and h.lamb == lamb and h.part == part and h.C == C and h.N == 10
        assert sizes.size == (48 * 32 * C + part - 1) // part
        z = q.decompress_latents(data)
        assert z.shape == SHAPE and z.dtype == np.float32 and np.array_equal(z, zhat[lamb])
        zt = q.decompress_latents(data, return_np=False)
        assert isinstance(zt, torch.Tensor) and zt.is_cuda and np.array_equal(zt.cpu().numpy(), z)
    assert files[LAMBS[0], part] == q.compress_latents_to_bytes(m, lv, LAMBS[0], part=part, layout="interleaved")   # deterministic


@pytest.mark.parametrize("part", [1 << 17, 1000])
def test_coded_nbytes_is_the_file_length(quant, part):
    q, m, lv, zhat, files = quant
    nb = q.coded_nbytes(m, lv, layout="interleaved", part=part)
    assert list(nb) == LAMBS
    for lamb in LAMBS:
        assert nb[lamb] == len(files[lamb, part])
    assert q.coded_nbytes(m, lv, [LAMBS[2]], layout="interleaved", part=part) == {LAMBS[2]: len(files[LAMBS[2], part])}


def test_budget_returns_the_smallest_lambda_that_fits(quant):
    q, m, lv, zhat, files = quant
    part = 1 << 17
    length = {lamb: len(files[lamb, part]) for lamb in LAMBS}
    for budget in sorted(set(length.values())) + [max(length.values()) + 100, min(length.values()) + 1]:
        fits = [lamb for lamb in LAMBS if length[lamb] <= budget]
        assert q.compress_latents_to_budget(m, lv, budget, layout="interleaved") == files[min(fits), part]
    # a subset of the lambdas and another part size: the lengths of THAT part size decide
    sub = {lamb: len(files[lamb, 1000]) for lamb in LAMBS[1:3]}
    assert q.compress_latents_to_budget(m, lv, max(sub.values()), lambs=LAMBS[1:3], layout="interleaved", part=1000) \
        == files[LAMBS[1], 1000]
    with pytest.raises(ValueError, match="no lambda fits"):
        q.compress_latents_to_budget(m, lv, min(length.values()) - 1, layout="interleaved")


def test_interleaved_file_is_shorter_and_the_default_is_unchanged(quant):
    q, m, lv, zhat, files = quant
    for lamb in LAMBS:
        default = q.compress_latents_to_bytes(m, lv, lamb)
        assert default[:4] == b"VBQb"
        assert default == q.compress_latents_to_bytes(m, lv, lamb, layout="segments", part=12345)
        assert default == q.compress_latents_to_bytes(m, lv, lamb, segment=1024, layout="segments")
        assert len(files[lamb, 1 << 17]) < len(default)
        assert np.array_equal(q.decompress_latents(default), zhat[lamb])
    assert q.coded_nbytes(m, lv) == q.coded_nbytes(m, lv, layout="segments", part=77)
    assert q.compress_latents_to_budget(m, lv, 10 ** 9) == q.compress_latents_to_budget(m, lv, 10 ** 9, layout="segments")


class _FixedVAE:
    """encode: the fixture's latents whatever the input; decode: the first three channels."""

    def __init__(self, m, lv):
        self.m, self.lv = torch.from_numpy(m).cuda(), torch.from_numpy(lv).cuda()

    def encode(self, X):
        return self.m, self.lv

    def decode(self, Z):
        return torch.as_tensor(Z).cuda()[..., :3].contiguous()


def test_image_level_calls_forward_the_layout(quant):
    q, m, lv, zhat, files = quant
    vae = _FixedVAE(m, lv)
    lamb = LAMBS[1]
    data = q.compress_to_bytes(None, vae, lamb, layout="interleaved")
    assert data == files[lamb, 1 << 17]
    assert np.array_equal(q.decompress(data, vae, clip=False), zhat[lamb][..., :3])
    assert q.compress_to_budget(None, vae, len(data), layout="interleaved") == \
        q.compress_latents_to_budget(m, lv, len(data), layout="interleaved")
    assert q.compress_to_bytes(None, vae, lamb, layout="interleaved", part=1000) == files[lamb, 1000]


def test_errors_and_damaged_files(quant):
    from vbq_amd import _lib, bitstream
    q, m, lv, zhat, files = quant
    with pytest.raises(ValueError, match="layout"):
        q.compress_latents_to_bytes(m, lv, LAMBS[0], layout="waves")
    for part in (0, (1 << 24) + 1):
        with pytest.raises(ValueError, match="part"):
            q.compress_latents_to_bytes(m, lv, LAMBS[0], layout="interleaved", part=part)
        with pytest.raises(ValueError, match="part"):
            q.coded_nbytes(m, lv, layout="interleaved", part=part)
    with pytest.raises(KeyError):
        q.compress_latents_to_bytes(m, lv, 0.123, layout="interleaved")
    data = files[LAMBS[1], 1000]
    h, sizes, off = bitstream.parse_compact(data)
    flipped = bytearray(data)
    flipped[off + 2 * (h.n_words // 2) + 1] ^= 0x5a
    with pytest.raises(_lib.VBQError):
        q.decompress_latents(bytes(flipped))
    d = bytearray(data)
    d[h.nbytes + 4: h.nbytes + 8] = np.uint32(127).tobytes()
    with pytest.raises(ValueError, match="part size 127"):
        q.decompress_latents(bytes(d))
    with pytest.raises(ValueError, match="truncated"):
        q.decompress_latents(data[:-2])
    d = bytearray(data)
    d[32] ^= 1
    with pytest.raises(ValueError, match="different quantizer or entropy model"):
        q.decompress_latents(bytes(d))
    assert np.array_equal(q.decompress_latents(data), zhat[LAMBS[1]])
