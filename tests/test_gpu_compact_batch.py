"""Batches of compact latent files on the GPU at quantizer level: compress_latents_to_compact_batch against the loop of
compress_latents_to_bytes(..., layout="interleaved"), byte for byte, and decompress_latents_compact_batch against
decompress_latents and compress_latents, bit for bit -- mixed lambdas, shapes and parts, repeated code points, damage and
refusals included."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import interleaved_reference as IR  # noqa: E402

pytestmark = pytest.mark.gpu
N, C_ = 10, 32
LAMBS = [2.0 ** -6, 2.0 ** -2, 2.0, 16.0]
SHAPES = [(1, 32, 48, C_), (1, 20, 30, C_), (2, 5, 7, C_), (3, C_), (1, 1, 1, C_)]
USE = [LAMBS[1], LAMBS[3], LAMBS[1], LAMBS[0], LAMBS[3]]         # mixed order, with repeats
PARTS = [64, 1000, 1 << 17]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


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


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def batch():
    """The quantizer, the five latents and, per part, the files of the one-file call: computed once, shared, never changed."""
    q, scale, rng = _gaussian_quantizer(C_, 11)
    lat = [_latents(rng, scale, s) for s in SHAPES]
    q.build_entropy_models_from_latents(lat[0][0].reshape(-1, C_), lat[0][1].reshape(-1, C_), LAMBS, add_n_smoothing=1,
                                        spread="logvar")
    assert q._strict
    loop = {part: [q.compress_latents_to_bytes(m, lv, lamb, layout="interleaved", part=part) for (m, lv), lamb in zip(lat, USE)]
            for part in PARTS}
    return q, lat, loop


@pytest.mark.parametrize("part", PARTS)
def test_the_writer_equals_the_loop_of_one_file_calls(batch, part):
    q, lat, loop = batch
    files = q.compress_latents_to_compact_batch(lat, USE, part=part)
    assert [bytes(f) for f in files] == loop[part]
    dev = [(torch.from_numpy(m).cuda(), torch.from_numpy(lv).cuda()) for m, lv in lat]
    assert q.compress_latents_to_compact_batch(dev, USE, part=part) == loop[part]
    # one lambda for all files
    one = q.compress_latents_to_compact_batch(lat[1:3], LAMBS[2], part=part)
    assert one == [q.compress_latents_to_bytes(m, lv, LAMBS[2], layout="interleaved", part=part) for m, lv in lat[1:3]]


def test_the_reader_equals_the_one_file_decode(batch):
    q, lat, loop = batch
    # files written with different parts, read in one call
    files = [loop[PARTS[f % 3]][f] for f in range(len(SHAPES))]
    want = [q.decompress_latents(d) for d in files]
    got = q.decompress_latents_compact_batch(files, stack=False)
    assert len(got) == len(files)
    base = got[0].untyped_storage().data_ptr()
    for g, w, shape in zip(got, want, SHAPES):
        assert isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == shape
        assert g.untyped_storage().data_ptr() == base              # views of one allocation
        assert np.array_equal(_bits(g), _bits(w))
    got = q.decompress_latents_compact_batch(files, stack=False, return_np=True)
    assert all(isinstance(g, np.ndarray) and np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))
    # round trip writer -> reader equals compress_latents
    for part in PARTS:
        back = q.decompress_latents_compact_batch(q.compress_latents_to_compact_batch(lat, USE, part=part), stack=False)
        for (m, lv), lamb, z in zip(lat, USE, back):
            assert np.array_equal(_bits(z), _bits(q.compress_latents(m, lv, [lamb])["Z_hat"][lamb]))


def test_stack(batch):
    q, lat, loop = batch
    same = [loop[64][0], q.compress_latents_to_bytes(*lat[0], LAMBS[2], layout="interleaved", part=1000)]
    got = q.decompress_latents_compact_batch(same)
    assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (2,) + SHAPES[0]
    assert np.array_equal(_bits(got), _bits(np.stack([q.decompress_latents(d) for d in same])))
    got = q.decompress_latents_compact_batch(same, return_np=True)
    assert isinstance(got, np.ndarray) and got.shape == (2,) + SHAPES[0]
    with pytest.raises(ValueError, match=r"file 1 has latent shape \(1, 20, 30, 32\)"):
        q.decompress_latents_compact_batch(loop[64][:2])
    assert tuple(q.decompress_latents_compact_batch([]).shape) == (0,) and q.decompress_latents_compact_batch([], stack=False) == []


def test_repeated_code_points():
    """The non-strict path: the writer's kernels map a rank to the canonical rank of its run of equal code points."""
    from scipy.stats import norm
    from vbq_amd import ChannelwisePriorCDFQuantizer

    class Coarse:
        def inverse_cdf(self, xi):
            return np.round(norm.ppf(xi) * np.array([24.0, 64.0])) / np.array([24.0, 64.0])
    q = ChannelwisePriorCDFQuantizer(2, N)
    q.build_code_points(Coarse())
    assert not q._strict
    rng = np.random.default_rng(21)
    shapes = [(1, 40, 50, 2), (7, 9, 2), (1, 2)]
    lat = [(rng.normal(0, 1.1, s).astype(np.float32), (2 * rng.normal(-2, 0.7, s)).astype(np.float32)) for s in shapes]
    lambs = [0.01, 0.3, 4.0]
    q.build_entropy_models_from_latents(lat[0][0].reshape(-1, 2), lat[0][1].reshape(-1, 2), lambs, add_n_smoothing=1, spread="logvar")
    use = [lambs[2], lambs[0], lambs[2]]
    for part in (64, 1000):
        loop = [q.compress_latents_to_bytes(m, lv, lamb, layout="interleaved", part=part) for (m, lv), lamb in zip(lat, use)]
        assert q.compress_latents_to_compact_batch(lat, use, part=part) == loop
        back = q.decompress_latents_compact_batch(loop, stack=False)
        for (m, lv), lamb, z in zip(lat, use, back):
            assert np.array_equal(_bits(z), _bits(q.compress_latents(m, lv, [lamb])["Z_hat"][lamb]))


def test_a_flipped_payload_word_names_its_file(batch):
    from vbq_amd import _lib, bitstream
    q, lat, loop = batch
    files = list(loop[1000][:3])
    h, sizes, start = bitstream.parse_compact(files[1])
    flipped = bytearray(files[1])
    flipped[start + 2 * (int(sizes[0]) + 3) + 1] ^= 0x01          # the high byte of a state word of part 1
    flipped = bytes(flipped)
    # the premise, by the NumPy coder: the damaged file is one a decoder must reject
    freq = q._coder_tables(q._lambda_key(h.lamb))[0].freq_host.numpy()
    pay = np.frombuffer(flipped, dtype="<u2", count=h.n_words, offset=start)
    with pytest.raises(ValueError):
        IR.decode(sizes, pay, freq, h.n_rows, h.part)
    with pytest.raises(_lib.VBQError, match="file 1: rANS bitstream rejected"):
        q.decompress_latents_compact_batch([files[0], flipped, files[2]], stack=False)
    # the process runs on
    got = q.decompress_latents_compact_batch(files, stack=False)
    assert np.array_equal(_bits(got[1]), _bits(q.decompress_latents(files[1])))


def test_refusals_before_any_launch(batch, monkeypatch):
    from vbq_amd import ops
    q, lat, loop = batch
    files = loop[1000]
    other, scale, rng = _gaussian_quantizer(C_, 12)
    m, lv = _latents(rng, scale, SHAPES[1])
    other.build_entropy_models_from_latents(m.reshape(-1, C_), lv.reshape(-1, C_), LAMBS, add_n_smoothing=1, spread="logvar")
    foreign = other.compress_latents_to_bytes(m, lv, LAMBS[1], layout="interleaved")
    segments = q.compress_latents_to_bytes(*lat[1], LAMBS[1])
    unknown = bytearray(files[0])
    unknown[16:24] = np.float64(3.0).tobytes()                    # a lambda without a model
    for name in ("rans_il_sizes_files", "rans_il_encode_files", "rans_il_decode_files", "gather"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("a kernel was launched"))
    with pytest.raises(ValueError, match="file 1 was compressed with a different quantizer"):
        q.decompress_latents_compact_batch([files[0], foreign], stack=False)
    with pytest.raises(KeyError):
        q.decompress_latents_compact_batch([files[0], bytes(unknown)], stack=False)
    with pytest.raises(ValueError, match=r"file 1 is a file in segments \(magic b'VBQb'\)"):
        q.decompress_latents_compact_batch([files[0], segments], stack=False)
    with pytest.raises(KeyError):
        q.compress_latents_to_compact_batch(lat[:2], [LAMBS[0], 3.0])
    with pytest.raises(ValueError, match="part"):
        q.compress_latents_to_compact_batch(lat[:2], LAMBS[0], part=0)
