"""Window and batch decode of latent files on the GPU: vbq_rans_decode_window_f32 against the known indices through
sorted[c][idx] and a NumPy slice, and the quantizer's decompress_latents_window / decompress_latents_batch against
decompress_latents and compress_latents, bit for bit -- damage, status bits and refusals included."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import adversarial_tables as AT  # noqa: E402
from oracle import c_oracle as CO

pytestmark = pytest.mark.gpu
N = 10
LAMBS = [2.0 ** -6, 2.0 ** -2, 2.0, 16.0]
S = slice


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


# ---------------------------------------------------------------------------------------------------------------- kernel level
class Coded:
    """Files coded with RansCodec.encode_packed, staged as the window decode reads them: one file per (leading shape, table).
    adversarial: tables and draws that do not fit each other (adversarial_tables.mixed_model) instead of the fitted ones; what
    the encoder made of them is compared with the C checker before anything decodes it."""

    def __init__(self, shapes, tables, n_tables, C_, seg, bits, seed, adversarial=False):
        from vbq_amd import _lib, ops
        from vbq_amd.coder import RansCodec, quantize_frequencies
        rng = np.random.default_rng(seed)
        T = 2 ** (bits + 1) - 1
        self.C, self.seg, self.bits, self.shapes, self.tables = C_, seg, bits, shapes, tables
        self.values = np.sort(rng.standard_normal((C_, T)).astype(np.float32), axis=1)
        centre = rng.integers(T // 8, T - T // 8, (n_tables, C_))
        spread = np.array([0.3, 2.0, 25.0, 300.0])[rng.integers(0, 4, (n_tables, C_))] * T / 2047
        draw = lambda t, n: np.clip(np.rint(rng.normal(centre[t, :, None], spread[t, :, None], (C_, n))), 0, T - 1).astype(np.uint16)
        if adversarial:
            self.freq, draw = AT.mixed_model(n_tables, C_, bits, seed)
        else:
            self.freq = np.stack([quantize_frequencies(np.stack([np.bincount(r, minlength=T) for r in draw(t, 4000)]))
                                  for t in range(n_tables)])
        self.idx, sizes, payloads, self.seg_base = [], [], [], []
        for shape, t in zip(shapes, tables):
            idx = draw(t, int(np.prod(shape)))
            sz, pay = RansCodec(self.freq[t], N=bits, segment=seg).encode_packed(torch.from_numpy(idx).cuda())
            if adversarial:
                w_ref, s_ref = CO.rans_encode(idx, self.freq[t], seg)
                assert np.array_equal(sz, s_ref)
                assert np.array_equal(pay, w_ref[np.arange(seg + 2)[None, None, :] < s_ref[..., None].astype(np.int64)])
            self.idx.append(idx)
            self.seg_base.append(sum(s.size for s in sizes))
            sizes.append(sz.reshape(-1).astype(np.uint16))
            payloads.append(pay)
        self.sizes_host, self.payload_host = np.concatenate(sizes), np.concatenate(payloads)
        self.sizes = torch.from_numpy(self.sizes_host).cuda()
        self.payload = torch.from_numpy(self.payload_host).cuda()
        self.offsets = torch.empty(self.sizes.numel(), dtype=torch.int64, device="cuda")
        st = torch.zeros(1, dtype=torch.uint32, device="cuda")
        _lib.check(_lib.lib().vbq_rans_segment_offsets_u16(ops._ptr(self.sizes), self.sizes.numel(), seg, self.payload.numel(),
                                                            ops._ptr(self.offsets), ops._ptr(st), None), "offsets")
        assert int(st.cpu().item()) == 0
        self.d_freq, self.d_values = torch.from_numpy(self.freq).cuda(), torch.from_numpy(self.values).cuda()
        # the reference, once: sorted[c][idx] channel-last, shaped like the latents
        self.full = [np.take_along_axis(self.values, i.astype(np.int64), axis=1).T.reshape(tuple(s) + (C_,))
                     for i, s in zip(self.idx, shapes)]

    def decode(self, regions, channels=None, payload=None, fill=None):
        """-> (out [F, *extents, C_sel] NumPy, status [F] list) of one launch over all files."""
        from vbq_amd import bitstream as bs, ops
        boxes, extents = bs.region_boxes(self.shapes, regions)
        lists = [bs.box_segments(d, lo, hi, self.seg) for d, lo, hi in boxes]
        n_sel = max(l.size for l in lists)
        segs = np.full((len(lists), n_sel), -1, np.int32)
        for f, l in enumerate(lists):
            segs[f, :l.size] = l
        files = np.array([[b, int(np.prod(s)), d[1], d[2], lo[0], lo[1], lo[2], t]
                          for b, s, (d, lo, hi), t in zip(self.seg_base, self.shapes, boxes, self.tables)], np.int64)
        box = tuple(h - l for l, h in zip(boxes[0][1], boxes[0][2]))
        ch = None if channels is None else torch.tensor(channels, dtype=torch.int32, device="cuda")
        n_ch_sel = self.C if channels is None else len(channels)
        out = None if fill is None else torch.full((len(lists),) + box + (n_ch_sel,), fill, dtype=torch.float32, device="cuda")
        out, st = ops.rans_decode_window(self.payload if payload is None else payload, self.sizes, self.offsets,
                                         torch.from_numpy(files).cuda(), torch.from_numpy(segs).cuda(), self.d_freq, self.d_values,
                                         box, seg=self.seg, N=self.bits, channels=ch, out=out)
        return out.cpu().numpy().reshape((len(lists),) + extents + (n_ch_sel,)), st.cpu().tolist(), lists

    def want(self, regions, channels=None):
        ch = slice(None) if channels is None else list(channels)
        return np.stack([full[tuple(r)][..., ch] for full, r in zip(self.full, regions)])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


KERNEL_CASES = {  # leading shape, segment, C, bits, a box of three levels where the shape allows one (two otherwise)
    "short-last-segment": ((1, 17, 23), 64, 3, N, (S(None), S(1, 16), S(3, 20))),
    "two-images": ((2, 17, 23), 64, 32, N, (S(None), S(1, 16), S(3, 20))),
    "three-workgroups": ((1, 25, 40), 7, 2, N, (S(None), S(2, 23), S(1, 39))),
    "kodak": ((1, 32, 48), 1024, 32, N, (S(None), S(2, 30), S(5, 40))),
    "four-bits": ((2, 9, 11), 16, 5, 4, (S(None), S(1, 8), S(2, 9))),
}


@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_kernel_boxes_and_channel_lists(case):
    shape, seg, C_, bits, nested = KERNEL_CASES[case]
    k = Coded([shape], [1], 2, C_, seg, bits, seed=len(case))
    D0, D1, D2 = shape
    n = D0 * D1 * D2
    r0 = (seg // D2 + 1) % D1                                   # rows r0 - 1 .. r0 + 1 in full cross a segment boundary where
    boxes = {"whole": (), "first": (S(0, 1), S(0, 1), S(0, 1)), "last": (S(D0 - 1, D0), S(D1 - 1, D1), S(D2 - 1, D2)),
             "rows": (S(0, 1), S(max(r0 - 1, 0), r0 + 2)), "columns": (S(None), S(None), S(7, 12)), "nested": nested}
    if seg < n:
        rows = np.arange(max(r0 - 1, 0) * D2, min(r0 + 2, D1) * D2)
        assert np.unique(rows // seg).size >= 2                  # ... the stream has more than one segment
    if case == "short-last-segment":
        assert n % seg == 7
    for name, region in boxes.items():
        region = tuple(region) + (S(None),) * (3 - len(region))
        got, st, lists = k.decode([region])
        assert st == [0], (name, st)
        assert np.array_equal(_bits(got), _bits(k.want([region]))), name
        if name in ("first", "last"):
            assert lists[0].tolist() == [0 if name == "first" else (n - 1) // seg]
    region = boxes["columns"]
    for channels in ([0], [C_ - 1], [5 % C_, 2 % C_, 2 % C_]):
        got, st, _ = k.decode([region], channels)
        assert st == [0] and np.array_equal(_bits(got), _bits(k.want([region], channels))), channels


def test_kernel_batch_of_three_files_and_damage_in_one():
    shapes = [(1, 17, 23), (1, 20, 30), (2, 9, 11)]
    regions = [(S(None), S(3, 11), S(5, 13)), (S(0, 1), S(12, 20), S(22, 30)), (S(1, 2), S(0, 8), S(2, 10))]
    k = Coded(shapes, [2, 0, 1], 3, 8, 64, N, seed=11)
    got, st, lists = k.decode(regions, fill=-7.0)
    assert len({l.size for l in lists}) > 1                      # lists of different lengths: padded with -1
    assert st == [0, 0, 0] and got.shape == (3, 1, 8, 8, 8)
    want = k.want(regions)
    assert np.array_equal(_bits(got), _bits(want))
    got, st, _ = k.decode(regions, [7, 0, 7])
    assert st == [0, 0, 0] and np.array_equal(_bits(got), _bits(k.want(regions, [7, 0, 7])))
    # one word of file 1, inside a segment its box touches (channel 4): that file's status alone, the other files' values right
    nseg1 = (20 * 30 + 63) // 64
    e = k.seg_base[1] + 4 * nseg1 + int(lists[1][0])
    damaged = k.payload_host.copy()
    damaged[int(k.offsets[e].item()) + int(k.sizes_host[e]) - 1] ^= 0x4000    # the high half of the segment's final state
    got, st, _ = k.decode(regions, payload=torch.from_numpy(damaged).cuda())
    assert st[0] == 0 and st[2] == 0 and st[1] != 0 and st[1] & ~(2 | 4) == 0, st
    assert np.array_equal(_bits(got[[0, 2]]), _bits(want[[0, 2]]))
    assert np.array_equal(_bits(np.delete(got[1], 4, axis=-1)), _bits(np.delete(want[1], 4, axis=-1)))


def test_kernel_batch_of_three_files_with_mismatched_tables():
    """A spike, the ramp and half_ones in the first channel of the three files (and cycling over the channels), none fitted to
    the data; every stream of file 0 holds only frequency-1 symbols, so its segments come close to seg + 2 words."""
    shapes = [(1, 17, 23), (1, 20, 30), (2, 9, 11)]
    regions = [(S(None), S(3, 11), S(5, 13)), (S(0, 1), S(12, 20), S(22, 30)), (S(1, 2), S(0, 8), S(2, 10))]
    k = Coded(shapes, [0, 1, 2], 3, 8, 64, 7, seed=13, adversarial=True)
    assert [k.freq[t, 0].tobytes() for t in range(3)] == [r.tobytes() for r in (AT.spike(7, 0), AT.ramp(), AT.half_ones(7))]
    assert np.all(np.take_along_axis(k.freq[0], k.idx[0].astype(np.int64), axis=1) == 1)         # file 0: all-rare data
    nseg0 = (17 * 23 + 63) // 64
    assert np.all(k.sizes_host[:8 * nseg0].reshape(8, nseg0)[:, :-1] == 2 + (15 * 64) // 16)     # 62 of at most 66 words
    got, st, lists = k.decode(regions, fill=-7.0)
    assert st == [0, 0, 0] and got.shape == (3, 1, 8, 8, 8)
    assert np.array_equal(_bits(got), _bits(k.want(regions)))
    got, st, _ = k.decode(regions, [7, 0, 7])
    assert st == [0, 0, 0] and np.array_equal(_bits(got), _bits(k.want(regions, [7, 0, 7])))
    for f, shape in enumerate(shapes):                           # every segment of every file
        one = Coded([shape], [f], 3, 8, 64, 7, seed=13 + f, adversarial=True)
        whole = (S(None),) * 3
        got, st, _ = one.decode([whole])
        assert st == [0] and np.array_equal(_bits(got), _bits(one.want([whole]))), f


def test_direct_c_call_sets_bits_5_and_7_per_file():
    """One direct C-ABI call over two files.  A listed id equal to nseg sets bit 5 in that file's status only and the other file's
    output is right; a descriptor whose box leaves the dimensions sets bit 7 and writes nothing of that file."""
    from vbq_amd import _lib
    shapes = [(1, 17, 23), (1, 17, 23)]
    k = Coded(shapes, [0, 0], 1, 3, 64, N, seed=5)
    nseg, n = 7, 391
    p = lambda t: C.c_void_p(t.data_ptr())                                  # noqa: E731
    region = (S(None), S(5, 9), S(None))                         # rows 5:9 in full: [115, 207) of one level, segments 1..3

    def call(files, segs):
        files, segs = torch.tensor(files, dtype=torch.int64, device="cuda"), torch.tensor(segs, dtype=torch.int32, device="cuda")
        out = torch.full((2, 1, 1, 92, 3), -7.0, dtype=torch.float32, device="cuda")
        st = torch.zeros(2, dtype=torch.uint32, device="cuda")
        r = _lib.lib().vbq_rans_decode_window_f32(p(k.payload), k.payload.numel(), p(k.sizes), p(k.offsets), k.sizes.numel(),
                                                  p(files), 2, p(segs), segs.shape[1], None, 3, 3, 64, N, p(k.d_freq), 1,
                                                  p(k.d_values), 1, 1, 92, p(out), p(st), None)
        torch.cuda.synchronize()
        assert r == 0, _lib.lib().vbq_last_error()
        return out.cpu().numpy().reshape(2, 1, 4, 23, 3), st.cpu().tolist()

    want = k.want([region, region])
    good = [[k.seg_base[0], n, 1, n, 0, 0, 115, 0], [k.seg_base[1], n, 1, n, 0, 0, 115, 0]]
    out, st = call(good, [[1, 2, 3, -1], [3, -1, 1, 2]])
    assert st == [0, 0] and np.array_equal(_bits(out), _bits(want))
    out, st = call(good, [[1, 2, 3, nseg], [1, 2, 3, -1]])
    assert st == [32, 0] and np.array_equal(_bits(out), _bits(want))         # the stray id wrote nothing; the rest is right
    out, st = call(good, [[1, 2, 3, -2], [1, 2, 3, -1]])
    assert st == [32, 0] and np.array_equal(_bits(out), _bits(want))
    for field, value in ((6, n - 91), (4, 1), (1, n + 1), (7, 1), (7, -1), (2, 0), (3, n - 1)):
        bad = [list(good[0]), list(good[1])]
        bad[1][field] = value
        out, st = call(bad, [[1, 2, 3], [1, 2, 3]])
        assert st == [0, 128], (field, value, st)
        assert np.array_equal(_bits(out[0]), _bits(want[0])) and np.all(out[1] == -7.0), (field, value)
    # size entries outside [0, M): bit 5, nothing read and nothing written
    for base in (k.sizes.numel() - 1, k.sizes.numel(), -1, 1 << 62):
        bad = [list(good[0]), list(good[1])]
        bad[1][0] = base
        out, st = call(bad, [[1, 2, 3], [1, 2, 3]])
        assert st == [0, 32] and np.array_equal(_bits(out[0]), _bits(want[0])) and np.all(out[1] == -7.0), base


# ------------------------------------------------------------------------------------------------------------- quantizer level
def _gaussian_quantizer(C_, seed):
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), C_))
    q = ChannelwisePriorCDFQuantizer(C_, N)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C_), scale))
    return q, scale, rng


def _latents(rng, scale, shape):
    m = (scale * rng.standard_normal(shape)).astype(np.float32)
    lv = (2 * (-2 + 0.7 * rng.standard_normal(shape))).astype(np.float32)
    return m, lv


@pytest.fixture(scope="module")
def kodak32():
    """A quantizer with C = 32, Kodak-shaped latents, their files at segment 64 and the full decodes: shared, never changed."""
    C_ = 32
    q, scale, rng = _gaussian_quantizer(C_, 7)
    m, lv = _latents(rng, scale, (1, 32, 48, C_))
    q.build_entropy_models_from_latents(m.reshape(-1, C_), lv.reshape(-1, C_), LAMBS, add_n_smoothing=1, spread="logvar")
    data = {lamb: q.compress_latents_to_bytes(m, lv, lamb, segment=64) for lamb in LAMBS}
    full = {lamb: q.decompress_latents(data[lamb]) for lamb in LAMBS}
    return q, scale, rng, m, lv, data, full


@pytest.mark.parametrize("C_", [32, 256])
def test_window_and_batch_match_the_full_decode(C_):
    q, scale, rng = _gaussian_quantizer(C_, C_)
    shapes = [(1, 32, 48, C_), (2, 17, 23, C_), (1, 20, 30, C_)]
    lat = [_latents(rng, scale, s) for s in shapes]
    q.build_entropy_models_from_latents(lat[0][0].reshape(-1, C_), lat[0][1].reshape(-1, C_), LAMBS, add_n_smoothing=1,
                                        spread="logvar")
    lambs = [LAMBS[1], LAMBS[3], LAMBS[0]]                       # mixed within the batch
    for seg in (64, 1024):
        files = [q.compress_latents_to_bytes(m, lv, lamb, segment=seg) for (m, lv), lamb in zip(lat, lambs)]
        full = [q.decompress_latents(d) for d in files]
        for (m, lv), lamb, z in zip(lat, lambs, full):
            assert np.array_equal(_bits(z), _bits(np.asarray(q.compress_latents(m, lv, [lamb])["Z_hat"][lamb])))
        regions = [(S(None), S(20, 28), S(40, 48)), (S(1, 2), S(9, 17), S(0, 8)), (S(None), S(3, 11), S(11, 19))]
        for channels in (None, [C_ - 1, 0, 5, 5]):
            ch = slice(None) if channels is None else channels
            want = np.stack([z[r][..., ch] for z, r in zip(full, regions)])
            got = q.decompress_latents_batch(files, regions, channels=channels)
            assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
            got = q.decompress_latents_batch(files, regions, channels=channels, return_np=True)
            assert isinstance(got, np.ndarray) and np.array_equal(_bits(got), _bits(want))
            for d, r, w in zip(files, regions, want):
                z = q.decompress_latents_window(d, r, channels=channels)
                assert isinstance(z, np.ndarray) and np.array_equal(_bits(z), _bits(w))
        zt = q.decompress_latents_window(files[1], (S(None), S(2, 3)), return_np=False)       # trailing axes in full
        assert isinstance(zt, torch.Tensor) and zt.is_cuda and np.array_equal(_bits(zt.cpu().numpy()), _bits(full[1][:, 2:3]))
        # one region for all files, and whole files
        same = [files[0], q.compress_latents_to_bytes(*lat[0], LAMBS[2], segment=seg)]
        got = q.decompress_latents_batch(same, (S(None), S(5, 9)), return_np=True)
        assert np.array_equal(_bits(got), _bits(np.stack([q.decompress_latents(d)[:, 5:9] for d in same])))
        got = q.decompress_latents_batch(same, return_np=True)
        assert np.array_equal(_bits(got), _bits(np.stack([q.decompress_latents(d) for d in same])))
        assert np.array_equal(_bits(q.decompress_latents_window(files[1], None)), _bits(full[1]))


def test_repeated_code_points():
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
    ref = q.compress_latents(m, lv, lambs)
    region = (S(None), S(7, 33), S(11, 12))
    for seg in (64, 1024):
        files = [q.compress_latents_to_bytes(m, lv, lamb, segment=seg) for lamb in lambs]
        got = q.decompress_latents_batch(files, region, return_np=True)
        assert np.array_equal(_bits(got), _bits(np.stack([np.asarray(ref["Z_hat"][lamb])[region] for lamb in lambs])))
        got = q.decompress_latents_window(files[2], region, channels=[1])
        assert np.array_equal(_bits(got), _bits(np.asarray(ref["Z_hat"][lambs[2]])[region][..., [1]]))


def _flip_that_the_checker_rejects(q, data, lamb, c, g):
    """`data` with one payload word of segment g (>= 1) of channel c flipped, the first word (in file order) after whose flip
    the CPU checker reports the segment damaged.  The checker decodes segments g - 1 and g as one stream of two segments, so
    that whatever it reads before a starved segment's first word still lies in its buffer."""
    from vbq_amd import bitstream
    h, sizes, start = bitstream.parse(data)
    seg, nseg = h.segment, h.nseg
    freq = q._coder_tables(q._lambda_key(lamb), seg)[0].freq_host.numpy()[c: c + 1]
    offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    pay = np.frombuffer(data, dtype="<u2", count=h.n_words, offset=start)
    n = seg + min(seg, h.n_rows - g * seg)
    for w in range(int(sizes[c * nseg + g])):
        words, sz = np.zeros((1, 2, seg + 2), np.uint16), np.zeros((1, 2), np.uint32)
        for j, e in enumerate((c * nseg + g - 1, c * nseg + g)):
            sz[0, j] = sizes[e]
            words[0, j, :sizes[e]] = pay[offs[e]: offs[e + 1]]
        CO.rans_decode(words, sz, freq, n, seg)                  # the segments as they are: accepted
        words[0, 1, w] ^= 0x0100
        try:
            CO.rans_decode(words, sz, freq, n, seg)
        except AssertionError:
            flipped = bytearray(data)
            flipped[start + 2 * (int(offs[c * nseg + g]) + w) + 1] ^= 0x01
            return bytes(flipped)
    raise AssertionError("no single flip of this segment is rejected by the checker")


def test_damage_outside_the_window_goes_unseen_and_inside_it_raises(kodak32):
    from vbq_amd import _lib
    q, scale, rng, m, lv, data, full = kodak32
    lamb = LAMBS[1]
    region = (S(None), S(8, 16), S(10, 30))                      # rows [384, 768): segments 6 .. 11 of the 24 of a channel
    want = full[lamb][region]
    outside = _flip_that_the_checker_rejects(q, data[lamb], lamb, 3, 20)
    inside = _flip_that_the_checker_rejects(q, data[lamb], lamb, 3, 8)
    assert np.array_equal(_bits(q.decompress_latents_window(outside, region)), _bits(want))
    with pytest.raises(_lib.VBQError):
        q.decompress_latents(outside)
    with pytest.raises(_lib.VBQError, match="file 0"):
        q.decompress_latents_window(inside, region)
    assert np.array_equal(_bits(q.decompress_latents_window(inside, region, channels=[2, 4])), _bits(want[..., [2, 4]]))
    # in a batch: the message names the damaged file; the same files decode where no box touches the damage
    files = [data[LAMBS[0]], inside, data[LAMBS[2]]]
    with pytest.raises(_lib.VBQError, match="file 1: rANS bitstream rejected"):
        q.decompress_latents_batch(files, region)
    away = (S(None), S(20, 28), S(10, 30))
    got = q.decompress_latents_batch(files, [region, away, region], return_np=True)
    assert np.array_equal(_bits(got), _bits(np.stack([full[LAMBS[0]][region], full[lamb][away], full[LAMBS[2]][region]])))
    with pytest.raises(_lib.VBQError, match="file 2"):
        q.decompress_latents_batch([data[LAMBS[0]], data[LAMBS[2]], inside], region)


def test_refusals(kodak32):
    q, scale, _, m, lv, data, full = kodak32
    rng = np.random.default_rng(99)
    lamb = LAMBS[1]
    good = data[lamb]
    region = (S(None), S(0, 4), S(0, 4))
    compact = q.compress_latents_to_bytes(m, lv, lamb, layout="interleaved")
    mapped = q.compress_latents_to_bytes_mapped(m, lv, LAMBS[:2], np.zeros((1, 32, 48), np.int64), segment=64)
    with pytest.raises(ValueError, match="file 1 is a compact file"):
        q.decompress_latents_batch([good, compact], region)
    with pytest.raises(ValueError, match="file 0 is a lambda-map file"):
        q.decompress_latents_window(mapped, region)
    with pytest.raises(ValueError, match="file 2 is in segments of 1024 symbols, file 0 in segments of 64"):
        q.decompress_latents_batch([good, good, q.compress_latents_to_bytes(m, lv, lamb, segment=1024)], region)
    with pytest.raises(ValueError, match="file 1: a region of extents"):
        q.decompress_latents_batch([good, good], [region, (S(None), S(0, 4), S(0, 5))])
    m2, lv2 = _latents(rng, scale, (1, 20, 30, 32))
    with pytest.raises(ValueError, match="file 1: a region of extents"):
        q.decompress_latents_batch([good, q.compress_latents_to_bytes(m2, lv2, lamb, segment=64)])     # whole files of two shapes
    with pytest.raises(ValueError, match="2 regions for 1 files"):
        q.decompress_latents_batch([good], [region, region])
    with pytest.raises(ValueError, match="file 1: truncated"):
        q.decompress_latents_batch([good, good[:-2]], region)
    for channels in ([32], [-1], [0.5]):
        with pytest.raises(ValueError, match="channels"):
            q.decompress_latents_window(good, region, channels=channels)
    with pytest.raises(ValueError, match="not a slice"):
        q.decompress_latents_window(good, (0, S(0, 4)))
    with pytest.raises(KeyError):
        d = bytearray(good)
        d[16:24] = np.float64(3.0).tobytes()                     # a lambda this quantizer has no model for
        q.decompress_latents_window(bytes(d), region)
    # a foreign digest: the same code points, models fitted on other data
    q2, _, _ = _gaussian_quantizer(32, 7)
    m3, lv3 = _latents(rng, scale * 2, (1, 32, 48, 32))
    q2.build_entropy_models_from_latents(m3.reshape(-1, 32), lv3.reshape(-1, 32), LAMBS, add_n_smoothing=1, spread="logvar")
    with pytest.raises(ValueError, match="file 0 was compressed with a different quantizer or entropy model"):
        q2.decompress_latents_window(good, region)
    with pytest.raises(ValueError, match="file 0 is for N = 10, C = 32"):
        _gaussian_quantizer(16, 1)[0].decompress_latents_window(good, region)
    # empty extents and empty channel lists: an empty tensor, no launch
    z = q.decompress_latents_batch([good, good], (S(None), S(4, 4)), return_np=True)
    assert z.shape == (2, 1, 0, 48, 32) and z.dtype == np.float32
    assert tuple(q.decompress_latents_window(good, region, channels=[], return_np=False).shape) == (1, 4, 4, 0)
    assert q.decompress_latents_batch([], region, return_np=True).shape[0] == 0
    assert np.array_equal(_bits(q.decompress_latents_window(good, region)), _bits(full[lamb][region]))
