"""Window and batch decode of lambda-map files on the GPU: vbq_rans_map_decode_window_f32 against the known indices through
sorted[c][idx] and a NumPy slice, bit for bit, over class maps, palettes, segment lengths, boxes and channel lists; against
vbq_rans_decode_window_f32 for files without a class block; its status bits for inputs staged by hand; and the quantizer's
decompress_latents_mapped_window / decompress_latents_mapped_batch against decompress_latents and compress_latents_mapped."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import adversarial_tables as AT  # noqa: E402
import mapped_reference as MR  # noqa: E402

pytestmark = pytest.mark.gpu
N = 10
LAMBS = [2.0 ** -6, 2.0 ** -2, 2.0, 16.0]
S = slice


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- kernel level
def class_maps(P, n, rng):
    """name -> u8 [n]: constant (the last class), halves, a change at every symbol, random, and for P >= 3 a map in which
    class 1 never occurs."""
    out = {"constant": np.full(n, P - 1, np.uint8), "halves": (np.arange(n) >= n // 2).astype(np.uint8) * (P - 1),
           "checker": (np.arange(n) % P).astype(np.uint8), "random": rng.integers(0, P, n).astype(np.uint8)}
    if P >= 3:
        out["skip1"] = np.where(rng.integers(0, 2, n) == 0, 0, P - 1).astype(np.uint8)
    return out


class MappedCoded:
    """Files coded with MappedRansCodec.encode_packed, staged as the mapped window decode reads them.  files: a list of (leading
    shape, palette = rows of the frequency stack, class map u8 [n] or None: a file without a class block, P = 1).  The tables
    are fitted around different centres, as Coded of test_gpu_window.py does, so that a wrong class decodes a wrong value."""

    def __init__(self, files, n_tables, C_, seg, bits, seed, model=None):
        from vbq_amd import _lib, bitstream as bs, ops
        from vbq_amd.coder import MappedRansCodec, quantize_frequencies
        rng = np.random.default_rng(seed)
        T = 2 ** (bits + 1) - 1
        self.C, self.seg, self.bits, self.n_tables = C_, seg, bits, n_tables
        self.shapes = [f[0] for f in files]
        self.values = np.sort(rng.standard_normal((C_, T)).astype(np.float32), axis=1)
        if model is None:
            centre = rng.integers(T // 8, T - T // 8, (n_tables, C_))
            spread = np.array([0.3, 2.0, 25.0, 300.0])[rng.integers(0, 4, (n_tables, C_))] * T / 2047
            draw = lambda t, n: np.clip(np.rint(rng.normal(centre[t, :, None], spread[t, :, None], (C_, n))), 0, T - 1).astype(np.uint16)
            self.freq = np.stack([quantize_frequencies(np.stack([np.bincount(r, minlength=T) for r in draw(t, 4000)]))
                                  for t in range(n_tables)])
        else:
            self.freq, draw = model
        self.idx, sizes, payloads, self.seg_base, self.cls_base, self.palettes, self.cls = [], [], [], [], [], [], []
        area = b""
        for shape, palette, cls in files:
            n = int(np.prod(shape))
            planes = np.stack([draw(t, n) for t in palette])                                  # [P, C, n]
            c = np.zeros(n, np.uint8) if cls is None else np.asarray(cls, np.uint8)
            assert c.size == n and int(c.max()) < len(palette)
            codec = MappedRansCodec(self.freq[list(palette)], N=bits, segment=seg)
            sz, pay = codec.encode_packed(torch.from_numpy(planes).cuda(), c)
            self.idx.append(MR.select(planes, c))
            self.seg_base.append(sum(s.size for s in sizes))
            sizes.append(sz.reshape(-1).astype(np.uint16))
            payloads.append(pay)
            self.palettes.append(list(palette))
            self.cls.append(c)
            self.cls_base.append(-1 if cls is None else len(area))
            if cls is not None:
                area += bs.pack_classes(c)
        self.area_host = np.frombuffer(area, np.uint8).copy()
        self.sizes_host, self.payload_host = np.concatenate(sizes), np.concatenate(payloads)
        self.sizes = torch.from_numpy(self.sizes_host).cuda()
        self.payload = torch.from_numpy(self.payload_host).cuda()
        self.offsets = torch.empty(self.sizes.numel(), dtype=torch.int64, device="cuda")
        st = torch.zeros(1, dtype=torch.uint32, device="cuda")
        _lib.check(_lib.lib().vbq_rans_segment_offsets_u16(ops._ptr(self.sizes), self.sizes.numel(), seg, self.payload.numel(),
                                                            ops._ptr(self.offsets), ops._ptr(st), None), "offsets")
        assert int(st.cpu().item()) == 0
        self.d_freq, self.d_values = torch.from_numpy(self.freq).cuda(), torch.from_numpy(self.values).cuda()
        self.max_P = max(len(p) for p in self.palettes)
        # the reference, once: sorted[c][idx] channel-last, shaped like the latents
        self.full = [np.take_along_axis(self.values, i.astype(np.int64), axis=1).T.reshape(tuple(s) + (C_,))
                     for i, s in zip(self.idx, self.shapes)]

    def stage(self, regions):
        """-> (files int64 [F, 16], segs int32 [F, n_sel], box, extents, lists) on the host."""
        from vbq_amd import bitstream as bs
        boxes, extents = bs.region_boxes(self.shapes, regions)
        lists = [bs.box_segments(d, lo, hi, self.seg) for d, lo, hi in boxes]
        n_sel = max(l.size for l in lists)
        segs = np.full((len(lists), n_sel), -1, np.int32)
        for f, l in enumerate(lists):
            segs[f, :l.size] = l
        files = np.zeros((len(lists), 16), np.int64)
        for f, (b, s, (d, lo, hi), pal, cb) in enumerate(zip(self.seg_base, self.shapes, boxes, self.palettes, self.cls_base)):
            files[f, :8] = (b, int(np.prod(s)), d[1], d[2], lo[0], lo[1], lo[2], len(pal))
            files[f, 8: 8 + len(pal)] = pal
            files[f, 12] = cb
        return files, segs, tuple(h - l for l, h in zip(boxes[0][1], boxes[0][2])), extents, lists

    def decode(self, regions, channels=None, payload=None, fill=None, files=None, segs=None, area=None, sizes=None, max_P=None):
        """-> (out [F, *extents, C_sel] NumPy, status [F] list, lists) of ONE launch over all files; files / segs / area / sizes /
        payload replace what stage() made."""
        from vbq_amd import ops
        f0, s0, box, extents, lists = self.stage(regions)
        files = f0 if files is None else files
        segs = s0 if segs is None else segs
        area = self.area_host if area is None else area
        ch = None if channels is None else torch.tensor(channels, dtype=torch.int32, device="cuda")
        n_ch_sel = self.C if channels is None else len(channels)
        F = len(lists)
        out = None if fill is None else torch.full((F,) + box + (n_ch_sel,), fill, dtype=torch.float32, device="cuda")
        out, st = ops.rans_map_decode_window(self.payload if payload is None else payload, self.sizes if sizes is None else sizes,
                                             self.offsets, torch.from_numpy(files).cuda(), torch.from_numpy(segs).cuda(),
                                             self.d_freq, self.d_values, torch.from_numpy(area).cuda() if area.size else None, box,
                                             seg=self.seg, max_classes=self.max_P if max_P is None else max_P, N=self.bits,
                                             channels=ch, out=out)
        return out.cpu().numpy().reshape((F,) + extents + (n_ch_sel,)), st.cpu().tolist(), lists

    def want(self, regions, channels=None):
        ch = slice(None) if channels is None else list(channels)
        return np.stack([full[tuple(r)][..., ch] for full, r in zip(self.full, regions)])


KERNEL_CASES = {  # leading shape, segment, C, bits, a nested box
    # 1025 positions: not a multiple of 4, padding bits in the last byte; segments of 7 enter the class words mid-word and
    # mid-byte; 147 segments per stream: three workgroups
    "seg7-three-workgroups": ((1, 25, 41), 7, 2, N, (S(None), S(2, 23), S(1, 39))),
    # 391 = 4 * 97 + 3 positions, 13 words and a padded last one; segments of 30: mid-byte; a last segment of one symbol
    "seg30-short-last-segment": ((1, 17, 23), 30, 3, N, (S(None), S(1, 16), S(3, 20))),
    "seg64-word-aligned": ((2, 17, 23), 64, 8, N, (S(None), S(1, 16), S(3, 20))),
    "seg1024-kodak": ((1, 32, 48), 1024, 32, N, (S(None), S(2, 30), S(5, 40))),
    "four-bits": ((2, 9, 11), 16, 5, 4, (S(None), S(1, 8), S(2, 9))),
}
WHOLE = (S(None),) * 3


@pytest.mark.parametrize("P", [1, 2, 3, 4])
@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_kernel_class_maps_and_palettes(case, P):
    """One file per class map, all in ONE launch, whole; the palettes take different rows of a stack of five tables."""
    shape, seg, C_, bits, _ = KERNEL_CASES[case]
    n = int(np.prod(shape))
    maps = class_maps(P, n, np.random.default_rng(P))
    names = list(maps)
    palettes = [[(3 * i + 2 * p + 1) % 5 for p in range(P)] for i in range(len(names))]
    k = MappedCoded([(shape, pal, maps[name]) for name, pal in zip(names, palettes)], 5, C_, seg, bits, seed=len(case) + P)
    if P >= 3:
        assert not (maps["skip1"] == 1).any()
    assert n % seg != 0 and (case != "seg7-three-workgroups" or (n % 4 == 1 and (n + seg - 1) // seg > 128))
    got, st, _ = k.decode([WHOLE] * len(names), fill=-7.0)
    assert st == [0] * len(names), st
    want = k.want([WHOLE] * len(names))
    for f, name in enumerate(names):
        assert np.array_equal(_bits(got[f]), _bits(want[f])), name


@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_kernel_boxes_and_channel_lists(case):
    shape, seg, C_, bits, nested = KERNEL_CASES[case]
    D0, D1, D2 = shape
    n = D0 * D1 * D2
    rng = np.random.default_rng(len(case))
    k = MappedCoded([(shape, [2, 0, 3], rng.integers(0, 3, n).astype(np.uint8))], 4, C_, seg, bits, seed=len(case))
    r0 = (seg // D2 + 1) % D1                                   # rows r0 - 1 .. r0 + 1 in full cross a segment boundary
    boxes = {"whole": (), "first": (S(0, 1), S(0, 1), S(0, 1)), "last": (S(D0 - 1, D0), S(D1 - 1, D1), S(D2 - 1, D2)),
             "rows": (S(0, 1), S(max(r0 - 1, 0), r0 + 2)), "columns": (S(None), S(None), S(7, 12)), "nested": nested}
    rows = np.arange(max(r0 - 1, 0) * D2, min(r0 + 2, D1) * D2)
    assert np.unique(rows // seg).size >= 2
    for name, region in boxes.items():
        region = tuple(region) + (S(None),) * (3 - len(region))
        got, st, lists = k.decode([region], fill=-7.0)
        assert st == [0], (name, st)
        assert np.array_equal(_bits(got), _bits(k.want([region]))), name
        if name in ("first", "last"):
            assert lists[0].tolist() == [0 if name == "first" else (n - 1) // seg]
    region = boxes["columns"]
    for channels in ([0], list(range(C_))[::-1], [5 % C_, 2 % C_, 2 % C_]):
        got, st, _ = k.decode([region], channels)
        assert st == [0] and np.array_equal(_bits(got), _bits(k.want([region], channels))), channels


SHAPES3 = [(1, 17, 23), (1, 20, 30), (2, 9, 11)]
REGIONS3 = [(S(None), S(3, 11), S(5, 13)), (S(0, 1), S(12, 20), S(22, 30)), (S(1, 2), S(0, 8), S(2, 10))]


@pytest.fixture(scope="module")
def three():
    """P = 1 without a class block, P = 2 and P = 4 in one staging: shared, never changed."""
    rng = np.random.default_rng(17)
    return MappedCoded([(SHAPES3[0], [2], None), (SHAPES3[1], [0, 3], rng.integers(0, 2, 600).astype(np.uint8)),
                        (SHAPES3[2], [1, 4, 0, 2], rng.integers(0, 4, 198).astype(np.uint8))], 5, 8, 64, N, seed=11)


def test_kernel_one_launch_of_palettes_of_one_two_and_four(three):
    k = three
    assert k.cls_base == [-1, 0, 152] and k.max_P == 4           # 600 positions: 19 words of 8 bytes
    got, st, lists = k.decode(REGIONS3, fill=-7.0)
    assert len({l.size for l in lists}) > 1                      # lists of different lengths: padded with -1
    assert st == [0, 0, 0] and got.shape == (3, 1, 8, 8, 8)
    assert np.array_equal(_bits(got), _bits(k.want(REGIONS3)))
    got, st, _ = k.decode(REGIONS3, [7, 0, 7])
    assert st == [0, 0, 0] and np.array_equal(_bits(got), _bits(k.want(REGIONS3, [7, 0, 7])))
    # what the unused table fields hold does not matter
    files = k.stage(REGIONS3)[0]
    files[0, 9:12] = (99, -5, 1 << 40)
    got, st, _ = k.decode(REGIONS3, files=files)
    assert st == [0, 0, 0] and np.array_equal(_bits(got), _bits(k.want(REGIONS3)))


def test_files_without_a_class_block_equal_the_plain_kernel():
    from vbq_amd import ops
    k = MappedCoded([(s, [t], None) for s, t in zip(SHAPES3, (2, 0, 1))], 3, 8, 64, N, seed=23)
    files, segs, box, extents, _ = k.stage(REGIONS3)
    assert k.max_P == 1 and k.area_host.size == 0 and files[:, 7].tolist() == [1, 1, 1] and files[:, 12].tolist() == [-1] * 3
    for channels in (None, [7, 0, 7]):
        got, st, _ = k.decode(REGIONS3, channels, fill=-7.0)
        plain = files[:, :8].copy()
        plain[:, 7] = files[:, 8]
        ch = None if channels is None else torch.tensor(channels, dtype=torch.int32, device="cuda")
        out = torch.full((3,) + box + (8 if channels is None else 3,), -7.0, dtype=torch.float32, device="cuda")
        ref, st_ref = ops.rans_decode_window(k.payload, k.sizes, k.offsets, torch.from_numpy(plain).cuda(), torch.from_numpy(segs).cuda(),
                                             k.d_freq, k.d_values, box, seg=64, N=N, channels=ch, out=out)
        assert st == st_ref.cpu().tolist() == [0, 0, 0]
        assert np.array_equal(_bits(got.reshape(-1)), _bits(ref.cpu().numpy().reshape(-1)))
        assert np.array_equal(_bits(got), _bits(k.want(REGIONS3, channels)))


def test_kernel_adversarial_tables():
    """Tables of other families per (class, stream) that do not fit the data (tests/adversarial_tables.py), a class change at
    every symbol; what the encoder made of them is compared with the NumPy coder before anything decodes it."""
    from vbq_amd.coder import MappedRansCodec
    P, n, bits = 3, 1003, 7
    planes, freq, cls, idx, w_ref, s_ref = AT.mapped_case(P, n, bits, "per-symbol")
    sz, pay = MappedRansCodec(freq.copy(), N=bits, segment=AT.MAPPED_SEG).encode_packed(torch.from_numpy(planes.copy()).cuda(), cls)
    assert np.array_equal(sz, s_ref)
    assert pay.tobytes() == w_ref[np.arange(AT.MAPPED_SEG + 2)[None, None, :] < s_ref[..., None].astype(np.int64)].tobytes()
    k = MappedCoded([((1, 17, 59), [0, 1, 2], cls)], P, AT.MAPPED_S, AT.MAPPED_SEG, bits, seed=3,
                    model=(freq.copy(), lambda t, m: planes[t]))
    assert np.array_equal(k.idx[0], idx) and k.payload_host.tobytes() == pay.tobytes()
    for region in (WHOLE, (S(None), S(3, 11), S(5, 50))):
        got, st, _ = k.decode([region])
        assert st == [0] and np.array_equal(_bits(got), _bits(k.want([region])))


# ---- status bits: inputs the kernel is specified to reject, staged by hand, one launch per cause.  Every index formed from
# ---- them is compared with its range first, so each launch completes and reports.
def test_a_class_outside_the_palette_sets_bit_6(three):
    k = three
    want = k.want(REGIONS3)
    # file 1 (P = 2, 20 x 30, box rows 12..19 x columns 22..29): class 2 at row 14, column 25 = position 445, in segment 6
    pos = 14 * 30 + 25
    area = k.area_host.copy()
    area[k.cls_base[1] + pos // 4] |= 2 << 2 * (pos % 4)
    got, st, _ = k.decode(REGIONS3, area=area, fill=-7.0)
    assert st == [0, 64, 0], st
    assert np.array_equal(_bits(got[[0, 2]]), _bits(want[[0, 2]]))
    rows = (np.arange(12, 20)[:, None] * 30 + np.arange(22, 30)[None, :])                      # the box's positions
    hit = (rows // 64 == pos // 64) & (rows >= pos)
    assert hit.sum() >= 2 and np.all(got[1, 0][hit] == 0.0)                                   # zeros from there on
    assert np.array_equal(_bits(got[1, 0][~hit]), _bits(want[1, 0][~hit]))                    # the rest of the file is right


@pytest.mark.parametrize("field,value", [(12, 4), (12, 156), (12, 208), (12, 64), (12, -8), (12, -2), (12, 1 << 62), (7, 0), (7, 5),
                                         (7, -1), (8, 5), (8, -1), (9, 5), (9, 1 << 40)])
def test_an_inconsistent_descriptor_sets_bit_7_and_writes_nothing(three, field, value):
    """File 1 (P = 2; its class block: 152 bytes at offset 0 of an area of 208): cls_base misaligned, misaligned further in,
    at the end of the area, aligned with too few bytes left (64 + 152 > 208), negative, huge; P = 0, 5, -1; the table of class
    0 or of class 1 out of range."""
    k = three
    assert k.area_host.size == 208
    files = k.stage(REGIONS3)[0]
    files[1, field] = value
    got, st, _ = k.decode(REGIONS3, files=files, fill=-7.0)
    assert st == [0, 128, 0], st
    want = k.want(REGIONS3)
    assert np.array_equal(_bits(got[[0, 2]]), _bits(want[[0, 2]])) and np.all(got[1] == -7.0)


def test_a_palette_larger_than_the_launch_allows_sets_bit_7(three):
    k = three
    got, st, _ = k.decode(REGIONS3, fill=-7.0, max_P=2)           # tables for two classes in LDS: file 2 (P = 4) is refused
    assert st == [0, 0, 128] and np.all(got[2] == -7.0)
    assert np.array_equal(_bits(got[:2]), _bits(k.want(REGIONS3)[:2]))


def test_damaged_payload_and_ids_set_their_bits_on_that_file_only(three):
    k = three
    want = k.want(REGIONS3)
    files, segs, _, _, lists = k.stage(REGIONS3)
    # the payload one word short: the last segment of the last file no longer lies in [0, n_words) -- bit 0 on that file
    got, st, _ = k.decode([(S(None), S(0, 8), S(0, 8)), (S(None), S(0, 8), S(0, 8)), (S(1, 2), S(1, 9), S(3, 11))],
                          payload=torch.from_numpy(k.payload_host[:-1].copy()).cuda())
    assert st == [0, 0, 1], st
    # one word of file 1, inside a segment its box touches (channel 4): the high half of the segment's final state
    nseg1 = (20 * 30 + 63) // 64
    e = k.seg_base[1] + 4 * nseg1 + int(lists[1][0])
    damaged = k.payload_host.copy()
    damaged[int(k.offsets[e].item()) + int(k.sizes_host[e]) - 1] ^= 0x4000
    got, st, _ = k.decode(REGIONS3, payload=torch.from_numpy(damaged).cuda())
    assert st[0] == 0 and st[2] == 0 and st[1] != 0 and st[1] & ~(2 | 4) == 0, st
    assert np.array_equal(_bits(got[[0, 2]]), _bits(want[[0, 2]]))
    assert np.array_equal(_bits(np.delete(got[1], 4, axis=-1)), _bits(np.delete(want[1], 4, axis=-1)))
    # a size entry of that segment outside [2, seg + 2]: bit 0
    for size in (1, 67):
        sizes = k.sizes_host.copy()
        sizes[e] = size
        got, st, _ = k.decode(REGIONS3, sizes=torch.from_numpy(sizes).cuda())
        assert st == [0, 1, 0], (size, st)
        assert np.array_equal(_bits(np.delete(got[1], 4, axis=-1)), _bits(np.delete(want[1], 4, axis=-1)))
    # listed ids outside [0, nseg): bit 5, nothing written for them, the rest right
    for stray in (nseg1, -2, 1 << 30):
        bad = np.concatenate([segs, np.full((3, 1), -1, np.int32)], axis=1)
        bad[1, -1] = stray
        got, st, _ = k.decode(REGIONS3, segs=bad, fill=-7.0)
        assert st == [0, 32, 0], (stray, st)
        assert np.array_equal(_bits(got), _bits(want))
    # a size entry outside [0, M): bit 5
    for base in (k.sizes.numel() - 1, k.sizes.numel(), -1, 1 << 62):
        bad = files.copy()
        bad[1, 0] = base
        got, st, _ = k.decode(REGIONS3, files=bad, fill=-7.0)
        assert st == [0, 32, 0] and np.all(got[1] == -7.0) and np.array_equal(_bits(got[[0, 2]]), _bits(want[[0, 2]])), base


# ------------------------------------------------------------------------------------------------------------- quantizer level
C32 = 32
Q_SHAPES = [(1, 16, 48, C32), (2, 9, 23, C32), (1, 20, 30, C32), (1, 12, 40, C32)]
Q_REGIONS = [(S(None), S(8, 16), S(40, 48)), (S(1, 2), S(1, 9), S(0, 8)), (S(None), S(3, 11), S(11, 19)), (S(None), S(4, 12), S(30, 38))]


@pytest.fixture(scope="module")
def world():
    """A quantizer with C = 32, four latents of different shapes, their files at segment 64 -- palettes of 2 lambdas, one
    lambda in segments (b"VBQb"), 4 and 3 lambdas -- and what decompress_latents and compress_latents_mapped give: shared,
    never changed."""
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    rng = np.random.default_rng(7)
    scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), C32))
    q = ChannelwisePriorCDFQuantizer(C32, N)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C32), scale))
    lat = [((scale * rng.standard_normal(s)).astype(np.float32), (2 * (-2 + 0.7 * rng.standard_normal(s))).astype(np.float32))
           for s in Q_SHAPES]
    q.build_entropy_models_from_latents(lat[0][0].reshape(-1, C32), lat[0][1].reshape(-1, C32), LAMBS, add_n_smoothing=1,
                                        spread="logvar")
    palettes = [[LAMBS[3], LAMBS[0]], [LAMBS[2]], [LAMBS[1], LAMBS[3], LAMBS[0], LAMBS[2]], [LAMBS[2], LAMBS[0], LAMBS[3]]]
    classes = [rng.integers(0, len(p), s[:-1]) for p, s in zip(palettes, Q_SHAPES)]
    files = [q.compress_latents_to_bytes(m, lv, pal[0], segment=64) if f == 1 else
             q.compress_latents_to_bytes_mapped(m, lv, pal, cl, segment=64)
             for f, ((m, lv), pal, cl) in enumerate(zip(lat, palettes, classes))]
    assert [bytes(d[:4]) for d in files] == [b"VBQm", b"VBQb", b"VBQm", b"VBQm"]
    full = [q.decompress_latents(d) for d in files]
    direct = [np.asarray(q.compress_latents_mapped(m, lv, pal, cl if f != 1 else np.zeros_like(cl))["Z_hat"])
              for f, ((m, lv), pal, cl) in enumerate(zip(lat, palettes, classes))]
    return q, files, full, direct


@pytest.mark.parametrize("channels", [None, [C32 - 1, 0, 5, 5]])
def test_batch_and_window_match_the_full_decode(world, channels):
    q, files, full, direct = world
    ch = slice(None) if channels is None else channels
    want = np.stack([z[r][..., ch] for z, r in zip(full, Q_REGIONS)])
    assert np.array_equal(_bits(want), _bits(np.stack([z[r][..., ch] for z, r in zip(direct, Q_REGIONS)])))
    got = q.decompress_latents_mapped_batch(files, Q_REGIONS, channels=channels)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    got = q.decompress_latents_mapped_batch(files, Q_REGIONS, channels=channels, return_np=True)
    assert isinstance(got, np.ndarray) and np.array_equal(_bits(got), _bits(want))
    for d, r, w in zip(files, Q_REGIONS, want):
        z = q.decompress_latents_mapped_window(d, r, channels=channels)
        assert isinstance(z, np.ndarray) and np.array_equal(_bits(z), _bits(w))
        one = q.decompress_latents_mapped_batch([d], [r], channels=channels, return_np=True)
        assert one.shape == (1,) + z.shape and np.array_equal(_bits(one[0]), _bits(z))
    zt = q.decompress_latents_mapped_window(files[3], (S(None), S(2, 3)), return_np=False)      # trailing axes in full
    assert isinstance(zt, torch.Tensor) and zt.is_cuda and np.array_equal(_bits(zt.cpu().numpy()), _bits(full[3][:, 2:3]))
    assert np.array_equal(_bits(q.decompress_latents_mapped_window(files[2], None)), _bits(full[2]))   # a whole file
    same = [files[0], files[0]]                                                                  # one region for all files
    got = q.decompress_latents_mapped_batch(same, (S(None), S(5, 9)), return_np=True)
    assert np.array_equal(_bits(got), _bits(np.stack([full[0][:, 5:9]] * 2)))


def _flip_final_state(data, c, g):
    """`data` (a lambda-map file) with the high half of the final state of segment g of channel c flipped in one bit."""
    from vbq_amd import bitstream
    h, _, sizes, start = bitstream.parse_mapped(data)
    offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    e = c * h.nseg + g
    flipped = bytearray(data)
    flipped[start + 2 * (int(offs[e]) + int(sizes[e]) - 1) + 1] ^= 0x40
    return bytes(flipped)


def test_damage_inside_a_box_names_the_file_and_outside_goes_unseen(world):
    from vbq_amd import _lib
    q, files, full, direct = world
    # file 2: 20 x 30, box rows 3..10 x columns 11..18: positions 101 .. 318, segments 1 .. 4 of 10
    inside, outside = _flip_final_state(files[2], 3, 2), _flip_final_state(files[2], 3, 8)
    with pytest.raises(_lib.VBQError, match="file 2: rANS bitstream rejected"):
        q.decompress_latents_mapped_batch(files[:2] + [inside, files[3]], Q_REGIONS)
    with pytest.raises(_lib.VBQError, match="file 0"):
        q.decompress_latents_mapped_window(inside, Q_REGIONS[2])
    want = np.stack([z[r] for z, r in zip(full, Q_REGIONS)])
    got = q.decompress_latents_mapped_batch(files[:2] + [outside, files[3]], Q_REGIONS, return_np=True)
    assert np.array_equal(_bits(got), _bits(want))
    with pytest.raises(_lib.VBQError):
        q.decompress_latents(outside)
    # the channels that the damage does not touch still decode
    got = q.decompress_latents_mapped_window(inside, Q_REGIONS[2], channels=[2, 4])
    assert np.array_equal(_bits(got), _bits(want[2][..., [2, 4]]))


def test_the_plain_batch_call_still_refuses_a_lambda_map_file(world):
    q, files, full, direct = world
    with pytest.raises(ValueError, match=r"file 1 is a lambda-map file \(magic b'VBQm'\): it has a table per symbol"):
        q.decompress_latents_batch([files[1], files[0]], [Q_REGIONS[1], Q_REGIONS[0]])
    with pytest.raises(ValueError, match="file 0 is a lambda-map file"):
        q.decompress_latents_window(files[2], Q_REGIONS[2])
    got = q.decompress_latents_mapped_batch([files[1], files[0]], [Q_REGIONS[1], Q_REGIONS[0]], return_np=True)
    assert np.array_equal(_bits(got[0]), _bits(q.decompress_latents_window(files[1], Q_REGIONS[1])))
