"""Batch encode of lambda-map files on the GPU: vbq_rans_map_encode_files_u16 / vbq_rans_map_sizes_files_u16 against the NumPy
coder of tests/mapped_reference.py, slot by slot and word by word -- untouched slots and status bits included --, against the
kernels that existed (vbq_rans_encode_files_u16, vbq_rans_map_encode_u16), and the quantizer's
compress_latents_to_bytes_mapped_batch / coded_nbytes_mapped_batch / compress_to_bytes_mapped_batch against the loop of one-file
calls, bytes == bytes."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import adversarial_tables as AT  # noqa: E402
import mapped_reference as MR  # noqa: E402
from vbq_amd import bitstream as bs  # noqa: E402

pytestmark = pytest.mark.gpu
N = 10
LAMBS = [2.0 ** -6, 2.0 ** -2, 2.0, 16.0]
WORD, SIZE = 0xABCD, 0xFFFFFFFF                                  # what the output buffers hold before a launch


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


# ---------------------------------------------------------------------------------------------------------------- kernel level
def fitted_tables(n_tables, C_, bits, seed):
    """(freq u16 [n_tables, C, T], draw(t, n) -> u16 [C, n]): rounded normals about random centres and their quantised histograms."""
    from vbq_amd.coder import quantize_frequencies
    rng = np.random.default_rng(seed)
    T = 2 ** (bits + 1) - 1
    centre = rng.integers(T // 8, T - T // 8, (n_tables, C_))
    spread = np.array([0.3, 2.0, 25.0, 300.0])[rng.integers(0, 4, (n_tables, C_))] * T / 2047
    draw = lambda t, n: np.clip(np.rint(rng.normal(centre[t, :, None], spread[t, :, None], (C_, n))), 0, T - 1).astype(np.uint16)
    freq = np.stack([quantize_frequencies(np.stack([np.bincount(r, minlength=T) for r in draw(t, 4000)])) for t in range(n_tables)])
    return freq, draw


class Batch:
    """One file per (rows, palette number), laid out by bitstream.mapped_encode_plan: file f has P_f index planes [P_f, C, n_f],
    plane p drawn for the table palettes[palette_of[f]][p], and a class map maps[f] u8 [n_f].  Everything between the files'
    symbols holds T - 1 and the class padding holds 255, which no check may ever see coded.  tight: the files of a palette
    follow each other without padding rows, the class bytes without padding bytes, and both arrays start one element in, so that
    plane and class bases are no multiples of 8 (descriptors of the test's own; segments and items stay the plan's).  The
    reference, once per file: mapped_reference.encode on the symbols the file codes."""

    def __init__(self, rows, palette_of, palettes, freq, planes, maps, seg, bits, canon=False, tight=False):
        self.rows, self.palette_of, self.palettes, self.freq, self.planes, self.maps = rows, palette_of, palettes, freq, planes, maps
        self.C, self.seg, self.bits, self.T = freq.shape[1], seg, bits, freq.shape[2]
        C_, T, F = self.C, self.T, len(rows)
        sizes = [len(p) for p in palettes]
        self.max_classes = max(sizes)
        self.plan = p = bs.mapped_encode_plan(rows, palette_of, sizes, seg, C_)
        self.files = p.files.copy()
        n_idx, n_cls = p.n_idx, p.n_cls
        if tight:
            group = [sum(n for n, g in zip(rows, palette_of) if g == h) for h in range(len(palettes))]
            gbase = np.cumsum([0] + [sizes[h] * C_ * group[h] for h in range(len(palettes))])
            for f, (n, g) in enumerate(zip(rows, palette_of)):
                row0 = sum(m for m, u in zip(rows[:f], palette_of[:f]) if u == g)
                self.files[f, :3] = 1 + gbase[g] + row0, group[g], C_ * group[g]
                self.files[f, 6] = 1 + sum(rows[:f])
            n_idx, n_cls = 1 + int(gbase[-1]), 1 + sum(rows)
        self.canon = np.tile((np.arange(T) & ~1).astype(np.uint16), (C_, 1)) if canon else None   # pairs of ranks -> the first
        flat, cls = np.full(n_idx, T - 1, np.uint16), np.full(n_cls, 255, np.uint8)
        for f in range(F):
            base, stride, plane, n = (int(v) for v in self.files[f, :4])
            for k in range(sizes[palette_of[f]]):
                for c in range(C_):
                    a = base + k * plane + c * stride
                    assert np.all(flat[a:a + n] == T - 1)                        # no two files share an index
                    flat[a:a + n] = planes[f][k, c]
            a = int(self.files[f, 6])
            assert np.all(cls[a:a + n] == 255)
            cls[a:a + n] = maps[f]
        self.pal_rows = np.full((len(palettes), 4), -1, np.int32)
        for g, pal in enumerate(palettes):
            self.pal_rows[g, :len(pal)] = pal
        self.d_idx, self.d_cls, self.d_freq = (torch.from_numpy(a).cuda() for a in (flat, cls, freq))
        self.d_canon = None if self.canon is None else torch.from_numpy(self.canon).cuda()
        self.want = [self.reference(f, maps[f]) for f in range(F)]

    def reference(self, f, cls):
        """(words [C, nseg, seg + 2], sizes [C, nseg]) of file f under the class map `cls` (every class < P)."""
        pal = list(self.palettes[self.palette_of[f]])
        idx = MR.select(self.planes[f], cls)
        if self.canon is not None:
            idx = np.take_along_axis(self.canon, idx.astype(np.int64), axis=1)
        return MR.encode(idx, cls, self.freq[pal], self.seg)

    def run(self, files=None, items=None, palettes=None, extra=0, max_classes=None):
        """One encode launch into buffers of M + extra slots filled with WORD / SIZE, and one sizes launch into another sizes
        buffer, which must come out the same -> (words, sizes, status) on the host."""
        from vbq_amd import ops
        p = self.plan
        M = p.M + extra
        files = torch.from_numpy(self.files if files is None else np.ascontiguousarray(files, np.int64)).cuda()
        items = torch.from_numpy(p.items if items is None else np.ascontiguousarray(items, np.int32)).cuda()
        pals = torch.from_numpy(self.pal_rows if palettes is None else np.ascontiguousarray(palettes, np.int32)).cuda()
        words = torch.from_numpy(np.full((M, self.seg + 2), WORD, np.uint16)).cuda()
        sizes = torch.from_numpy(np.full(M, SIZE, np.uint32)).cuda()
        sizes2 = sizes.clone()
        kw = dict(seg=self.seg, max_classes=self.max_classes if max_classes is None else max_classes, N=self.bits, canon=self.d_canon)
        words, sizes, status = ops.rans_map_encode_files(self.d_idx, self.d_cls, files, pals, items, self.d_freq, M, words=words,
                                                         sizes=sizes, **kw)
        sizes2, status2 = ops.rans_map_sizes_files(self.d_idx, self.d_cls, files, pals, items, self.d_freq, M, sizes=sizes2, **kw)
        torch.cuda.synchronize()
        assert torch.equal(sizes.view(torch.int32), sizes2.view(torch.int32))           # the sizes entry writes the same d_sizes
        assert torch.equal(status.view(torch.int32), status2.view(torch.int32))
        return words.cpu().numpy(), sizes.cpu().numpy(), status.cpu().tolist()

    def slots(self, f):
        p = self.plan
        return int(p.seg_base[f]), int(p.seg_base[f]) + self.C * int(p.nseg[f])

    def check_file(self, f, words, sizes, want=None):
        """Every slot of file f: the reference's size, the reference's words below it and WORD above it."""
        w_ref, s_ref = self.want[f] if want is None else want
        a, b = self.slots(f)
        got_s, got_w = sizes[a:b], words[a:b]
        assert np.array_equal(got_s, s_ref.reshape(-1)), (f, got_s, s_ref.reshape(-1))
        valid = np.arange(self.seg + 2)[None, :] < got_s.astype(np.int64)[:, None]
        assert np.array_equal(got_w[valid], w_ref.reshape(b - a, -1)[valid]), f
        assert np.all(got_w[~valid] == WORD), f

    def check_untouched(self, f, words, sizes):
        a, b = self.slots(f)
        assert np.all(sizes[a:b] == SIZE) and np.all(words[a:b] == WORD), f

    def check_all(self, words, sizes, st, skip=()):
        assert st == [0] * len(self.rows), st
        for f in range(len(self.rows)):
            if f not in skip:
                self.check_file(f, words, sizes)
        assert np.all(sizes[self.plan.M:] == SIZE) and np.all(words[self.plan.M:] == WORD)   # slots past the plan's


def map_of(P, n, k):
    """The k-th class map of mapped_reference.maps(P, n), cyclically: uniform per class, mid, checker, skip1 (P = 3)."""
    m = MR.maps(P, n)
    return m[sorted(m)[k % len(m)]]


def fitted_batch(rows, palette_of, palettes, n_tables, C_, seg, bits, seed, round_=0, maps=None, **kw):
    freq, draw = fitted_tables(n_tables, C_, bits, seed)
    planes = [np.stack([draw(t, n) for t in palettes[g]]) for n, g in zip(rows, palette_of)]
    if maps is None:
        maps = [map_of(len(palettes[g]), n, f + round_) for f, (n, g) in enumerate(zip(rows, palette_of))]
    return Batch(rows, palette_of, palettes, freq, planes, maps, seg, bits, **kw)


ROWS = [1, 7, 64, 65, 200]
# palette sizes 1..4; the same two tables at different class numbers in (0, 1) and (1, 0)
MIXED = dict(rows=ROWS, palette_of=[0, 1, 2, 3, 4], palettes=[(0, 1), (1, 0), (2,), (0, 1, 2, 3), (3, 1, 2)], n_tables=4, C_=3, seg=64)


def removed_item_leaves_its_slots(k):
    """An item taken off the list: the slots of its segment keep what they held, in every channel; the rest is coded."""
    p = k.plan
    f, g = (int(v) for v in p.items[p.items[:, 0] >= 0][-1])
    items = p.items.copy()
    items[np.flatnonzero((items[:, 0] == f) & (items[:, 1] == g))] = -1
    words, sizes, st = k.run(items=items)
    assert st == [0] * len(k.rows)
    for c in range(k.C):
        slot = int(p.seg_base[f]) + c * int(p.nseg[f]) + g
        assert sizes[slot] == SIZE and np.all(words[slot] == WORD)
    for other in range(len(k.rows)):
        if other != f:
            k.check_file(other, words, sizes)


@pytest.mark.parametrize("round_", range(6))
def test_mixed_palettes_equal_the_reference(round_):
    """Six rounds take every file through every map of its palette size: uniform per class, mid, checker, skip1."""
    k = fitted_batch(**MIXED, bits=N, seed=11, round_=round_, tight=True)
    assert np.sum(k.files[:, 0] % 8 != 0) >= 3 and np.any(k.files[:, 2] % 8 != 0) and np.sum(k.files[:, 6] % 8 != 0) >= 3
    assert sorted(len(p) for p in k.palettes) == [1, 2, 2, 3, 4]
    assert len({map_of(3, 200, 4 + r).tobytes() for r in range(6)}) == 6             # file 4: all six maps of P = 3
    k.check_all(*k.run(extra=2))
    if round_ == 0:
        removed_item_leaves_its_slots(k)


def test_several_blocks_of_one_palette():
    """More than 64 segments of one palette: two blocks, and the lanes of the second belong to different files."""
    k = fitted_batch([70 * 7, 7, 5, 1], [0, 0, 0, 0], [(1, 0, 2)], 3, 2, 7, N, seed=12, round_=0)
    p = k.plan
    assert p.items.shape[0] == 128 and {int(f) for f in p.items[64:128, 0]} == {0, 1, 2, 3, -1}
    assert len(set(k.maps[0].tolist())) == 3                      # (the checkerboard)
    k.check_all(*k.run(extra=2))
    removed_item_leaves_its_slots(k)


def test_four_bits():
    k = fitted_batch([16, 40, 3, 33], [0, 1, 1, 0], [(0, 1), (1, 2, 0)], 3, 5, 16, 4, seed=13, round_=3)
    k.check_all(*k.run(extra=2))


def test_aligned_bases_take_the_wide_loads():
    """Segments of 1024 at bases that are multiples of 8: classes by 8-byte loads and, over the runs of eight equal classes,
    symbols by 16-byte loads; the map is uniform over most runs of eight and mixed in some."""
    rows, pals = [1536, 1536], [(0, 1), (1, 2, 0)]
    maps = []
    for f, P in enumerate((2, 3)):
        m = (np.arange(1536) // 8 * (f + 3) // 5 % P).astype(np.uint8)       # constant over every aligned run of eight
        m[np.arange(5 + f, 1536, 37)] = (m[np.arange(5 + f, 1536, 37)] + 1) % P   # ... but for a symbol every 37
        maps.append(m)
    k = fitted_batch(rows, [0, 1], pals, 3, 8, 1024, N, seed=14, maps=maps)
    for f in range(2):
        runs = k.maps[f].reshape(-1, 8)
        mixed = np.any(runs != runs[:, :1], axis=1)
        assert 30 <= mixed.sum() <= 50 and len(set(runs[~mixed, 0].tolist())) == len(pals[f])
    assert np.all(k.files[:, [0, 1, 2, 6]] % 8 == 0) and k.d_idx.data_ptr() % 16 == 0 and k.d_cls.data_ptr() % 8 == 0
    k.check_all(*k.run(extra=2))


def test_canonical_map_that_is_not_the_identity():
    k = fitted_batch(**MIXED, bits=N, seed=15, round_=5, canon=True)
    assert not np.array_equal(k.canon[0], np.arange(k.T))
    assert any(np.any(pl & 1) for pl in k.planes)                 # odd ranks are coded as the even rank below them
    k.check_all(*k.run(extra=2))


def test_tables_that_do_not_fit_the_data():
    """The rows and draws of adversarial_tables.mapped_rows / mapped_planes: every class's row of every channel from another
    family, data kinds that cycle over (class, channel)."""
    bits, C_ = 7, 3
    table_rows = AT.mapped_rows(4, C_, bits)                     # [4, C, T]: one table per class number
    rows, palette_of, pals = [1, 7, 64, 65, 200], [0, 1, 0, 2, 1], [(0, 1), (3, 2, 1, 0), (2,)]
    planes = [AT.mapped_planes(table_rows[list(pals[g])], n, seed=f) for f, (n, g) in enumerate(zip(rows, palette_of))]
    maps = [AT.class_map(AT.MAPPED_MAPS[f % 2], len(pals[g]), n) for f, (n, g) in enumerate(zip(rows, palette_of))]
    k = Batch(rows, palette_of, pals, np.ascontiguousarray(table_rows), planes, maps, 64, bits)
    k.check_all(*k.run(extra=2))


def test_uniform_files_equal_the_plain_batch_encoder():
    """A file whose classes are all p: slot for slot what vbq_rans_encode_files_u16 writes with the table palette[p]."""
    from vbq_amd import ops
    rows, palette_of, pals = MIXED["rows"], MIXED["palette_of"], MIXED["palettes"]
    pick = [1, 0, 0, 3, 2]                                        # the class of every file
    maps = [np.full(n, p, np.uint8) for n, p in zip(rows, pick)]
    k = fitted_batch(**MIXED, bits=N, seed=16, maps=maps)
    words, sizes, st = k.run()
    k.check_all(words, sizes, st)
    tables = [pals[g][p] for g, p in zip(palette_of, pick)]
    e = bs.encode_plan(rows, tables, k.seg, k.C, 4)
    assert np.array_equal(e.seg_base, k.plan.seg_base) and e.M == k.plan.M
    files = e.files.copy()
    files[:, 0] = k.files[:, 0] + np.array(pick) * k.files[:, 2]  # plane p of the file
    files[:, 1] = k.files[:, 1]
    w2 = torch.from_numpy(np.full((e.M, k.seg + 2), WORD, np.uint16)).cuda()
    s2 = torch.from_numpy(np.full(e.M, SIZE, np.uint32)).cuda()
    w2, s2, st2 = ops.rans_encode_files(k.d_idx, torch.from_numpy(files).cuda(), torch.from_numpy(e.items).cuda(), k.d_freq, e.M,
                                        seg=k.seg, N=N, words=w2, sizes=s2)
    assert st2.cpu().tolist() == [0] * 5
    assert np.array_equal(s2.cpu().numpy(), sizes) and np.array_equal(w2.cpu().numpy(), words)


def test_one_file_equals_the_one_file_kernel():
    """One file: the output of vbq_rans_map_encode_u16 for the same planes, classes and palette."""
    from vbq_amd.coder import MappedRansCodec
    pal = (2, 0, 1)
    k = fitted_batch([333], [0], [pal], 3, 3, 64, N, seed=17, round_=0)
    assert len(set(k.maps[0].tolist())) == 3                      # (the checkerboard)
    words, sizes, st = k.run()
    k.check_all(words, sizes, st)
    codec = MappedRansCodec(k.freq[list(pal)], N=N, segment=64)
    w1, s1 = codec.encode(torch.from_numpy(k.planes[0]).cuda(), k.maps[0])
    w1, s1 = w1.cpu().numpy().reshape(-1, 66), s1.cpu().numpy().reshape(-1)
    assert np.array_equal(s1, sizes)
    valid = np.arange(66)[None, :] < sizes.astype(np.int64)[:, None]
    assert np.array_equal(w1[valid], words[valid])


def test_a_class_outside_the_palette_is_coded_as_class_0():
    rows, pals = [100, 100], [(1, 0)]
    maps = [map_of(2, 100, 0) for _ in rows]                      # the checkerboard
    k = fitted_batch(rows, [0, 0], pals, 2, 3, 64, N, seed=18, maps=maps)
    wild = k.maps[1].copy()
    wild[[0, 3, 50, 63, 64, 99]] = [2, 3, 255, 2, 128, 4]
    cls = k.d_cls.cpu().numpy()
    cls[int(k.files[1, 6]): int(k.files[1, 6]) + 100] = wild
    k.d_cls = torch.from_numpy(cls).cuda()
    words, sizes, st = k.run()
    assert st == [0, 0]
    k.check_file(0, words, sizes)
    k.check_file(1, words, sizes, want=k.reference(1, np.where(wild >= 2, 0, wild).astype(np.uint8)))
    assert not np.array_equal(k.want[1][0], k.reference(1, np.where(wild >= 2, 0, wild).astype(np.uint8))[0])


def test_defective_descriptors_and_items_one_at_a_time():
    """Four files of 100 rows (two segments each): files 0..2 of palette 0 in block 0, file 3 of palette 1 in block 1.  Every
    defect of a descriptor gives that file status 128 and nothing of it is written whatever its items; a defective item writes
    nothing itself; the other files come out right with status 0."""
    rows, C_, seg = [100, 100, 100, 100], 3, 64
    pals = [(0, 1), (1, 0)]
    k = fitted_batch(rows, [0, 0, 0, 1], pals, 3, C_, seg, N, seed=19, round_=5)
    p = k.plan
    n_idx, n_cls, n_tables = k.d_idx.numel(), k.d_cls.numel(), k.freq.shape[0]
    assert all(int(s) == 2 for s in p.nseg) and p.items.shape[0] == 128
    k.check_all(*k.run())
    good = k.files
    stride, plane = int(good[1, 1]), int(good[1, 2])
    # palettes 2..5 are defective rows; a file that names one is refused
    rows6 = np.array([[0, 1, -1, -1], [1, 0, -1, -1], [-1, 0, 1, -1], [0, n_tables, -1, -1], [0, -2, -1, -1], [0, 1, 2, -1]], np.int32)
    defects = [(5, 6), (5, -1), (5, 1 << 62),                     # the palette id
               (5, 2),                                            # a palette row starting -1
               (5, 3), (5, 4),                                    # a table id out of range
               (5, 5),                                            # more classes than max_classes = 2
               (3, 0), (3, -5), (3, 1 << 62),                     # n
               (2, n_idx), (2, -1), (2, 1 << 62),                 # plane 1 past n_idx
               (2, n_idx - int(good[1, 0]) - (C_ - 1) * stride - 100 + 1),          # ... by one symbol, in the last channel
               (0, -8), (0, 1 << 62), (1, -1), (1, 1 << 62),      # the index base and stride
               (6, n_cls - 100 + 1), (6, -1), (6, 1 << 62),       # the class range past n_cls
               (4, p.M - 5), (4, -1), (4, 1 << 62)]               # slots past M
    for field, value in defects:
        bad = good.copy()
        bad[1, field] = value
        words, sizes, st = k.run(files=bad, palettes=rows6)
        assert st == [0, 128, 0, 0], (field, value, st)
        k.check_untouched(1, words, sizes)
        for f in (0, 2, 3):
            k.check_file(f, words, sizes)
    # the largest plane stride that fits is taken (the check is exact): plane 1 then ends at n_idx
    fits = good.copy()
    fits[1, 2] = n_idx - int(good[1, 0]) - (C_ - 1) * stride - 100
    words, sizes, st = k.run(files=fits, palettes=rows6)
    assert st == [0, 0, 0, 0]
    # a segment id outside the file: that item writes nothing and flags the file; the file's own segments are coded
    items = p.items.copy()
    pad = np.flatnonzero(items[:64, 0] < 0)
    items[pad[:3]] = [(1, 2), (1, -1), (1, 1 << 30)]
    words, sizes, st = k.run(items=items)
    assert st == [0, 128, 0, 0], st
    for f in range(4):
        k.check_file(f, words, sizes)
    # an item in a block of another palette: segment 0 of file 3 moved into block 0
    items = p.items.copy()
    at = np.flatnonzero((items[:, 0] == 3) & (items[:, 1] == 0))
    items[at] = -1
    items[pad[0]] = (3, 0)
    words, sizes, st = k.run(items=items)
    assert st == [0, 0, 0, 128], st
    for f in range(3):
        k.check_file(f, words, sizes)
    a, _ = k.slots(3)
    for c in range(C_):
        assert sizes[a + 2 * c] == SIZE and np.all(words[a + 2 * c] == WORD)
        assert sizes[a + 2 * c + 1] == k.want[3][1][c, 1]
    # a file id outside [0, n_files): nothing is written for it, bit 7 lands in word 0
    items = p.items.copy()
    items[pad[:3]] = [(4, 0), (-2, 0), (1 << 30, 1)]
    words, sizes, st = k.run(items=items)
    assert st == [128, 0, 0, 0], st
    for f in range(4):
        k.check_file(f, words, sizes)


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


def _same_files(got, want):
    """bytes == bytes, file by file; where they differ, say in which part of the file."""
    assert isinstance(got, list) and len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, bytes)
        if g != w:
            h, _, _, start = bs.parse_mapped(w)
            first = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
            part = "header" if first < h.nbytes else "class block" if first < h.sizes_offset else "size block" if first < start \
                else "payload"
            pytest.fail(f"file {f}: {len(g)} bytes against {len(w)}, first difference at byte {first} ({part})")


def _class_map(shape, P, kind, rng):
    """Classes shaped like the latents without the channel axis: bands along the rows, or one class per position at random."""
    B = int(np.prod(shape[:-1]))
    if kind == "bands":
        m = (np.arange(B) * P // max(B, 1)).astype(np.int64)
    else:
        m = rng.integers(0, P, B)
    return m.reshape(shape[:-1])


_BUILT = {}
SHAPES = lambda C_: [(1, 12, 20, C_), (2, 9, 11, C_), (1, 1, 1, C_), (5, C_), (300, C_)]          # noqa: E731


def _built(C_):
    """A quantizer with C channels and five latents of different shapes and ranks: shared, never changed."""
    if C_ not in _BUILT:
        q, scale, rng = _gaussian_quantizer(C_, C_)
        lat = [_latents(rng, scale, s) for s in SHAPES(C_)]
        q.build_entropy_models_from_latents(lat[0][0].reshape(-1, C_), lat[0][1].reshape(-1, C_), LAMBS, add_n_smoothing=1,
                                            spread="logvar")
        _BUILT[C_] = (q, lat)
    return _BUILT[C_]


A, B_, C3, D = LAMBS
PALETTES = [(A, B_), (B_, A), (A, B_), (C3,), (D, A, C3, B_)]    # repeats, a reversed order, P = 1 and P = 4


def _maps(C_, palettes, seed):
    rng = np.random.default_rng(seed)
    return [_class_map(s, len(p), ("bands", "random")[f % 2], rng) for f, (s, p) in enumerate(zip(SHAPES(C_), palettes))]


def _loop(q, lat, palettes, maps, seg):
    return [q.compress_latents_to_bytes_mapped(m, lv, list(p), cl, segment=seg) for (m, lv), p, cl in zip(lat, palettes, maps)]


@pytest.mark.parametrize("C_,seg", [(8, 64), (8, 1024), (256, 1024)])
def test_batch_equals_the_loop_of_one_file_calls(C_, seg):
    q, lat = _built(C_)
    maps = _maps(C_, PALETTES, seed=seg)
    want = _loop(q, lat, PALETTES, maps, seg)
    got = q.compress_latents_to_bytes_mapped_batch(lat, PALETTES, maps, segment=seg)
    _same_files(got, want)
    assert q.coded_nbytes_mapped_batch(lat, PALETTES, maps, segment=seg) == [len(w) for w in want]
    if C_ != 8:
        return
    on_dev = [(torch.from_numpy(m).cuda(), torch.from_numpy(lv).cuda()) for m, lv in lat]
    _same_files(q.compress_latents_to_bytes_mapped_batch(on_dev, PALETTES, maps, segment=seg), want)
    mixed_in = [on_dev[0], lat[1], (torch.from_numpy(lat[2][0]), lat[2][1]), lat[3], on_dev[4]]            # host and device
    _same_files(q.compress_latents_to_bytes_mapped_batch(mixed_in, PALETTES, [torch.from_numpy(m) for m in maps], segment=seg), want)
    for one in ((B_, D), (C3,), (D, C3, B_)):                     # one palette for all files; P = 1
        maps1 = _maps(C_, [one] * 5, seed=len(one))
        want1 = _loop(q, lat, [one] * 5, maps1, seg)
        _same_files(q.compress_latents_to_bytes_mapped_batch(lat, list(one), maps1, segment=seg), want1)
        assert q.coded_nbytes_mapped_batch(on_dev, list(one), maps1, segment=seg) == [len(w) for w in want1]
    _same_files(q.compress_latents_to_bytes_mapped_batch(lat[1:2], [PALETTES[1]], maps[1:2], segment=seg), want[1:2])   # F = 1


def test_more_than_64_segments_of_one_palette_across_files():
    q, scale, rng = _gaussian_quantizer(2, 2)
    lat = [_latents(rng, scale, (1, 1, 3, 2)) for _ in range(70)]
    m, lv = _latents(rng, scale, (400, 2))
    q.build_entropy_models_from_latents(m, lv, LAMBS[:2], add_n_smoothing=1, spread="logvar")
    maps = [rng.integers(0, 2, (1, 1, 3)) for _ in range(70)]
    pal = [LAMBS[1], LAMBS[0]]
    want = [q.compress_latents_to_bytes_mapped(m_, lv_, pal, cl, segment=2) for (m_, lv_), cl in zip(lat, maps)]
    _same_files(q.compress_latents_to_bytes_mapped_batch(lat, pal, maps, segment=2), want)
    assert q.coded_nbytes_mapped_batch(lat, pal, maps, segment=2) == [len(w) for w in want]


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
    shapes = ((1, 20, 25, 2), (2, 7, 9, 2), (5, 2), (1, 20, 25, 2))
    lat = [(rng.normal(0, 1.1, s).astype(np.float32), (2 * rng.normal(-2, 0.7, s)).astype(np.float32)) for s in shapes]
    lambs = [0.01, 0.3, 4.0]
    q.build_entropy_models_from_latents(lat[0][0].reshape(-1, 2), lat[0][1].reshape(-1, 2), lambs, add_n_smoothing=1, spread="logvar")
    pals = [(4.0, 0.01), (0.01, 4.0), (0.3,), (0.3, 0.01, 4.0)]
    maps = [_class_map(s, len(p), ("random", "bands")[f % 2], rng) for f, (s, p) in enumerate(zip(shapes, pals))]
    for seg in (64, 1024):
        want = _loop(q, lat, pals, maps, seg)
        _same_files(q.compress_latents_to_bytes_mapped_batch(lat, pals, maps, segment=seg), want)
        assert q.coded_nbytes_mapped_batch(lat, pals, maps, segment=seg) == [len(w) for w in want]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_written_batch_reads_back_through_the_batch_decoder():
    C_ = 8
    q, lat = _built(C_)
    rng = np.random.default_rng(77)
    same = [lat[0], (lat[0][0] + rng.standard_normal(lat[0][0].shape).astype(np.float32), lat[0][1]), lat[0]]
    pals = [(C3, A), (A, C3), (D, B_, A)]
    maps = [_class_map(lat[0][0].shape, len(p), ("bands", "random", "random")[f], rng) for f, p in enumerate(pals)]
    files = q.compress_latents_to_bytes_mapped_batch(same, pals, maps, segment=64)
    got = q.decompress_latents_mapped_batch(files, return_np=True)
    one = np.stack([q.decompress_latents(d) for d in files])
    want = np.stack([np.asarray(q.compress_latents_mapped(m, lv, list(p), cl)["Z_hat"]) for (m, lv), p, cl in zip(same, pals, maps)])
    assert np.array_equal(_bits(got), _bits(one)) and np.array_equal(_bits(got), _bits(want))


def test_compress_to_bytes_mapped_batch_encodes_every_image():
    C_ = 8
    q, lat = _built(C_)

    class Stored:
        """A stand-in VAE: `encode(i)` returns the stored latents of image i."""
        def encode(self, i):
            return lat[i]
    order = [4, 0, 2]
    pals = [(A, D), (D, A), (A, D)]
    maps = [_class_map(SHAPES(C_)[i], 2, "random", np.random.default_rng(i)) for i in order]
    want = [q.compress_to_bytes_mapped(i, Stored(), list(p), cl, segment=64) for i, p, cl in zip(order, pals, maps)]
    _same_files(q.compress_to_bytes_mapped_batch(order, Stored(), pals, maps, segment=64), want)
