"""Byte budgets over lambda maps on the GPU: vbq_rans_map_rates_files_u16 against the NumPy coder of tests/mapped_reference.py,
every one of the F x K totals for equality -- status bits included -- and against the per-palette sums of
vbq_rans_map_sizes_files_u16; then the quantizer's coded_nbytes_mapped_palettes_batch / compress_latents_to_budget_mapped_batch
/ compress_latents_to_total_budget_mapped and their one-file and image forms against the loop of one-file calls, bytes ==
bytes."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import adversarial_tables as AT  # noqa: E402
import mapped_reference as MR  # noqa: E402
from vbq_amd import bitstream as bs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


# ---------------------------------------------------------------------------------------------------------------- kernel level
C, SEG = 3, 16
# 80 segments of 16: two blocks, the second padded; heads and tails on both sides of the 8-byte class alignment and of the
# 16-byte symbol alignment
ROWS = [1, 7, 8, 9, 16, 17, 63, 64, 65, 130, 200, 600]
BASE = 7                                                         # what every total holds before a launch: the kernel adds
VICTIM = 5                                                       # the file the status cases damage: 17 rows, two segments


def fitted_tables(L, bits, seed):
    """(freq u16 [L, C, T], draw(t, n) -> u16 [C, n]): rounded normals about random centres and their quantised histograms."""
    from vbq_amd.coder import quantize_frequencies
    rng = np.random.default_rng(seed)
    T = 2 ** (bits + 1) - 1
    centre = rng.integers(T // 8, T - T // 8, (L, C))
    spread = np.array([0.02, 0.06, 0.15, 0.4])[rng.integers(0, 4, (L, C))] * T     # (wide for a small table: words to count)
    draw = lambda t, n: np.clip(np.rint(rng.normal(centre[t, :, None], spread[t, :, None], (C, n))), 0, T - 1).astype(np.uint16)
    freq = np.stack([quantize_frequencies(np.stack([np.bincount(r, minlength=T) for r in draw(t, 4000)])) for t in range(L)])
    return freq, draw


def class_maps(P, rows, round_=0):
    """One map per file, the kinds cycling over the files: uniform per class, a change in the middle, bands, checkerboard."""
    out = []
    for f, n in enumerate(rows):
        kind = (f + round_) % (P + 3)
        i = np.arange(n)
        m = np.full(n, kind, np.int64) if kind < P else np.where(i < n // 2 + 3, 0, P - 1) if kind == P else \
            i * P // n if kind == P + 1 else i % P
        out.append(m.astype(np.uint8))
    return out


class Rates:
    """F files under K candidates over L lambda planes.  File f has the planes planes[f] u16 [L, C, n_f] -- plane t drawn for
    table t -- and the class map maps[f] u8 [n_f]; plane t of all files is d_idx[t * stride_l : (t + 1) * stride_l], laid out by
    bitstream.mapped_encode_plan with every file in one palette group.  Everything between the files' symbols holds T - 1 and
    the class padding holds 255, which no check may ever see coded.  tight: the files follow each other without padding rows,
    the class bytes without padding bytes, and every plane and the class bytes start one element in, so that bases are no
    multiples of 8 (descriptors of the test's own; items stay the plan's).  The reference, once per (candidate, file): the sum
    of mapped_reference.sizes over the symbols the file codes under that candidate."""

    def __init__(self, rows, freq, planes, maps, cands, seg, bits, canon=False, tight=False):
        self.rows, self.freq, self.planes, self.maps, self.cands, self.seg, self.bits = rows, freq, planes, maps, cands, seg, bits
        self.L, self.T, F = freq.shape[0], freq.shape[2], len(rows)
        T = self.T
        self.plan = p = bs.mapped_encode_plan(rows, [0] * F, [1], seg, C)
        self.files = p.files.copy()
        R, n_cls, lead = p.n_rows, p.n_cls, 0
        if tight:
            R, lead = sum(rows), 1
            for f in range(F):
                self.files[f, 0] = self.files[f, 6] = 1 + sum(rows[:f])
            self.files[:, 1] = R
            n_cls = 1 + R
        self.stride_l = lead + C * R
        self.canon = np.tile((np.arange(T) & ~1).astype(np.uint16), (C, 1)) if canon else None    # pairs of ranks -> the first
        flat, cls = np.full(self.L * self.stride_l, T - 1, np.uint16), np.full(n_cls, 255, np.uint8)
        for f, n in enumerate(rows):
            base, stride = int(self.files[f, 0]), int(self.files[f, 1])
            for t in range(self.L):
                for c in range(C):
                    a = t * self.stride_l + base + c * stride
                    assert np.all(flat[a:a + n] == T - 1)                            # no two files share an index
                    flat[a:a + n] = planes[f][t, c]
            a = int(self.files[f, 6])
            assert np.all(cls[a:a + n] == 255)
            cls[a:a + n] = maps[f]
        self.flat, self.cls = flat, cls
        self.d_idx, self.d_cls, self.d_freq = (torch.from_numpy(a).cuda() for a in (flat, cls, freq))
        self.d_canon = None if self.canon is None else torch.from_numpy(self.canon).cuda()
        self.want = np.array([[self.reference(f, cand, maps[f]) for f in range(F)] for cand in cands], np.int64)   # [K, F]

    def reference(self, f, cand, cls, planes=None):
        """The words of file f under `cand` and the class map `cls` (every class < P), all segments of all channels."""
        planes = self.planes[f] if planes is None else planes
        idx = MR.select(planes[list(cand)], cls)
        if self.canon is not None:
            idx = np.take_along_axis(self.canon, idx.astype(np.int64), axis=1)
        return int(MR.sizes(idx, cls, self.freq[list(cand)], self.seg).sum())

    def rows4(self, cands=None):
        out = np.full((len(self.cands if cands is None else cands), 4), -1, np.int32)
        for k, cand in enumerate(self.cands if cands is None else cands):
            out[k, :len(cand)] = cand
        return out

    def run(self, files=None, items=None, rows4=None, max_classes=None, status=True):
        """One launch on totals that hold BASE -> (what it added int64 [K, F], status list)."""
        from vbq_amd import ops
        rows4 = self.rows4() if rows4 is None else np.ascontiguousarray(rows4, np.int32)
        K, F = rows4.shape[0], len(self.rows)
        files = torch.from_numpy(self.files if files is None else np.ascontiguousarray(files, np.int64)).cuda()
        items = torch.from_numpy(self.plan.items if items is None else np.ascontiguousarray(items, np.int32)).cuda()
        totals = torch.full((K, F), BASE, dtype=torch.int64, device="cuda").view(torch.uint64)
        totals, st = ops.rans_map_rates_files(self.d_idx, self.d_cls, files, torch.from_numpy(rows4).cuda(), items, self.d_freq,
                                              lambda_stride=self.stride_l, seg=self.seg,
                                              max_classes=max(len(c) for c in self.cands) if max_classes is None else max_classes,
                                              N=self.bits, canon=self.d_canon, totals=totals)
        torch.cuda.synchronize()
        return totals.view(torch.int64).cpu().numpy() - BASE, st.cpu().tolist()

    def check(self):
        got, st = self.run()
        assert st == [0] * len(self.rows), st
        assert np.array_equal(got, self.want), (got, self.want)
        return got

    def sums_of_the_sizes_kernel(self, cand):
        """The per-file sums of vbq_rans_map_sizes_files_u16 with the palette `cand`: its planes gathered next to each other."""
        from vbq_amd import ops
        p, P = self.plan, len(cand)
        idx = np.ascontiguousarray(self.flat.reshape(self.L, self.stride_l)[list(cand)]).reshape(-1)
        files = self.files.copy()
        files[:, 2] = self.stride_l                               # plane p of the palette
        pal = np.array([[0, 1, 2, 3][:P] + [-1] * (4 - P)], np.int32)
        freq = np.ascontiguousarray(self.freq[list(cand)])
        sizes, st = ops.rans_map_sizes_files(torch.from_numpy(idx).cuda(), self.d_cls, torch.from_numpy(files).cuda(),
                                             torch.from_numpy(pal).cuda(), torch.from_numpy(p.items).cuda(),
                                             torch.from_numpy(freq).cuda(), p.M, seg=self.seg, max_classes=P, N=self.bits,
                                             canon=self.d_canon)
        assert st.cpu().tolist() == [0] * len(self.rows)
        s = sizes.cpu().numpy().astype(np.int64)
        return [int(s[int(p.seg_base[f]): int(p.seg_base[f]) + C * int(p.nseg[f])].sum()) for f in range(len(self.rows))]


def fitted(cands, L, bits=4, seg=SEG, seed=0, rows=ROWS, maps=None, round_=0, **kw):
    freq, draw = fitted_tables(L, bits, seed)
    planes = [np.stack([draw(t, n) for t in range(L)]) for n in rows]
    P = len(cands[0])
    return Rates(rows, freq, planes, class_maps(P, rows, round_) if maps is None else maps, cands, seg, bits, **kw)


# candidates that share tables, (a, b) next to (b, a), a ladder step
SIX = {1: [(0,), (3,), (1,), (3,), (4,), (2,)],
       2: [(0, 1), (1, 0), (1, 2), (2, 3), (4, 0), (3, 4)],
       3: [(0, 1, 2), (2, 1, 0), (1, 2, 3), (2, 3, 4), (4, 0, 2), (0, 3, 1)],
       4: [(0, 1, 2, 3), (3, 2, 1, 0), (1, 2, 3, 4), (4, 0, 1, 2), (2, 4, 0, 3), (0, 2, 4, 1)]}


def test_the_shared_shapes_are_the_ones_the_kernel_can_go_wrong_at():
    p = bs.mapped_encode_plan(ROWS, [0] * len(ROWS), [1], SEG, C)
    assert int(p.nseg.sum()) == 80 and p.items.shape[0] == 128 and int((p.items[:, 0] < 0).sum()) == 48
    assert {int(f) for f in p.items[64:128, 0]} == {11, -1}       # the second block: one file's segments and padding


@pytest.mark.parametrize("P", [1, 2, 3, 4])
@pytest.mark.parametrize("K", [1, 6])
def test_totals_equal_the_reference(P, K):
    k = fitted(SIX[P][:K], 5, seed=10 * P + K, round_=P + K, tight=True)
    assert np.sum(k.files[:, 0] % 8 != 0) >= 6 and np.sum(k.files[:, 6] % 8 != 0) >= 6 and k.stride_l % 8 != 0
    k.check()


def test_every_row_equals_the_sums_of_the_sizes_kernel():
    """Each candidate's row is the per-file sum of what vbq_rans_map_sizes_files_u16 writes with that palette; (a, b) and
    (b, a) differ."""
    k = fitted(SIX[2], 5, seed=21, tight=True)
    got = k.check()
    for j, cand in enumerate(k.cands):
        assert k.sums_of_the_sizes_kernel(cand) == got[j].tolist(), cand
    assert not np.array_equal(got[0], got[1])
    k3 = fitted(SIX[3][:2], 5, seed=22, round_=3)
    got = k3.check()
    for j, cand in enumerate(k3.cands):
        assert k3.sums_of_the_sizes_kernel(cand) == got[j].tolist(), cand


def test_uniform_maps_on_aligned_bases_take_the_wide_loads():
    """The plan's own layout: bases that are multiples of 8, and maps that are one class per file, so that every aligned run of
    eight classes agrees and its symbols come by one 16-byte load."""
    maps = [np.full(n, f % 2, np.uint8) for f, n in enumerate(ROWS)]
    k = fitted(SIX[2], 5, seed=23, maps=maps)
    assert np.all(k.files[:, [0, 1, 6]] % 8 == 0) and k.stride_l % 8 == 0
    assert k.d_idx.data_ptr() % 16 == 0 and k.d_cls.data_ptr() % 8 == 0
    k.check()
    # runs of eight that agree next to runs that do not
    maps = [((np.arange(n) // 8 * 3 // 5 + (np.arange(n) % 37 == 5)) % 2).astype(np.uint8) for n in ROWS]
    fitted(SIX[2][:3], 5, seed=24, maps=maps).check()


def test_banded_and_checkerboard_maps():
    for P in (2, 4):
        bands = [(np.arange(n) * P // n).astype(np.uint8) for n in ROWS]
        checker = [((np.arange(n) + f) % P).astype(np.uint8) for f, n in enumerate(ROWS)]
        fitted(SIX[P][:3], 5, seed=25 + P, maps=bands, tight=True).check()
        fitted(SIX[P][:3], 5, seed=26 + P, maps=checker, tight=True).check()


def test_canonical_map_that_is_not_the_identity():
    k = fitted(SIX[3][:4], 5, seed=27, canon=True, tight=True)
    assert not np.array_equal(k.canon[0], np.arange(k.T)) and any(np.any(pl & 1) for pl in k.planes)
    k.check()


def test_ten_bits():
    fitted(SIX[2][:3], 5, bits=10, seed=28, tight=True).check()


def test_segments_of_64():
    k = fitted(SIX[4][:2], 5, seg=64, seed=29, tight=True)
    assert k.plan.items.shape[0] == 64 and int(k.plan.nseg[-1]) == 10
    k.check()


def test_tables_that_do_not_fit_the_data():
    """The rows and draws of adversarial_tables.mapped_rows / mapped_planes: every lambda's row of every channel from another
    family, data kinds that cycle over (lambda, channel)."""
    bits = 7
    table_rows = np.ascontiguousarray(AT.mapped_rows(4, C, bits))
    rows = [1, 7, 64, 65, 200]
    planes = [AT.mapped_planes(table_rows, n, seed=f) for f, n in enumerate(rows)]
    maps = [AT.class_map(AT.MAPPED_MAPS[f % 2], 2, n) for f, n in enumerate(rows)]
    Rates(rows, table_rows, planes, maps, [(0, 1), (1, 0), (3, 2), (2, 0)], 64, bits).check()


def test_a_class_outside_the_palette_is_coded_as_class_0():
    k = fitted(SIX[2][:3], 5, seed=30, tight=True)
    f = 9                                                         # 130 rows
    wild = k.maps[f].copy()
    wild[[0, 3, 50, 63, 64, 129]] = [2, 3, 255, 2, 128, 4]
    wild[72:80] = 7                                               # a whole run of eight
    cls = k.cls.copy()
    cls[int(k.files[f, 6]): int(k.files[f, 6]) + 130] = wild
    k.d_cls = torch.from_numpy(cls).cuda()
    got, st = k.run()
    want = k.want.copy()
    tamed = np.where(wild >= 2, 0, wild).astype(np.uint8)
    want[:, f] = [k.reference(f, cand, tamed) for cand in k.cands]
    assert not np.array_equal(want, k.want)
    assert st == [0] * len(ROWS) and np.array_equal(got, want)


def test_an_index_outside_the_table_is_coded_as_symbol_0():
    k = fitted(SIX[2][:3], 5, seed=31, tight=True)
    f, T = 8, k.T                                                 # 65 rows
    flat, planes = k.flat.copy(), k.planes[f].copy()
    for t, c, i, v in [(0, 0, 0, T), (1, 2, 64, 65535), (2, 1, 17, T + 5), (1, 0, 33, 2 * T), (0, 2, 40, 1 << 15)]:
        flat[t * k.stride_l + int(k.files[f, 0]) + c * int(k.files[f, 1]) + i] = v
        planes[t, c, i] = 0
    k.d_idx = torch.from_numpy(flat).cuda()
    got, st = k.run()
    want = k.want.copy()
    want[:, f] = [k.reference(f, cand, k.maps[f], planes=planes) for cand in k.cands]
    assert st == [0] * len(ROWS) and np.array_equal(got, want)


def test_fields_the_kernel_does_not_read():
    k = fitted(SIX[2][:2], 5, seed=32, tight=True)
    files = k.files.copy()
    files[:, 2], files[:, 4], files[:, 5], files[:, 7] = -1, 1 << 62, 99, -7       # plane_stride, seg_base, palette, reserved
    got, st = k.run(files=files)
    assert st == [0] * len(ROWS) and np.array_equal(got, k.want)


def test_defective_descriptors_items_and_candidates_one_at_a_time():
    """Every defect of a descriptor gives that file status 128 and nothing of it is added, under any candidate; a defective
    item adds nothing itself; a defective candidate adds nothing to its row and flags every listed file; everything else comes
    out right."""
    k = fitted(SIX[2][:3], 5, seed=33, tight=True)
    p, F, v = k.plan, len(ROWS), VICTIM
    n_idx, n_cls, L = k.d_idx.numel(), k.d_cls.numel(), k.L
    good = k.files
    n, base, stride = (int(good[v, j]) for j in (3, 0, 1))
    room = n_idx - (L - 1) * k.stride_l                          # what a file may span: its last plane ends at n_idx
    assert base + (C - 1) * stride + n < room                    # (files follow the victim)
    none = k.want.copy()
    none[:, v] = 0
    flagged = [128 if f == v else 0 for f in range(F)]
    defects = [(3, 0), (3, -5), (3, 1 << 62),                     # n
               (0, -1), (0, 1 << 62), (0, room - (C - 1) * stride - n + 1),          # the index base: by one symbol
               (1, -1), (1, 1 << 62), (1, (room - n - base) // (C - 1) + 1),         # the channel stride: by one
               (6, n_cls - n + 1), (6, -1), (6, 1 << 62)]         # the class range past n_cls
    for field, value in defects:
        bad = good.copy()
        bad[v, field] = value
        got, st = k.run(files=bad)
        assert st == flagged, (field, value, st)
        assert np.array_equal(got, none), (field, value)
    # the largest stride and the largest class base that fit are taken: the checks are exact (the symbols read there are other
    # files' or guards, all inside the arrays)
    for field, value in [(1, (room - n - base) // (C - 1)), (6, n_cls - n)]:
        fits = good.copy()
        fits[v, field] = value
        got, st = k.run(files=fits)
        assert st == [0] * F, (field, st)
        assert np.array_equal(np.delete(got, v, axis=1), np.delete(k.want, v, axis=1))
    # a segment id outside the file: that item adds nothing and flags the file; the file's own segments are counted
    items = p.items.copy()
    pad = np.flatnonzero(items[:, 0] < 0)
    items[pad[:3]] = [(v, 2), (v, -1), (v, 1 << 30)]
    got, st = k.run(items=items)
    assert st == flagged and np.array_equal(got, k.want)
    # a file id outside [0, n_files): nothing is added for it, bit 7 lands in word 0
    items = p.items.copy()
    items[pad[:3]] = [(F, 0), (-2, 0), (1 << 30, 1)]
    got, st = k.run(items=items)
    assert st == [128] + [0] * (F - 1) and np.array_equal(got, k.want)
    # an item taken off the list is not counted
    items = p.items.copy()
    items[np.flatnonzero((items[:, 0] == v) & (items[:, 1] == 1))] = -1
    got, st = k.run(items=items)
    assert st == [0] * F
    assert np.array_equal(np.delete(got, v, axis=1), np.delete(k.want, v, axis=1)) and np.all(got[:, v] < k.want[:, v])
    # defective candidate rows: a first entry of -1, an entry outside [0, n_lambda), more classes than max_classes
    for row in ([-1, 0, 1, -1], [0, L, -1, -1], [0, -2, -1, -1], [L, 0, -1, -1], [0, 1, 2, -1]):
        rows4 = k.rows4()
        rows4[1] = row
        got, st = k.run(rows4=rows4, max_classes=2)
        assert st == [128] * F, (row, st)
        want = k.want.copy()
        want[1] = 0
        assert np.array_equal(got, want), row
    # what follows the first -1 is not read
    rows4 = k.rows4()
    rows4[:, 2:] = [-1, 1 << 30]
    got, st = k.run(rows4=rows4)
    assert st == [0] * F and np.array_equal(got, k.want)


# ------------------------------------------------------------------------------------------------------------- quantizer level
QC, QN = 4, 6
LAMBS = [2.0 ** -6, 2.0 ** -2, 2.0, 16.0]
A, B_, C3, D = LAMBS
# The first lambda falls and rises along the list, and so does the second: a file whose classes are all 0 has lengths that go
# large, small, medium, smallest; one whose classes are all 1 medium, largest, smallest, small.  Neither row is monotonic, and
# between them every column is somewhere the first to reach its length.
CANDS = [(A, B_), (C3, A), (B_, D), (D, C3)]
SHAPES = [(2, 9, 8, QC), (1, 12, 10, QC), (1, 3, 5, QC), (37, QC), (1, 1, 1, QC), (2, 9, 8, QC)]
SEGMENT = 16


def _class_maps():
    rng = np.random.default_rng(3)
    out = []
    for f, s in enumerate(SHAPES):
        n = int(np.prod(s[:-1]))
        m = np.zeros(n, np.int64) if f == 0 else np.ones(n, np.int64) if f == 1 else np.arange(n) * 2 // n if f == 2 else \
            rng.integers(0, 2, n)
        out.append(m.reshape(s[:-1]))
    return out


_BUILT = {}


def _built():
    """(quantizer, latents, class maps, want int64 [F, K]: the one-file lengths): shared, never changed."""
    if not _BUILT:
        from vbq_amd import ChannelwisePriorCDFQuantizer, priors
        rng = np.random.default_rng(QC)
        scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), QC))
        q = ChannelwisePriorCDFQuantizer(QC, QN)
        q.build_code_points(priors.FactoredGaussianPrior(np.zeros(QC), scale))
        lat = [((scale * rng.standard_normal(s)).astype(np.float32), (2 * (-2 + 0.7 * rng.standard_normal(s))).astype(np.float32))
               for s in SHAPES]
        q.build_entropy_models_from_latents(lat[0][0].reshape(-1, QC), lat[0][1].reshape(-1, QC), LAMBS, add_n_smoothing=1,
                                            spread="logvar")
        maps = _class_maps()
        want = np.array([[q.coded_nbytes_mapped(m, lv, list(cand), cl, segment=SEGMENT) for cand in CANDS]
                         for (m, lv), cl in zip(lat, maps)], np.int64)
        want.setflags(write=False)
        _BUILT["all"] = (q, lat, maps, want)
    return _BUILT["all"]


def _first_fit(want, budgets):
    """The rule, restated: per file the first column whose length is within the budget."""
    return [next(k for k in range(want.shape[1]) if want[f, k] <= budgets[f]) for f in range(want.shape[0])]


def _one_file(q, pair, cand, cl):
    return q.compress_latents_to_bytes_mapped(pair[0], pair[1], list(cand), cl, segment=SEGMENT)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _count_launches(monkeypatch):
    from vbq_amd import ops
    calls, real = [], ops.rans_map_rates_files
    monkeypatch.setattr(ops, "rans_map_rates_files", lambda *a, **kw: (calls.append(a[3].shape[0]), real(*a, **kw))[1])
    return calls


def test_lengths_equal_the_loop_of_one_file_calls(monkeypatch):
    q, lat, maps, want = _built()
    calls = _count_launches(monkeypatch)
    got = q.coded_nbytes_mapped_palettes_batch(lat, CANDS, maps, segment=SEGMENT)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want)
    assert calls == [len(CANDS)]                                  # one launch for all files and candidates
    on_dev = [(torch.from_numpy(m).cuda(), torch.from_numpy(lv).cuda()) for m, lv in lat]
    assert np.array_equal(q.coded_nbytes_mapped_palettes_batch(on_dev, CANDS, [torch.from_numpy(m) for m in maps], segment=SEGMENT), want)
    # the default segment, P = 1 and P = 4, repeated candidates
    for cands in ([(D,), (A,), (D,)], [(A, B_, C3, D), (D, C3, B_, A)]):
        cl = [np.asarray(m) * (len(cands[0]) - 1) for m in maps]
        ref = [[q.coded_nbytes_mapped(m, lv, list(cand), c) for cand in cands] for (m, lv), c in zip(lat, cl)]
        assert q.coded_nbytes_mapped_palettes_batch(lat, cands, cl).tolist() == ref
    # the one-file form
    assert q.coded_nbytes_mapped_palettes(lat[3][0], lat[3][1], CANDS, maps[3], segment=SEGMENT) == want[3].tolist()
    assert q.coded_nbytes_mapped_palettes_batch([], CANDS, []).shape == (0, len(CANDS))


def test_lengths_in_several_chunks_of_candidates(monkeypatch):
    """No room for more than one table per solve: every candidate is a chunk of its own, solved and sized by itself."""
    from vbq_amd import quantizer as qz
    q, lat, maps, want = _built()
    monkeypatch.setattr(qz, "RATE_SCRATCH_BYTES", 1)
    calls = _count_launches(monkeypatch)
    assert np.array_equal(q.coded_nbytes_mapped_palettes_batch(lat, CANDS, maps, segment=SEGMENT), want)
    assert calls == [1] * len(CANDS)


def test_budgets_pick_the_first_candidate_that_fits():
    q, lat, maps, want = _built()
    F, K = want.shape
    assert any(np.any(np.diff(row) > 0) and np.any(np.diff(row) < 0) for row in want)           # a row that is not monotonic
    # budgets from the reference table, so that every column is chosen: column k for a file where it is the first of its length
    first = np.array([[k == 0 or want[f, k] < want[f, :k].min() for k in range(K)] for f in range(F)])
    assert first.any(axis=0).all(), want
    pick, free = {}, list(range(F))
    for k in sorted(range(K), key=lambda k: first[:, k].sum()):   # the columns few files can choose go first
        f = next(f for f in free if first[f, k])
        pick[f] = k
        free.remove(f)
    for f in free:
        pick[f] = int(np.flatnonzero(first[f])[-1])
    budgets = [int(want[f, pick[f]]) for f in range(F)]
    assert _first_fit(want, budgets) == [pick[f] for f in range(F)] and set(pick.values()) == set(range(K))
    files = q.compress_latents_to_budget_mapped_batch(lat, budgets, CANDS, maps, segment=SEGMENT)
    assert isinstance(files, list) and len(files) == F
    for f in range(F):
        assert files[f] == _one_file(q, lat[f], CANDS[pick[f]], maps[f]), f
        assert len(files[f]) == want[f, pick[f]] and bs.parse_mapped(files[f])[0].lambs == CANDS[pick[f]]
        z = q.compress_latents_mapped(lat[f][0], lat[f][1], list(CANDS[pick[f]]), maps[f])["Z_hat"]
        assert np.array_equal(_bits(q.decompress_latents(files[f])), _bits(z)), f
    # one more byte changes nothing; budgets as a NumPy array
    assert q.compress_latents_to_budget_mapped_batch(lat, np.array(budgets) + 1, CANDS, maps, segment=SEGMENT) == files
    # one budget for all files
    for scalar in (int(want.min(axis=1).max()), int(want.max())):
        cols = _first_fit(want, [scalar] * F)
        got = q.compress_latents_to_budget_mapped_batch(lat, scalar, CANDS, maps, segment=SEGMENT)
        assert got == [_one_file(q, lat[f], CANDS[cols[f]], maps[f]) for f in range(F)]
    assert len(set(_first_fit(want, [int(want.min(axis=1).max())] * F))) > 1
    # the one-file form
    assert q.compress_latents_to_budget_mapped(lat[1][0], lat[1][1], budgets[1], CANDS, maps[1], segment=SEGMENT) == files[1]


def test_a_budget_nothing_fits_raises_before_anything_is_encoded(monkeypatch):
    from vbq_amd import ops
    q, lat, maps, want = _built()
    monkeypatch.setattr(ops, "rans_map_encode_files", lambda *a, **kw: pytest.fail("an encode launch"))
    budgets = [int(v) for v in want.max(axis=1)]
    budgets[2] = int(want[2].min()) - 1
    with pytest.raises(ValueError, match=f"file 2: no palette fits in {budgets[2]} bytes: the smallest file is {budgets[2] + 1} bytes"):
        q.compress_latents_to_budget_mapped_batch(lat, budgets, CANDS, maps, segment=SEGMENT)
    with pytest.raises(ValueError, match="file 0: no palette fits"):
        q.compress_latents_to_budget_mapped_batch(lat, int(want.min()) - 1, CANDS, maps, segment=SEGMENT)
    with pytest.raises(ValueError, match="file 0: no palette fits"):
        q.compress_latents_to_budget_mapped(lat[4][0], lat[4][1], int(want[4].min()) - 1, CANDS, maps[4], segment=SEGMENT)
    sums = want.sum(axis=0)
    with pytest.raises(ValueError, match=f"no palette fits in {int(sums.min()) - 1} bytes in total: the smallest total is "
                                         f"{int(sums.min())} bytes, at palette {int(np.argmin(sums))}"):
        q.compress_latents_to_total_budget_mapped(lat, int(sums.min()) - 1, CANDS, maps, segment=SEGMENT)
    assert q.compress_latents_to_budget_mapped_batch([], 5, CANDS, []) == []


def test_total_budget_against_the_column_sums():
    q, lat, maps, want = _built()
    sums = want.sum(axis=0)
    for budget in (int(sums[0]), int(sums.min()), int(sums.max()), int(sorted(sums)[1])):
        k_want = int(np.flatnonzero(sums <= budget)[0])           # the rule, restated: the first column that fits
        k, files = q.compress_latents_to_total_budget_mapped(lat, budget, CANDS, maps, segment=SEGMENT)
        assert k == k_want and sum(len(d) for d in files) == sums[k] <= budget
        assert files == [_one_file(q, lat[f], CANDS[k], maps[f]) for f in range(len(lat))]


def test_image_forms_encode_with_the_vae_first():
    q, lat, maps, want = _built()

    class Stored:
        """A stand-in VAE: `encode(i)` returns the stored latents of image i."""
        def encode(self, i):
            return lat[i]
    order = [3, 0, 2]
    budgets = [int(want[i, 1 + j % 2 * 2]) for j, i in enumerate(order)]
    cols = _first_fit(want[order], budgets)
    got = q.compress_to_budget_mapped_batch(order, Stored(), budgets, CANDS, [maps[i] for i in order], segment=SEGMENT)
    assert got == [_one_file(q, lat[i], CANDS[c], maps[i]) for i, c in zip(order, cols)]
    assert q.compress_to_budget_mapped(0, Stored(), budgets[1], CANDS, maps[0], segment=SEGMENT) == got[1]
