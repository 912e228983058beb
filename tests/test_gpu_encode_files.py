"""Batch encode of latent files on the GPU: vbq_rans_encode_files_u16 against the C checker's segment encoder, slot by slot and
word by word -- untouched slots, status bits and the pack round trip included --, and the quantizer's
compress_latents_to_bytes_batch / compress_to_bytes_batch against the loop of one-file calls, bytes == bytes."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import adversarial_tables as AT  # noqa: E402
from oracle import c_oracle as CO
from vbq_amd import bitstream as bs

pytestmark = pytest.mark.gpu
N = 10
LAMBS = [2.0 ** -6, 2.0 ** -2, 2.0, 16.0]
WORD, SIZE = 0xABCD, 0xFFFFFFFF                                  # what the output buffers hold before a launch


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


# ---------------------------------------------------------------------------------------------------------------- kernel level
class Batch:
    """Synthetic indices and frequency tables (built as `Coded` of test_gpu_window.py builds them), one file per (rows, table),
    laid out by bitstream.encode_plan; the padding rows between files hold T - 1, which no check may ever see coded.  tight:
    the files of a table follow each other without padding rows and the whole array starts one element in, so that plane bases
    are no multiples of 8 symbols (descriptors of the test's own; segments and items stay the plan's).  adversarial: tables and
    draws that do not fit each other (adversarial_tables.mixed_model) instead of the fitted ones."""

    def __init__(self, rows, tables, n_tables, C_, seg, bits, seed, canon=False, tight=False, adversarial=False):
        from vbq_amd.coder import quantize_frequencies
        rng = np.random.default_rng(seed)
        T = 2 ** (bits + 1) - 1
        self.C, self.seg, self.bits, self.T, self.rows, self.tables = C_, seg, bits, T, rows, tables
        centre = rng.integers(T // 8, T - T // 8, (n_tables, C_))
        spread = np.array([0.3, 2.0, 25.0, 300.0])[rng.integers(0, 4, (n_tables, C_))] * T / 2047
        draw = lambda t, n: np.clip(np.rint(rng.normal(centre[t, :, None], spread[t, :, None], (C_, n))), 0, T - 1).astype(np.uint16)
        if adversarial:
            self.freq, draw = AT.mixed_model(n_tables, C_, bits, seed)
        else:
            self.freq = np.stack([quantize_frequencies(np.stack([np.bincount(r, minlength=T) for r in draw(t, 4000)]))
                                  for t in range(n_tables)])
        self.idx = [draw(t, n) for n, t in zip(rows, tables)]
        # pairs of ranks mapped to the first of each pair: not the identity
        self.canon = np.tile((np.arange(T) & ~1).astype(np.uint16), (C_, 1)) if canon else None
        self.plan = p = bs.encode_plan(rows, tables, seg, C_, n_tables)
        self.files = p.files.copy()
        if tight:
            group = [sum(n for n, t in zip(rows, tables) if t == g) for g in range(n_tables)]
            for f, (n, t) in enumerate(zip(rows, tables)):
                row0 = sum(m for m, u in zip(rows[:f], tables[:f]) if u == t)
                self.files[f, :2] = 1 + C_ * sum(group[:t]) + row0, group[t]
        flat = np.full(1 + C_ * p.n_rows, T - 1, np.uint16)
        for f, idx in enumerate(self.idx):
            base, stride, n = (int(v) for v in self.files[f, :3])
            for c in range(C_):
                flat[base + c * stride: base + c * stride + n] = idx[c]
        self.flat = flat
        self.d_idx, self.d_freq = torch.from_numpy(flat).cuda(), torch.from_numpy(self.freq).cuda()
        self.d_canon = None if self.canon is None else torch.from_numpy(self.canon).cuda()
        # the reference, once per file: the checker on the symbols the file codes
        coded = [i if self.canon is None else np.take_along_axis(self.canon, i.astype(np.int64), axis=1) for i in self.idx]
        self.want = [CO.rans_encode(i, self.freq[t], seg) for i, t in zip(coded, tables)]

    def run(self, files=None, items=None, extra=0):
        """One launch into buffers of M + extra slots filled with WORD / SIZE -> (words, sizes, status) on the host."""
        from vbq_amd import ops
        p = self.plan
        M = p.M + extra
        files = torch.from_numpy(self.files if files is None else np.ascontiguousarray(files, np.int64)).cuda()
        items = torch.from_numpy(p.items if items is None else np.ascontiguousarray(items, np.int32)).cuda()
        words = torch.from_numpy(np.full((M, self.seg + 2), WORD, np.uint16)).cuda()
        sizes = torch.from_numpy(np.full(M, SIZE, np.uint32)).cuda()
        words, sizes, status = ops.rans_encode_files(self.d_idx, files, items, self.d_freq, M, seg=self.seg, N=self.bits,
                                                     canon=self.d_canon, words=words, sizes=sizes)
        torch.cuda.synchronize()
        self.d_words, self.d_sizes = words, sizes
        return words.cpu().numpy(), sizes.cpu().numpy(), status.cpu().tolist()

    def check_file(self, f, words, sizes):
        """Every slot of file f: the checker's size, the checker's words below it and WORD above it."""
        p, (w_ref, s_ref) = self.plan, self.want[f]
        a, b = int(p.seg_base[f]), int(p.seg_base[f]) + self.C * int(p.nseg[f])
        got_s, got_w = sizes[a:b], words[a:b]
        assert np.array_equal(got_s, s_ref.reshape(-1)), (f, got_s, s_ref.reshape(-1))
        valid = np.arange(self.seg + 2)[None, :] < got_s.astype(np.int64)[:, None]
        assert np.array_equal(got_w[valid], w_ref.reshape(b - a, -1)[valid]), f
        assert np.all(got_w[~valid] == WORD), f

    def check_untouched(self, f, words, sizes):
        p = self.plan
        a, b = int(p.seg_base[f]), int(p.seg_base[f]) + self.C * int(p.nseg[f])
        assert np.all(sizes[a:b] == SIZE) and np.all(words[a:b] == WORD), f


KERNEL_CASES = {  # rows, tables, n_tables, C, seg, bits, canon
    # a segment shorter than 8, an exact one, a short last one; laid out tight: unaligned plane bases
    "rows-and-tables": ([1, 7, 64, 65, 200], [1, 0, 1, 0, 1], 2, 3, 64, N, False),
    # two blocks for one table; lanes of one block belong to different files
    "several-blocks": ([70 * 7, 7, 5, 1], [0, 0, 0, 0], 1, 2, 7, N, False),
    "four-bits": ([16, 40, 3, 33], [0, 1, 1, 0], 2, 5, 16, 4, False),
    # bases that are multiples of 8 and segments of 1024: the 16-byte loads
    "aligned-vector-path": ([1536, 1536], [0, 1], 2, 32, 1024, N, False),
    "canonical-map": ([1, 7, 64, 65, 200], [1, 0, 1, 0, 1], 2, 3, 64, N, True),
    # tables that do not fit the data: a spike, the ramp and half_ones across the files; files 1 and 3 hold frequency-1 symbols only
    "mismatched-tables": ([1, 7, 64, 65, 200], [1, 0, 2, 0, 1], 3, 3, 64, 7, False),
}


@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_kernel_words_and_sizes_equal_the_checker(case):
    rows, tables, n_tables, C_, seg, bits, canon = KERNEL_CASES[case]
    k = Batch(rows, tables, n_tables, C_, seg, bits, seed=len(case), canon=canon, tight=case == "rows-and-tables",
              adversarial=case == "mismatched-tables")
    p = k.plan
    if case == "mismatched-tables":
        assert [k.freq[t, 0].tobytes() for t in range(3)] == [r.tobytes() for r in (AT.spike(7, 0), AT.ramp(), AT.half_ones(7))]
        assert all(np.all(np.take_along_axis(k.freq[0], k.idx[f].astype(np.int64), axis=1) == 1) for f in (1, 3))
        assert np.all(k.want[3][1][:, 0] == 2 + (15 * 64) // 16)  # a full segment of them: 62 of at most 66 words
    if case == "several-blocks":
        assert p.items.shape[0] == 128 and {int(f) for f in p.items[64:128, 0]} == {0, 1, 2, 3, -1}
    if case == "aligned-vector-path":
        assert np.all(k.files[:, 0] % 8 == 0) and np.all(k.files[:, 1] % 8 == 0) and k.d_idx.data_ptr() % 16 == 0
    if case == "rows-and-tables":
        assert np.sum(k.files[:, 0] % 8 != 0) >= 3 and np.any(k.files[:, 1] % 8 != 0)
    words, sizes, st = k.run(extra=2)
    assert st == [0] * len(rows)
    for f in range(len(rows)):
        k.check_file(f, words, sizes)
    assert np.all(sizes[p.M:] == SIZE) and np.all(words[p.M:] == WORD)       # slots past the plan's
    # an item taken off the list: the slots of its segment keep what they held, in every channel
    f, g = (int(v) for v in p.items[p.items[:, 0] >= 0][-1])
    items = p.items.copy()
    items[np.flatnonzero((items[:, 0] == f) & (items[:, 1] == g))] = -1
    words, sizes, st = k.run(items=items)
    assert st == [0] * len(rows)
    for c in range(C_):
        slot = int(p.seg_base[f]) + c * int(p.nseg[f]) + g
        assert sizes[slot] == SIZE and np.all(words[slot] == WORD)
    for other in range(len(rows)):
        if other != f:
            k.check_file(other, words, sizes)


def test_pack_of_all_files_at_once_round_trips():
    from vbq_amd import _lib, ops
    from vbq_amd.coder import RansCodec
    rows, tables, n_tables, C_, seg, bits, _ = KERNEL_CASES["rows-and-tables"]
    k = Batch(rows, tables, n_tables, C_, seg, bits, seed=4)
    p = k.plan
    words, sizes, st = k.run()
    assert st == [0] * len(rows)
    payload = torch.empty(p.M * (seg + 2), dtype=torch.uint16, device="cuda")
    offsets = torch.empty(p.M, dtype=torch.int64, device="cuda")
    total = torch.empty(1, dtype=torch.uint64, device="cuda")
    _lib.check(_lib.lib().vbq_rans_pack_u16(ops._ptr(k.d_words), ops._ptr(k.d_sizes), 1, p.M * seg, seg, ops._ptr(payload),
                                            ops._ptr(offsets), ops._ptr(total), None), "vbq_rans_pack_u16")
    torch.cuda.synchronize()
    ends = np.cumsum(sizes.astype(np.int64))
    assert int(total.cpu().numpy().view(np.uint64)[0]) == int(ends[-1])
    for f, (n, t) in enumerate(zip(rows, tables)):
        a, b = int(p.seg_base[f]), int(p.seg_base[f]) + C_ * int(p.nseg[f])
        lo, hi = int(ends[a - 1]) if a else 0, int(ends[b - 1])
        d_sz = torch.from_numpy(sizes[a:b].astype(np.uint16)).cuda()
        got = RansCodec(k.freq[t], N=bits, segment=seg).decode_packed(payload[lo:hi].clone(), d_sz, n)
        assert np.array_equal(got.cpu().numpy(), k.idx[f]), f


def test_direct_c_call_flags_defective_descriptors_and_items():
    """One direct C-ABI call over four files of one table.  File 1 lists a segment id equal to its nseg (its only item), file 2
    names table n_tables, file 3's index range leaves n_idx: each gets status 128 and nothing of it is written; file 0 beside
    them is coded right with status 0.  A defect of the descriptor leaves the whole file unwritten whatever its items; a stray
    segment id refuses that item alone (include/vbq.h): beside the file's own segments it flags the file and they are still
    coded.  Last, an item that names a file outside [0, n_files): nothing is written for it, bit 7 lands in word 0."""
    from vbq_amd import _lib
    rows, C_, seg = [100, 100, 100, 100], 3, 64
    k = Batch(rows, [0, 0, 0, 0], 1, C_, seg, N, seed=9)
    p = k.plan
    p_ = lambda t: C.c_void_p(t.data_ptr())                                  # noqa: E731

    def call(files, items):
        files = torch.tensor(files, dtype=torch.int64, device="cuda")
        it = np.full((64, 2), -1, np.int32)
        it[:len(items)] = items
        it = torch.from_numpy(it).cuda()
        words = torch.from_numpy(np.full((p.M, seg + 2), WORD, np.uint16)).cuda()
        sizes = torch.from_numpy(np.full(p.M, SIZE, np.uint32)).cuda()
        st = torch.zeros(4, dtype=torch.uint32, device="cuda")
        r = _lib.lib().vbq_rans_encode_files_u16(p_(k.d_idx), k.d_idx.numel(), p_(files), 4, p_(it), 64, C_, seg, N, p_(k.d_freq), 1,
                                                 None, p_(words), p_(sizes), p.M, p_(st), None)
        torch.cuda.synchronize()
        assert r == 0, _lib.lib().vbq_last_error()
        return words.cpu().numpy(), sizes.cpu().numpy(), st.cpu().tolist()

    good = [[int(v) for v in row] for row in p.files]
    assert all(int(s) == 2 for s in p.nseg)
    every = [(f, g) for f in range(4) for g in range(2)]
    words, sizes, st = call(good, every)
    assert st == [0, 0, 0, 0]
    for f in range(4):
        k.check_file(f, words, sizes)
    bad = [list(r) for r in good]
    bad[2][4] = 1                                                 # table == n_tables
    bad[3][0] = k.d_idx.numel() - (C_ - 1) * bad[3][1] - 100 + 1  # the last channel's symbols end one past n_idx
    words, sizes, st = call(bad, [(0, 0), (0, 1), (1, 2), (2, 0), (2, 1), (3, 0), (3, 1)])
    assert st == [0, 128, 128, 128], st
    k.check_file(0, words, sizes)
    for f in (1, 2, 3):
        k.check_untouched(f, words, sizes)
    for field, value in ((0, -8), (0, 1 << 62), (1, -1), (1, 1 << 62), (2, 0), (2, 1 << 62), (3, -1), (3, p.M - 5), (3, 1 << 62),
                         (4, -1)):
        bad = [list(r) for r in good]
        bad[1][field] = value
        words, sizes, st = call(bad, every)
        assert st == [0, 128, 0, 0], (field, value, st)
        k.check_untouched(1, words, sizes)
        for f in (0, 2, 3):
            k.check_file(f, words, sizes)
    words, sizes, st = call(good, every + [(1, 2), (1, -1), (1, 1 << 30)])
    assert st == [0, 128, 0, 0], st
    for f in range(4):
        k.check_file(f, words, sizes)
    words, sizes, st = call(good, every + [(4, 0), (-2, 0), (1 << 30, 1)])
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
            h, _, start = bs.parse(w)
            first = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
            part = "header" if first < h.nbytes else "size block" if first < start else "payload"
            pytest.fail(f"file {f}: {len(g)} bytes against {len(w)}, first difference at byte {first} ({part})")


_BUILT = {}


def _built(C_):
    """A quantizer with C channels, five latents of different shapes and their one-file results: shared, never changed."""
    if C_ not in _BUILT:
        q, scale, rng = _gaussian_quantizer(C_, C_)
        shapes = [(1, 32, 48, C_), (2, 17, 23, C_), (1, 20, 30, C_), (1, 1, 1, C_), (5, C_)]
        lat = [_latents(rng, scale, s) for s in shapes]
        q.build_entropy_models_from_latents(lat[0][0].reshape(-1, C_), lat[0][1].reshape(-1, C_), LAMBS, add_n_smoothing=1,
                                            spread="logvar")
        _BUILT[C_] = (q, lat, {})
    return _BUILT[C_]


def _loop(C_, lambs, seg, which=None):
    """The one-file calls of latents `which` (default: all five, in order) at `lambs`, each made once."""
    q, lat, cache = _built(C_)
    out = []
    for f, lamb in zip(range(5) if which is None else which, lambs):
        if (f, lamb, seg) not in cache:
            cache[(f, lamb, seg)] = q.compress_latents_to_bytes(*lat[f], lamb, segment=seg)
        out.append(cache[(f, lamb, seg)])
    return out


MIXED = [LAMBS[1], LAMBS[3], LAMBS[0], LAMBS[3], LAMBS[1]]


@pytest.mark.parametrize("C_,seg", [(32, 64), (32, 1024), (256, 1024)])
def test_batch_equals_the_loop_of_one_file_calls(C_, seg):
    q, lat, _ = _built(C_)
    _same_files(q.compress_latents_to_bytes_batch(lat, MIXED, segment=seg), _loop(C_, MIXED, seg))
    if C_ != 32:
        return
    _same_files(q.compress_latents_to_bytes_batch(lat, LAMBS[2], segment=seg), _loop(C_, [LAMBS[2]] * 5, seg))    # one lambda
    _same_files(q.compress_latents_to_bytes_batch(lat[1:2], [LAMBS[0]], segment=seg), _loop(C_, [LAMBS[0]], seg, [1]))   # F = 1
    on_dev = [(torch.from_numpy(m).cuda(), torch.from_numpy(lv).cuda()) for m, lv in lat]
    _same_files(q.compress_latents_to_bytes_batch(on_dev, MIXED, segment=seg), _loop(C_, MIXED, seg))
    mixed_in = [on_dev[0], lat[1], (torch.from_numpy(lat[2][0]), lat[2][1]), lat[3], on_dev[4]]                     # host and device
    _same_files(q.compress_latents_to_bytes_batch(mixed_in, MIXED, segment=seg), _loop(C_, MIXED, seg))


def test_more_than_64_segments_of_one_table_across_files():
    q, scale, rng = _gaussian_quantizer(2, 2)
    lat = [_latents(rng, scale, (1, 1, 3, 2)) for _ in range(70)]
    m, lv = _latents(rng, scale, (400, 2))
    q.build_entropy_models_from_latents(m, lv, LAMBS[:2], add_n_smoothing=1, spread="logvar")
    want = [q.compress_latents_to_bytes(m_, lv_, LAMBS[1], segment=2) for m_, lv_ in lat]
    _same_files(q.compress_latents_to_bytes_batch(lat, LAMBS[1], segment=2), want)


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
    lat = []
    for shape in ((1, 40, 50, 2), (2, 7, 9, 2), (5, 2), (1, 40, 50, 2)):
        lat.append((rng.normal(0, 1.1, shape).astype(np.float32), (2 * rng.normal(-2, 0.7, shape)).astype(np.float32)))
    lambs = [0.01, 0.3, 4.0]
    q.build_entropy_models_from_latents(lat[0][0].reshape(-1, 2), lat[0][1].reshape(-1, 2), lambs, add_n_smoothing=1, spread="logvar")
    mixed = [lambs[2], lambs[0], lambs[1], lambs[0]]
    for seg in (64, 1024):
        want = [q.compress_latents_to_bytes(m, lv, lamb, segment=seg) for (m, lv), lamb in zip(lat, mixed)]
        _same_files(q.compress_latents_to_bytes_batch(lat, mixed, segment=seg), want)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_written_batch_reads_back_through_the_batch_decoder():
    C_ = 32
    q, lat, _ = _built(C_)
    rng = np.random.default_rng(77)
    same = [lat[0], (lat[0][0] + rng.standard_normal(lat[0][0].shape).astype(np.float32), lat[0][1]), lat[0]]
    lambs = [LAMBS[2], LAMBS[0], LAMBS[3]]
    files = q.compress_latents_to_bytes_batch(same, lambs, segment=64)
    got = q.decompress_latents_batch(files, return_np=True)
    want = np.stack([np.asarray(q.compress_latents(m, lv, [lamb])["Z_hat"][lamb]) for (m, lv), lamb in zip(same, lambs)])
    assert np.array_equal(_bits(got), _bits(want))


def test_compress_to_bytes_batch_encodes_every_image():
    C_ = 32
    q, lat, _ = _built(C_)

    class Stored:
        """A stand-in VAE: `encode(i)` returns the stored latents of image i."""
        def encode(self, i):
            return lat[i]
    order = [4, 0, 2]
    lambs = [LAMBS[0], LAMBS[2], LAMBS[0]]
    want = [q.compress_to_bytes(i, Stored(), lamb, segment=64) for i, lamb in zip(order, lambs)]
    _same_files(q.compress_to_bytes_batch(order, Stored(), lambs, segment=64), want)
