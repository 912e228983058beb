"""vbq_rans_il_rates_files_u16 on the GPU (include/vbq.h, "Compact batch") through ops.rans_il_rates_files against the NumPy
coder of tests/interleaved_reference.py: the part sizes of three files at three lambdas in one launch -- another index plane
and another table per lambda --, the entries no item names untouched, the canon map, tables that do not fit the data, and
bad descriptors and items refused by status bit, file by file, with the other files sized in full."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import adversarial_tables as AT  # noqa: E402
import interleaved_reference as IR  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 60000                                                 # above every table
GAP = 5                                                          # sentinel columns before, between and after the files
BETWEEN = 7                                                      # sentinel indices between two planes
# (n, part) of the three files of C = 3 streams: one part of three runs; 37 parts, runs split inside streams, short steps, a
# short last part; runs of one symbol
FILES3 = [(100, 1000), (777, 64), (1, 64)]
C_, L_ = 3, 3
KEEP = 7                                                         # what an entry of `sizes` holds before the launch


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _u32(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                    # (a copy: the shared arrays are read-only)


class Planes:
    """L planes of the three files: in every plane the files are columns of a [C, W] matrix with sentinel columns around
    them, and BETWEEN sentinel indices follow every plane.  idxs[l][f] u16 [C, n_f], freq u16 [L, C, T].  The descriptors,
    the items -- every (file, part) once, shuffled, interleaved with padding -- and, from the NumPy coder, sizes [L, P_all]."""

    def __init__(self, idxs, freq, N, canon=None, seed=0):
        self.idxs, self.freq, self.N = idxs, freq, N
        ns, parts = [n for n, _ in FILES3], [p for _, p in FILES3]
        self.F = len(FILES3)
        self.col = [GAP + sum(ns[:f]) + GAP * f for f in range(self.F)]
        self.W = self.col[-1] + ns[-1] + GAP
        self.stride = C_ * self.W + BETWEEN
        self.array = np.full(L_ * self.stride, SENTINEL, np.uint16)
        for l in range(L_):
            m = self.array[l * self.stride: l * self.stride + C_ * self.W].reshape(C_, self.W)
            for f in range(self.F):
                m[:, self.col[f]: self.col[f] + ns[f]] = idxs[l][f]
        coded = idxs if canon is None else [[np.take_along_axis(canon, i.astype(np.int64), axis=1) for i in plane] for plane in idxs]
        ref = [[IR.encode(coded[l][f], freq[l], parts[f])[0] for f in range(self.F)] for l in range(L_)]
        self.n_parts = [r.size for r in ref[0]]
        self.part_base = [sum(self.n_parts[:f]) for f in range(self.F)]
        self.P_all = sum(self.n_parts)
        self.sizes = np.stack([np.concatenate(r) for r in ref]).astype(np.uint32)        # [L, P_all]
        self.files = np.array([[self.col[f], self.W, ns[f], self.part_base[f], 0, parts[f], 0, 0] for f in range(self.F)], np.int64)
        items = [(f, p) for f in range(self.F) for p in range(self.n_parts[f])]
        np.random.default_rng(seed).shuffle(items)
        self.items = np.array([it for pair in zip(items, [(-1, -1)] * len(items)) for it in pair][:-1] + [(-1, 7)], np.int32)

    def slots(self, f):
        return slice(self.part_base[f], self.part_base[f] + self.n_parts[f])

    def run(self, files=None, items=None, canon=None, fill=None, array=None):
        """One launch -> (sizes u32 [L, P_all], status [F] list); the index array must come back unchanged."""
        from vbq_amd import ops
        d_idx = _dev(self.array if array is None else array)
        before = _u16(d_idx).copy()
        sizes = None if fill is None else torch.full((L_, self.P_all), fill, dtype=torch.int32, device="cuda").view(torch.uint32)
        got, st = ops.rans_il_rates_files(d_idx, _dev(self.files if files is None else files),
                                          _dev(self.items if items is None else items), _dev(self.freq), self.P_all,
                                          lambda_stride=self.stride, N=self.N, canon=None if canon is None else _dev(canon),
                                          sizes=sizes)
        assert tuple(got.shape) == (L_, self.P_all) and got.dtype == torch.uint32 and tuple(st.shape) == (self.F,)
        assert np.array_equal(_u16(d_idx), before)                # (the kernel reads the indices only)
        return _u32(got), _u32(st).tolist()


def _fitted(N):
    """Plane l, stream c: rounded normals about a centre and with a spread of its own (narrow, middling and wide, in another
    order per plane), and the table fitted to 4000 draws of it (every entry >= 1): the sizes of a plane are its own, so a
    kernel that took another plane's indices or another lambda's table would be found out."""
    from vbq_amd.coder import quantize_frequencies
    T = 2 ** (N + 1) - 1
    rng = np.random.default_rng(77 + N)
    centre = rng.integers(T // 8, T - T // 8, (L_, C_))
    spread = np.array([[0.3, 2.0, 25.0], [2.0, 300.0, 0.3], [300.0, 25.0, 2.0]] if N == 10 else
                      [[0.5, 1.5, 5.0], [1.5, 5.0, 0.5], [5.0, 0.5, 1.5]])                  # (a table of 15 symbols)

    def draw(l, n):
        return np.clip(np.rint(rng.normal(centre[l, :, None], spread[l, :, None], (C_, n))), 0, T - 1).astype(np.uint16)
    freq = np.stack([quantize_frequencies(np.stack([np.bincount(r, minlength=T) for r in draw(l, 4000)])) for l in range(L_)])
    return [[draw(l, n) for n, _ in FILES3] for l in range(L_)], freq


@pytest.fixture(scope="module")
def three():
    """The three files on three planes at N = 10 with their reference sizes: shared by the cases below, never changed."""
    b = Planes(*_fitted(10), 10)
    for a in (b.array, b.sizes, b.files, b.items, b.freq):
        a.setflags(write=False)
    return b


@pytest.mark.parametrize("N", [10, 3])
def test_three_files_at_three_lambdas_in_one_launch_match_the_numpy_coder(N):
    b = Planes(*_fitted(N), N)
    assert b.n_parts == [1, 37, 1] and b.stride == C_ * b.W + 7 and len(b.items) == 2 * 39
    # every plane has a table and sizes of its own: file 0's one part of 300 symbols costs another number of words in each
    assert len({b.freq[l].tobytes() for l in range(L_)}) == L_ and len({int(b.sizes[l, 0]) for l in range(L_)}) == L_
    got, st = b.run()                                             # (sizes zeroed by the wrapper)
    assert st == [0, 0, 0]
    for l in range(L_):
        assert np.array_equal(got[l], b.sizes[l]), l


def test_each_plane_equals_the_one_lambda_sizes_call(three):
    """The contract in its own words: row l is what vbq_rans_il_sizes_files_u16 gives on plane l with the row block freq[l]."""
    from vbq_amd import ops
    b = three
    got, _ = b.run()
    for l in range(L_):
        plane = _dev(b.array[l * b.stride: (l + 1) * b.stride])
        one, st = ops.rans_il_sizes_files(plane, _dev(b.files), _dev(b.items), _dev(b.freq[l:l + 1]), b.P_all, N=b.N)
        assert not _u32(st).any() and np.array_equal(_u32(one), got[l])


def test_entries_of_unlisted_parts_are_left_untouched_at_every_lambda(three):
    b = three
    left_out = {(1, 20), (1, 36), (2, 0)}
    keep = np.array([(f, p) for f, p in b.items.tolist() if (f, p) not in left_out], np.int32)
    got, st = b.run(items=keep, fill=KEEP)
    want = b.sizes.copy()
    for f, p in left_out:
        want[:, b.part_base[f] + p] = KEEP
    assert st == [0, 0, 0] and np.array_equal(got, want)


def test_canon_is_applied_to_the_staged_table():
    """With a map that folds some ranks onto lower ones the sizes are those of the reference coding canon[c][idx]."""
    N = 10
    idxs, freq = _fitted(N)
    T = 2 ** (N + 1) - 1
    canon = np.tile(np.arange(T, dtype=np.uint16), (C_, 1))
    canon[0, 1::2] -= 1                                           # stream 0: odd ranks onto the even rank below
    canon[2, 900:1200] = 900                                      # stream 2: a run of 300 ranks onto its first
    b, plain = Planes(idxs, freq, N, canon=canon), Planes(idxs, freq, N)
    assert not np.array_equal(b.sizes, plain.sizes)               # the map changes what is coded
    got, st = b.run(canon=canon)
    assert st == [0, 0, 0] and np.array_equal(got, b.sizes)


def test_tables_that_do_not_fit_the_data():
    """A spike, the ramp and half_ones across the streams, another family order per lambda, none fitted to the data; plane 0
    holds frequency-1 symbols only: 15 bits a symbol on top of the 16 of a lane's start state.  File 0's one part has three
    runs of 100 symbols: lanes 0 .. 35 own six symbols, the others three."""
    N = 7
    freq, draw = AT.mixed_model(L_, C_, N)
    idxs = [[draw(l, n) for n, _ in FILES3] for l in range(L_)]
    b = Planes(idxs, freq, N)
    assert all(np.all(np.take_along_axis(freq[0], i.astype(np.int64), axis=1) == 1) for i in idxs[0])
    assert int(b.sizes[0, 0]) == 128 + 36 * (15 * 6 // 16) + 28 * (15 * 3 // 16) == 364
    got, st = b.run()
    assert st == [0, 0, 0] and np.array_equal(got, b.sizes)


# ---- refusals: one kind per case, in one file of the three; the others are sized in full.  None of these inputs faults a
# correct kernel: each is refused by a compare before anything is indexed with it.
def _only(b, got, bad):
    """Every entry of the files other than `bad` is the reference's, every entry of `bad` still holds KEEP."""
    want = b.sizes.copy()
    want[:, b.slots(bad)] = KEEP
    return np.array_equal(got, want)


@pytest.mark.parametrize("f,field,value", [(1, 4, 1), (0, 4, -1), (1, 2, 0), (2, 5, 0), (1, 5, (1 << 24) + 1)],
                         ids=["table-1", "table-negative", "n-0", "part-0", "part-too-long"])
def test_a_bad_descriptor_sets_bit_7_and_nothing_of_the_file_is_written(three, f, field, value):
    b = three
    files = b.files.copy()
    files[f, field] = value
    got, st = b.run(files=files, fill=KEEP)
    assert st == [128 if g == f else 0 for g in range(b.F)] and _only(b, got, f)


def test_a_size_block_past_P_all_sets_bit_7(three):
    b = three
    files = b.files.copy()
    files[2, 3] = b.P_all                                         # file 2's one part would be entry P_all: the next lambda's row
    got, st = b.run(files=files, fill=KEEP)
    assert st == [0, 0, 128] and _only(b, got, 2)
    files[2, 3] = -1
    got, st = b.run(files=files, fill=KEEP)
    assert st == [0, 0, 128] and _only(b, got, 2)


def test_a_file_that_crosses_into_the_next_plane_is_refused_at_every_lambda(three):
    """File 2 moved so that its last stream ends one symbol past its plane: inside [0, n_idx) for the planes 0 and 1 (the
    symbol is the first between-plane sentinel), and refused for all three."""
    b = three
    files = b.files.copy()
    files[2, 0] = b.stride - (C_ - 1) * b.W - 1 + 1               # idx_base + (C - 1) stride + n == lambda_stride + 1
    assert files[2, 0] + (C_ - 1) * b.W + 1 == b.stride + 1 <= b.array.size
    got, st = b.run(files=files, fill=KEEP)
    assert st == [0, 0, 128] and _only(b, got, 2)
    files[2, 0] -= 1                                              # ending exactly at the plane's end is accepted
    got, st = b.run(files=files, fill=KEEP)
    assert st == [0, 0, 0] and np.array_equal(got[:, :b.part_base[2]], b.sizes[:, :b.part_base[2]])
    T = b.freq.shape[2]
    for l in range(L_):                                           # the symbols now there; a sentinel is coded as symbol 0
        sym = b.array[l * b.stride + files[2, 0] + b.W * np.arange(C_)].reshape(C_, 1)
        assert got[l, b.part_base[2]] == IR.encode(np.where(sym < T, sym, 0), b.freq[l], 64)[0][0]


def test_an_item_outside_its_file_or_of_no_file_sets_bit_7(three):
    b = three
    got, st = b.run(items=np.concatenate([b.items, np.array([[1, b.n_parts[1]]], np.int32)]), fill=KEEP)
    assert st == [0, 128, 0] and np.array_equal(got, b.sizes)
    got, st = b.run(items=np.concatenate([np.array([[1, -1]], np.int32), b.items]), fill=KEEP)
    assert st == [0, 128, 0] and np.array_equal(got, b.sizes)
    got, st = b.run(items=np.concatenate([np.array([[b.F, 0]], np.int32), b.items]), fill=KEEP)
    assert st == [128, 0, 0] and np.array_equal(got, b.sizes)
    got, st = b.run(items=np.array([[-2, 0], [-1, 0]], np.int32), fill=KEEP)
    assert st == [128, 0, 0] and (got == KEEP).all()


def test_the_wrapper_checks_its_arguments(three):
    from vbq_amd import _lib, ops
    b = three
    args = lambda: (_dev(b.array), _dev(b.files), _dev(b.items), _dev(b.freq), b.P_all)      # noqa: E731
    with pytest.raises(ValueError, match="sizes"):
        ops.rans_il_rates_files(*args(), lambda_stride=b.stride, N=b.N,
                                sizes=torch.zeros(L_ * b.P_all, dtype=torch.int32, device="cuda").view(torch.uint32))
    with pytest.raises(ValueError, match="files must be"):
        ops.rans_il_rates_files(_dev(b.array), _dev(b.files[:, :6]), _dev(b.items), _dev(b.freq), b.P_all, lambda_stride=b.stride)
    with pytest.raises(ValueError, match="canon must be"):
        ops.rans_il_rates_files(*args(), lambda_stride=b.stride, N=b.N, canon=torch.zeros((C_, 5), dtype=torch.uint16, device="cuda"))
    with pytest.raises(_lib.VBQError, match="do not fit"):
        ops.rans_il_rates_files(*args(), lambda_stride=b.stride + 1, N=b.N)
