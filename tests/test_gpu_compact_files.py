"""The compact batch kernels on the GPU (vbq_rans_il_sizes_files_u16 / _encode_files_u16 / _decode_files_u16, include/vbq.h
"Compact batch") against the NumPy coder of tests/interleaved_reference.py: the files are made on the host, so the decoder is
tested without the encoder and the encoder against bytes -- sizes, payload bytes and decoded indices identical, the positions
between the files untouched, and damaged input refused by status bit, file by file."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import adversarial_tables as AT  # noqa: E402
import interleaved_reference as IR  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 60000                                                 # above every table: no decoder writes it
GAP = 5                                                          # sentinel columns before, between and after the files
# (n, part, table) of the three files of C = 3 streams: one part of three runs; 37 parts, runs split inside streams, short
# steps, a short last part; runs of one symbol
FILES3 = [(100, 1000, 0), (777, 64, 1), (1, 64, 0)]


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


class Batch:
    """Files of C streams laid side by side as columns of one [C, W] index matrix with sentinel columns around them, their
    descriptors, items and -- from the NumPy coder -- sizes, offsets and payloads, as the three kernels take them."""

    def __init__(self, idxs, tables, parts, freq, N, seed=0, canon=None):
        self.idxs, self.tables, self.parts, self.freq, self.N = idxs, tables, parts, freq, N
        self.F, self.C = len(idxs), idxs[0].shape[0]
        ns = [i.shape[1] for i in idxs]
        self.col = [GAP + sum(ns[:f]) + GAP * f for f in range(self.F)]
        self.W = self.col[-1] + ns[-1] + GAP
        self.matrix = np.full((self.C, self.W), SENTINEL, np.uint16)
        for f, i in enumerate(idxs):
            self.matrix[:, self.col[f]: self.col[f] + ns[f]] = i
        coded = idxs if canon is None else [np.take_along_axis(canon, i.astype(np.int64), axis=1) for i in idxs]
        ref = [IR.encode(i, freq[t], p) for i, t, p in zip(coded, tables, parts)]
        self.n_parts = [r[0].size for r in ref]
        self.part_base = [sum(self.n_parts[:f]) for f in range(self.F)]
        self.P_all = sum(self.n_parts)
        self.sizes = np.concatenate([r[0] for r in ref]).astype(np.uint32)
        self.payload = np.concatenate([r[1] for r in ref]).astype(np.uint16)
        self.offsets = (np.cumsum(self.sizes, dtype=np.int64) - self.sizes).astype(np.int64)
        n_words_f = [int(r[1].size) for r in ref]
        self.word_base = [sum(n_words_f[:f]) for f in range(self.F)]
        self.files = np.array([[self.col[f], self.W, ns[f], self.part_base[f], tables[f], parts[f], self.word_base[f], n_words_f[f]]
                               for f in range(self.F)], np.int64)
        # every (file, part) once, shuffled, interleaved with padding
        items = [(f, p) for f in range(self.F) for p in range(self.n_parts[f])]
        rng = np.random.default_rng(seed)
        rng.shuffle(items)
        self.items = np.array([it for pair in zip(items, [(-1, -1)] * len(items)) for it in pair][:-1] + [(-1, 7)], np.int32)

    def expect(self, f_zero=None, zero_parts=(), untouched=()):
        """The index matrix a decode leaves: file f_zero with the listed parts zeroed; the files of `untouched` all sentinel."""
        want = self.matrix.copy()
        for f in untouched:
            want[:, self.col[f]: self.col[f] + self.idxs[f].shape[1]] = SENTINEL
        if f_zero is not None:
            flat, part = self.idxs[f_zero].reshape(-1).copy(), self.parts[f_zero]
            for p in zero_parts:
                flat[p * part: (p + 1) * part] = 0
            want[:, self.col[f_zero]: self.col[f_zero] + self.idxs[f_zero].shape[1]] = flat.reshape(self.idxs[f_zero].shape)
        return want

    def decode(self, sizes=None, offsets=None, payload=None, files=None, items=None, freq=None):
        """One launch -> (status [F] list, the index matrix)."""
        from vbq_amd import ops
        out = torch.full((self.C, self.W), SENTINEL - 65536, dtype=torch.int16, device="cuda").view(torch.uint16)
        pick = lambda given, own: _dev(own if given is None else given)                       # noqa: E731
        _, st = ops.rans_il_decode_files(pick(payload, self.payload), pick(sizes, self.sizes), pick(offsets, self.offsets),
                                         pick(files, self.files), pick(items, self.items), pick(freq, self.freq),
                                         out.view(-1), N=self.N)
        return _u32(st).tolist(), _u16(out)


def _three(N, adversarial=False):
    """adversarial: tables and draws that do not fit each other (adversarial_tables.mixed_model) instead of the fitted ones."""
    if adversarial:
        freq, draw = AT.mixed_model(2, 3, N)
        return [draw(t, n) for n, _, t in FILES3], [t for _, _, t in FILES3], [p for _, p, _ in FILES3], freq
    cases = [IR.make_case(3, n, N, seed=s) for s, (n, _, _) in enumerate(FILES3)]
    freq = np.stack([cases[0][1], cases[1][1]])                  # table 0 from file 0, table 1 from file 1: every entry >= 1
    return [c[0] for c in cases], [t for _, _, t in FILES3], [p for _, p, _ in FILES3], freq


@pytest.fixture(scope="module")
def three():
    """The three files at N = 10 with their reference coding: shared by the damage cases, never changed."""
    b = Batch(*_three(10), 10)
    for a in (b.sizes, b.offsets, b.payload, b.files, b.items, b.freq, b.matrix):
        a.setflags(write=False)
    return b


def _check_all_three(b, canon=None):
    from vbq_amd import ops
    d_idx, d_files, d_items, d_freq = _dev(b.matrix).view(-1), _dev(b.files), _dev(b.items), _dev(b.freq)
    d_canon = None if canon is None else _dev(canon)
    sizes, st = ops.rans_il_sizes_files(d_idx, d_files, d_items, d_freq, b.P_all, N=b.N, canon=d_canon)
    assert np.array_equal(_u32(sizes), b.sizes) and not _u32(st).any()
    s64 = sizes.view(torch.int32).to(torch.int64)
    payload = torch.zeros(b.payload.size, dtype=torch.uint16, device="cuda")
    _, st = ops.rans_il_encode_files(d_idx, d_files, d_items, d_freq, sizes, torch.cumsum(s64, 0) - s64, payload, N=b.N,
                                     canon=d_canon)
    assert not _u32(st).any()
    assert _u16(payload).tobytes() == b.payload.tobytes()
    assert np.array_equal(_u16(d_idx.view(b.C, b.W)), b.matrix)   # (the encode side reads the indices only)


@pytest.mark.parametrize("N", [10, 3])
def test_three_files_in_one_launch_match_the_numpy_coder(N):
    b = Batch(*_three(N), N)
    assert b.n_parts == [1, 37, 1] and len(b.items) == 2 * 39
    st, got = b.decode()
    assert st == [0, 0, 0]
    assert np.array_equal(got, b.matrix)                          # every index, and every sentinel intact
    _check_all_three(b)


def test_three_files_of_mismatched_tables_match_the_numpy_coder():
    """A spike, the ramp and half_ones across the streams of the two tables, none fitted to the data; files 0 and 2 hold
    frequency-1 symbols only: 15 bits a symbol on top of the 16 of a lane's start state, so a lane with k symbols takes
    15 k // 16 words.  File 0's one part has three runs of 100 symbols: lanes 0 .. 35 own six symbols, the others three."""
    N = 7
    b = Batch(*_three(N, adversarial=True), N)
    assert [b.freq[0, c].tobytes() for c in range(3)] == [r.tobytes() for r in (AT.spike(7, 0), AT.ramp(), AT.half_ones(7))]
    assert all(np.all(np.take_along_axis(b.freq[0], b.idxs[f].astype(np.int64), axis=1) == 1) for f in (0, 2))
    assert b.n_parts == [1, 37, 1] and int(b.sizes[0]) == 128 + 36 * (15 * 6 // 16) + 28 * (15 * 3 // 16) == 364
    st, got = b.decode()
    assert st == [0, 0, 0]
    assert np.array_equal(got, b.matrix)
    _check_all_three(b)


@pytest.mark.parametrize("N", [10, 3])
def test_one_large_file_whose_runs_carry_lane_states_across_streams(N):
    S, n, part = IR.CASES[-1]
    assert (S, n, part) == (64, 1536, 1 << 17)
    idx, freq, sizes_ref, payload_ref = IR.reference_case(S, n, part, N)
    b = Batch([idx], [0], [part], freq[None].copy(), N)
    assert np.array_equal(b.sizes, sizes_ref) and b.payload.tobytes() == payload_ref.tobytes()
    st, got = b.decode()
    assert st == [0] and np.array_equal(got, b.matrix)
    _check_all_three(b)


def test_canon_is_applied_to_the_staged_table():
    """With a map that folds some ranks onto lower ones the bytes are those of the reference coding canon[c][idx]."""
    N = 10
    idxs, tables, parts, freq = _three(N)
    T = 2 ** (N + 1) - 1
    canon = np.tile(np.arange(T, dtype=np.uint16), (3, 1))
    canon[0, 1::2] -= 1                                           # stream 0: odd ranks onto the even rank below
    canon[2, 900:1200] = 900                                      # stream 2: a run of 300 ranks onto its first
    b = Batch(idxs, tables, parts, freq, N, canon=canon)
    plain = Batch(idxs, tables, parts, freq, N)
    assert b.payload.tobytes() != plain.payload.tobytes()         # the map changes what is coded
    _check_all_three(b, canon)


def test_entries_and_words_of_unlisted_parts_are_left_untouched(three):
    from vbq_amd import ops
    b = three
    keep = np.array([(f, p) for f, p in b.items.tolist() if (f, p) != (1, 20)], np.int32)
    sizes = torch.full((b.P_all,), 7, dtype=torch.int32, device="cuda").view(torch.uint32)
    ops.rans_il_sizes_files(_dev(b.matrix).view(-1), _dev(b.files), _dev(keep), _dev(b.freq), b.P_all, N=b.N, sizes=sizes)
    want = b.sizes.copy()
    want[b.part_base[1] + 20] = 7
    assert np.array_equal(_u32(sizes), want)
    st, got = b.decode(items=keep)
    want = b.expect()
    flat = np.full(3 * 777, SENTINEL, np.uint16)
    flat[: 20 * 64], flat[21 * 64:] = b.idxs[1].reshape(-1)[: 20 * 64], b.idxs[1].reshape(-1)[21 * 64:]
    want[:, b.col[1]: b.col[1] + 777] = flat.reshape(3, 777)
    assert st == [0, 0, 0] and np.array_equal(got, want)


# ---- damage: one kind per case, in file 1 of the three; the other files decode in full.  None of these inputs faults a correct
# kernel: each is refused by a compare before anything is indexed with it.
def test_a_part_size_of_127_sets_bit_0(three):
    b, p = three, 5
    sizes = b.sizes.copy()
    sizes[b.part_base[1] + p] = 127
    st, got = b.decode(sizes=sizes)
    assert st == [0, 1, 0] and np.array_equal(got, b.expect(1, [p]))


def test_a_part_short_of_words_sets_bit_1(three):
    """A part of 64 symbols or fewer in one run has no renormalisation words (every lane codes one symbol from the start
    state), so the part that starves is file 0's one part of 300 symbols: it and its file claim one word less."""
    b = three
    assert b.n_parts[0] == 1 and int(b.sizes[0]) > 128 + 1
    sizes, files = b.sizes.copy(), b.files.copy()
    sizes[0] -= 1
    files[0, 7] -= 1                                              # (the file's words still end where its last part ends: no bit 4)
    st, got = b.decode(sizes=sizes, files=files)
    assert st == [2, 0, 0] and np.array_equal(got, b.expect(0, [0]))


def test_a_word_left_over_sets_bit_2(three):
    b, p = three, 7
    assert int(b.sizes[b.part_base[1] + p]) < 64 + 128            # one more word still fits the size range and the file's words
    sizes = b.sizes.copy()
    sizes[b.part_base[1] + p] += 1
    st, got = b.decode(sizes=sizes)
    assert st == [0, 4, 0] and np.array_equal(got, b.expect(1, [p]))


def test_a_frequency_row_not_summing_to_2_15_sets_bit_3(three):
    b = three
    freq = b.freq.copy()
    freq[1, 1, 0] += 1                                            # table 1 is file 1's alone; its stream 1 is symbols [777, 1554)
    st, got = b.decode(freq=freq)
    assert st == [0, 8, 0] and np.array_equal(got, b.expect(1, range(777 // 64, 1553 // 64 + 1)))


def test_an_offset_into_the_next_files_words_sets_bit_4(three):
    b, p = three, 9
    offsets = b.offsets.copy()
    offsets[b.part_base[1] + p] = b.word_base[2]
    st, got = b.decode(offsets=offsets)
    assert st == [0, 16, 0] and np.array_equal(got, b.expect(1, [p]))


@pytest.mark.parametrize("field,value", [(4, 2), (0, None), (5, 0)], ids=["table", "idx_base", "part"])
def test_a_bad_descriptor_sets_bit_7_and_nothing_of_the_file_is_written(three, field, value):
    b = three
    files = b.files.copy()
    # idx_base: the last stream of file 1 ends one symbol past n_idx
    files[1, field] = b.C * b.W - (b.C - 1) * b.W - 777 + 1 if value is None else value
    st, got = b.decode(files=files)
    assert st == [0, 128, 0] and np.array_equal(got, b.expect(untouched=[1]))


def test_an_item_outside_its_file_or_of_no_file_sets_bit_7(three):
    b = three
    st, got = b.decode(items=np.concatenate([b.items, np.array([[1, b.n_parts[1]]], np.int32)]))
    assert st == [0, 128, 0] and np.array_equal(got, b.matrix)
    st, got = b.decode(items=np.concatenate([np.array([[b.F, 0]], np.int32), b.items]))
    assert st == [128, 0, 0] and np.array_equal(got, b.matrix)
