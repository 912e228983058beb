"""The host side of the batch writer (compress_latents_to_bytes_batch): bitstream.encode_plan against a brute-force restatement,
the argument validation of vbq_rans_encode_files_u16 through the built library, and the quantizer's checks that raise before
any device work.  No GPU is needed."""
import numpy as np
import pytest

from vbq_amd import bitstream as bs

SEG = 64


def brute_plan(rows, tables, segment, C, n_tables):
    """encode_plan restated with Python loops."""
    F = len(rows)
    nseg = [-(-n // segment) for n in rows]
    seg_base, M = [], 0
    for f in range(F):
        seg_base.append(M)
        M += C * nseg[f]
    row0, group_rows, items = [0] * F, [0] * n_tables, []
    for t in range(n_tables):
        count = 0
        for f in range(F):
            if tables[f] != t:
                continue
            row0[f] = group_rows[t]
            group_rows[t] += -(-rows[f] // 8) * 8
            for g in range(nseg[f]):
                items.append((f, g))
                count += 1
        items += [(-1, -1)] * (-count % 64)
    group_row_base = [sum(group_rows[:t]) for t in range(n_tables)]
    files = [(C * group_row_base[tables[f]] + row0[f], group_rows[tables[f]], rows[f], seg_base[f], tables[f], 0) for f in range(F)]
    return nseg, seg_base, M, row0, group_rows, group_row_base, files, items


def _cases():
    rng = np.random.default_rng(3)
    edge = [1, SEG - 1, SEG, SEG + 1]
    # tables in mixed order; table 0 has more than 64 segments (several blocks), table 2 exactly 64, table 3 is unused
    rows = edge + [int(v) for v in rng.integers(1, 6 * SEG, 20)] + [70 * SEG + 3, 64 * SEG]
    tables = [1, 0, 1, 0] + [int(v) for v in rng.integers(0, 2, 20)] + [0, 2]
    yield "mixed", rows, tables, SEG, 3, 4
    yield "one-file", [5], [0], SEG, 2, 1
    yield "segment-1", [3, 1, 70], [1, 1, 0], 1, 1, 2
    yield "no-files", [], [], SEG, 3, 0


@pytest.mark.parametrize("case", list(_cases()), ids=lambda c: c[0])
def test_encode_plan_matches_the_brute_force(case):
    _, rows, tables, segment, C, n_tables = case
    p = bs.encode_plan(rows, tables, segment, C, n_tables)
    nseg, seg_base, M, row0, group_rows, group_row_base, files, items = brute_plan(rows, tables, segment, C, n_tables)
    assert p.nseg.tolist() == nseg and p.seg_base.tolist() == seg_base and p.M == M
    assert p.row0.tolist() == row0 and p.group_rows.tolist() == group_rows and p.group_row_base.tolist() == group_row_base
    assert p.n_rows == sum(group_rows)
    assert p.files.dtype == np.int64 and p.files.shape == (len(rows), 6) and [tuple(r) for r in p.files.tolist()] == files
    assert p.items.dtype == np.int32 and p.items.shape == (len(items), 2) and [tuple(r) for r in p.items.tolist()] == items


def test_encode_plan_properties():
    _, rows, tables, segment, C, n_tables = next(_cases())
    p = bs.encode_plan(rows, tables, segment, C, n_tables)
    F = len(rows)
    real = p.items[p.items[:, 0] >= 0]
    # every (file, segment) exactly once
    want = sorted((f, g) for f in range(F) for g in range(-(-rows[f] // segment)))
    assert sorted(map(tuple, real.tolist())) == want
    # blocks of 64, each of one table; padding only at the end of a table's blocks
    assert p.items.shape[0] % bs.ENCODE_BLOCK == 0
    block_tables = []
    for b in range(p.items.shape[0] // 64):
        blk = p.items[64 * b: 64 * b + 64]
        fs = blk[blk[:, 0] >= 0, 0]
        assert fs.size >= 1                                       # no block of padding alone
        ts = {tables[f] for f in fs}
        assert len(ts) == 1
        block_tables.append(ts.pop())
        pad = np.flatnonzero(blk[:, 0] < 0)
        assert np.all(blk[pad] == -1)
        if pad.size:                                              # padding is a suffix of the block ...
            assert pad[0] == 64 - pad.size
    assert block_tables == sorted(block_tables)                   # table by table
    for b in range(len(block_tables) - 1):                        # ... and only the last block of a table has any
        if block_tables[b] == block_tables[b + 1]:
            assert np.all(p.items[64 * b: 64 * b + 64, 0] >= 0)
    n_blocks = {t: block_tables.count(t) for t in set(block_tables)}
    segs = {t: sum(-(-rows[f] // segment) for f in range(F) if tables[f] == t) for t in range(n_tables)}
    assert segs[0] > 64 and n_blocks[0] == -(-segs[0] // 64) and segs[2] == 64 and n_blocks[2] == 1 and 3 not in n_blocks
    # seg_base is the file-major sum
    assert p.seg_base.tolist() == [sum(C * -(-n // segment) for n in rows[:f]) for f in range(F)]
    # rows: runs of one group do not overlap, start at multiples of 8 and fill the group
    for t in range(n_tables):
        fs = [f for f in range(F) if tables[f] == t]
        ends = [int(p.row0[f]) + -(-rows[f] // 8) * 8 for f in fs]
        assert [int(p.row0[f]) for f in fs] == ([0] + ends)[:len(fs)] and int(p.group_rows[t]) == (ends[-1] if ends else 0)
    # descriptors: the index range of every channel stays inside the C * n_rows indices
    for f in range(F):
        base, stride, n = (int(v) for v in p.files[f, :3])
        assert base % 8 == 0 and stride % 8 == 0 and base + (C - 1) * stride + n <= C * p.n_rows
    # a size block filled slot by slot through the plan is the concatenation of the per-file size blocks
    size_of = lambda f, c, g: 2 + (7 * f + 3 * c + g) % (segment + 1)                    # noqa: E731
    block = np.zeros(p.M, np.uint32)
    for f, g in real.tolist():
        for c in range(C):
            slot = int(p.seg_base[f]) + c * int(p.nseg[f]) + g
            assert block[slot] == 0
            block[slot] = size_of(f, c, g)
    per_file = [np.array([[size_of(f, c, g) for g in range(-(-rows[f] // segment))] for c in range(C)], np.uint32).reshape(-1)
                for f in range(F)]
    assert np.array_equal(block, np.concatenate(per_file))


def test_encode_plan_refusals():
    for rows, tables, segment, C, match in (([4], [0], 0, 2, "segment"), ([4], [0], 65534, 2, "segment"), ([4], [0], 8, 0, "channels"),
                                            ([4, 0], [0, 0], 8, 2, "file 1 has no rows"), ([4], [0, 1], 8, 2, "tables for"),
                                            ([4], [-1], 8, 2, "table outside"), ([1] * 65536, [0] * 65536, 8, 1, "65536 files")):
        with pytest.raises(ValueError, match=match):
            bs.encode_plan(rows, tables, segment, C)
    with pytest.raises(ValueError, match="table outside"):
        bs.encode_plan([4], [2], 8, 2, n_tables=2)


def test_argument_validation_of_the_batch_encoder():
    """Sizes and pointers are checked before any device work: callable on a CPU-only host."""
    import ctypes as C
    from vbq_amd import _lib, build
    build.build_hip()
    h = _lib.lib()
    one = C.c_void_p(8)                                           # a non-null pointer that a refused call never follows
    good = dict(d_idx=one, n_idx=100, d_files=one, n_files=1, d_items=one, n_items=64, n_ch=2, seg=64, N=10, d_freq=one,
                n_tables=1, d_canon=None, d_words=one, d_sizes=one, M=4, d_status=None, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return h.vbq_rans_encode_files_u16(*[a[k] for k in good])

    for kw in (dict(n_files=65536), dict(n_ch=65536), dict(seg=0), dict(seg=65534), dict(N=0), dict(N=11), dict(n_tables=0),
               dict(n_idx=-1), dict(n_files=-1), dict(n_items=-64), dict(n_ch=-1), dict(M=-1), dict(n_items=63), dict(n_items=65),
               dict(d_idx=None), dict(d_files=None), dict(d_items=None), dict(d_freq=None), dict(d_words=None), dict(d_sizes=None)):
        assert call(**kw) == -1, kw
        assert b"vbq_rans_encode_files_u16" in h.vbq_last_error(), kw
    assert b"null pointer" in h.vbq_last_error()
    assert call(n_items=63) == -1 and b"multiple of 64" in h.vbq_last_error()
    assert call(n_files=0) == 0 and call(n_items=0) == 0
    assert call(n_files=0, d_idx=None, d_files=None, d_items=None, d_freq=None, d_words=None, d_sizes=None) == 0


# ---------------------------------------------------------------------------------------------- the quantizer's own checks
N, C_ = 4, 3
LAMBS = [0.25, 2.0]


@pytest.fixture(scope="module")
def quantizer():
    """Code points and entropy models installed from arrays: nothing here touches a device."""
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    q = ChannelwisePriorCDFQuantizer(C_, N)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C_), np.array([0.5, 1.0, 2.0])))
    T = q.quantization_levels
    rng = np.random.default_rng(0)
    counts = {lamb: rng.integers(0, 50, (C_, T)) for lamb in LAMBS}
    q._code_counts, q._add_n_smoothing = counts, 1
    q.entropy_models = {lamb: -np.log2((c + 1) / (c + 1).sum(axis=1, keepdims=True)).astype(np.float32) for lamb, c in counts.items()}
    return q


def _pair(shape):
    return np.zeros(shape, np.float32), np.zeros(shape, np.float32)


def test_no_files_is_an_empty_list(quantizer):
    from vbq_amd import ChannelwisePriorCDFQuantizer
    assert quantizer.compress_latents_to_bytes_batch([], LAMBS[0]) == []
    assert quantizer.compress_latents_to_bytes_batch([], []) == []
    assert quantizer.compress_to_bytes_batch([], None, LAMBS[0]) == []
    assert ChannelwisePriorCDFQuantizer(C_, N).compress_latents_to_bytes_batch([], 1.0) == []      # (no models: nothing to look up)


def test_errors_are_raised_before_any_device_work(quantizer, monkeypatch):
    q = quantizer
    monkeypatch.setattr(type(q), "device", property(lambda self: pytest.fail("the device was asked for")))
    good = _pair((1, 4, 5, C_))
    for bad, match in ((_pair((1, 4, 5, C_ + 1)), "file 1: expected channel-last"),
                       ((good[0], np.zeros((1, 4, 6, C_), np.float32)), "file 1: expected channel-last"),
                       (_pair(()), "file 1: expected channel-last"), ((good[0],), "file 1: expected a pair"),
                       (_pair((1, 0, 5, C_)), "file 1: empty latent shape")):
        with pytest.raises(ValueError, match=match):
            q.compress_latents_to_bytes_batch([good, bad], LAMBS[0])
    for segment in (0, -3, 65534):
        with pytest.raises(ValueError, match="segment"):
            q.compress_latents_to_bytes_batch([good], LAMBS[0], segment=segment)
    with pytest.raises(ValueError, match="1 lambdas for 2 files"):
        q.compress_latents_to_bytes_batch([good, good], [LAMBS[0]])
    with pytest.raises(ValueError, match="3 lambdas for 2 files"):
        q.compress_latents_to_bytes_batch([good, good], LAMBS + LAMBS[:1])
    with pytest.raises(KeyError):
        q.compress_latents_to_bytes_batch([good, good], [LAMBS[0], 3.0])
    with pytest.raises(KeyError):
        q.compress_latents_to_bytes_batch([good], 3.0)

    class Vae:
        def encode(self, X):
            return _pair((1, 2, 2, C_ + 1))
    with pytest.raises(ValueError, match="file 0: expected channel-last"):
        q.compress_to_bytes_batch([None], Vae(), LAMBS[1])
