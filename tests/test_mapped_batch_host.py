"""The host side of the mapped batch writer (compress_latents_to_bytes_mapped_batch): bitstream.mapped_encode_plan against a
brute-force restatement, the ctypes signatures and the argument validation of vbq_rans_map_encode_files_u16 /
vbq_rans_map_sizes_files_u16 through the built library, and the quantizer's checks that raise before any device work.  No GPU is
needed."""
import re

import numpy as np
import pytest

import mapped_window_reference as WR
from vbq_amd import bitstream as bs

ROWS, PALETTE_OF, SIZES = [1, 7, 64, 65, 200], [1, 0, 1, 2, 0], [2, 4, 1]


def brute_plan(rows, pal, sizes, segment, C):
    """mapped_encode_plan restated with Python loops."""
    F, G = len(rows), len(sizes)
    nseg = [-(-n // segment) for n in rows]
    seg_base, M = [], 0
    for f in range(F):
        seg_base.append(M)
        M += C * nseg[f]
    row0, group_rows, items = [0] * F, [0] * G, []
    for g in range(G):
        count = 0
        for f in range(F):
            if pal[f] != g:
                continue
            row0[f] = group_rows[g]
            group_rows[g] += -(-rows[f] // 8) * 8
            for s in range(nseg[f]):
                items.append((f, s))
                count += 1
        items += [(-1, -1)] * (-count % 64)
    idx_base, n_idx = [], 0
    for g in range(G):
        idx_base.append(n_idx)
        n_idx += sizes[g] * C * group_rows[g]
    cls_base, n_cls = [], 0
    for f in range(F):
        cls_base.append(n_cls)
        n_cls += -(-rows[f] // 8) * 8
    files = [(idx_base[pal[f]] + row0[f], group_rows[pal[f]], C * group_rows[pal[f]], rows[f], seg_base[f], pal[f], cls_base[f], 0)
             for f in range(F)]
    palettes = [[0] * sizes[g] + [-1] * (4 - sizes[g]) for g in range(G)]
    return nseg, seg_base, M, row0, group_rows, idx_base, n_idx, cls_base, n_cls, files, palettes, items


@pytest.mark.parametrize("segment,C", [(64, 3), (7, 2), (1024, 1)])
def test_mapped_encode_plan_matches_the_brute_force(segment, C):
    p = bs.mapped_encode_plan(ROWS, PALETTE_OF, SIZES, segment, C)
    nseg, seg_base, M, row0, group_rows, idx_base, n_idx, cls_base, n_cls, files, palettes, items = brute_plan(
        ROWS, PALETTE_OF, SIZES, segment, C)
    assert p.nseg.tolist() == nseg and p.seg_base.tolist() == seg_base and p.M == M
    assert p.row0.tolist() == row0 and p.group_rows.tolist() == group_rows and p.n_rows == sum(group_rows)
    assert p.group_row_base.tolist() == [sum(group_rows[:g]) for g in range(len(SIZES))]
    assert p.group_idx_base.tolist() == idx_base and p.n_idx == n_idx
    assert p.cls_base.tolist() == cls_base and p.n_cls == n_cls
    assert p.files.dtype == np.int64 and p.files.shape == (len(ROWS), 8) and [tuple(r) for r in p.files.tolist()] == files
    assert p.palettes.dtype == np.int32 and p.palettes.tolist() == palettes
    assert p.items.dtype == np.int32 and [tuple(r) for r in p.items.tolist()] == items
    # nseg, seg_base, M and the items are encode_plan's with the palette in the place of the table
    e = bs.encode_plan(ROWS, PALETTE_OF, segment, C, len(SIZES))
    assert np.array_equal(p.items, e.items) and np.array_equal(p.seg_base, e.seg_base) and p.M == e.M
    assert np.array_equal(p.nseg, e.nseg) and np.array_equal(p.row0, e.row0) and np.array_equal(p.group_rows, e.group_rows)


def test_mapped_encode_plan_properties():
    segment, C = 64, 3
    p = bs.mapped_encode_plan(ROWS, PALETTE_OF, SIZES, segment, C)
    F, G = len(ROWS), len(SIZES)
    # groups are adjacent, row runs are multiples of 8 and fill their group without overlap
    for g in range(G):
        fs = [f for f in range(F) if PALETTE_OF[f] == g]
        ends = [int(p.row0[f]) + -(-ROWS[f] // 8) * 8 for f in fs]
        assert [int(p.row0[f]) for f in fs] == ([0] + ends)[:len(fs)] and int(p.group_rows[g]) == ends[-1]
        assert all(int(p.row0[f]) % 8 == 0 for f in fs) and int(p.group_rows[g]) % 8 == 0
    # group bases account for P_g planes: the index ranges of the groups tile [0, n_idx), and every plane and channel of every
    # file stays inside its group's range
    run = 0
    for g in range(G):
        assert int(p.group_idx_base[g]) == run
        run += SIZES[g] * C * int(p.group_rows[g])
    assert run == p.n_idx
    taken = np.zeros(p.n_idx, np.int32)
    for f in range(F):
        base, stride, plane, n = (int(v) for v in p.files[f, :4])
        g = PALETTE_OF[f]
        assert stride == int(p.group_rows[g]) and plane == C * stride and base % 8 == 0 and plane % 8 == 0
        lo, hi = int(p.group_idx_base[g]), int(p.group_idx_base[g]) + SIZES[g] * C * int(p.group_rows[g])
        for k in range(SIZES[g]):
            for c in range(C):
                a = base + k * plane + c * stride
                assert lo <= a and a + n <= hi
                taken[a:a + n] += 1
    assert taken.max() == 1                                      # no two (file, plane, channel) share an index
    # every block of 64 items holds one palette; padding is (-1, -1)
    assert p.items.shape[0] % 64 == 0
    for b in range(p.items.shape[0] // 64):
        blk = p.items[64 * b: 64 * b + 64]
        fs = blk[blk[:, 0] >= 0, 0]
        assert fs.size >= 1 and len({PALETTE_OF[f] for f in fs}) == 1
        assert np.all(blk[blk[:, 0] < 0] == -1)
    real = p.items[p.items[:, 0] >= 0]
    assert sorted(map(tuple, real.tolist())) == sorted((f, s) for f in range(F) for s in range(-(-ROWS[f] // segment)))
    # class bases are multiples of 8 and the files' class bytes do not overlap
    spans = sorted((int(p.cls_base[f]), int(p.cls_base[f]) + ROWS[f]) for f in range(F))
    assert all(a % 8 == 0 for a, _ in spans) and all(spans[k][1] <= spans[k + 1][0] for k in range(F - 1))
    assert spans[-1][1] <= p.n_cls and p.n_cls % 8 == 0


def test_mapped_encode_plan_refusals():
    for rows, pal, sizes, segment, C, match in (([4], [0], [2], 0, 2, "segment"), ([4], [0], [2], 65534, 2, "segment"),
                                                ([4, 0], [0, 0], [1], 8, 2, "file 1 has no rows"),
                                                ([4], [1], [2], 8, 2, "outside"), ([4], [-1], [2], 8, 2, "outside"),
                                                ([4], [0], [5], 8, 2, "palette sizes"), ([4], [0], [0], 8, 2, "palette sizes"),
                                                ([4], [0], [1], 8, 0, "channels")):
        with pytest.raises(ValueError, match=match):
            bs.mapped_encode_plan(rows, pal, sizes, segment, C)
    p = bs.mapped_encode_plan([], [], [], 64, 3)
    assert p.M == 0 and p.n_idx == 0 and p.n_cls == 0 and p.files.shape == (0, 8) and p.items.shape == (0, 2)


NAMES = ("vbq_rans_map_encode_files_u16", "vbq_rans_map_sizes_files_u16")


def test_signatures_agree_with_the_header():
    """One ctypes argument per declared parameter, pointers where the header has pointers."""
    import ctypes as C
    import os
    from vbq_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vbq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    for name in NAMES:
        assert name in _lib.SIGNATURES
        params = [p.strip() for p in re.search(name + r"\s*\(([^)]*)\)", src).group(1).split(",")]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(params), name
        for p, t in zip(params, argtypes):
            assert t is (C.c_void_p if "*" in p else kinds[p.split()[0]]), (name, p)
    enc = re.search(NAMES[0] + r"\s*\(([^)]*)\)", src).group(1)
    siz = re.search(NAMES[1] + r"\s*\(([^)]*)\)", src).group(1)
    strip = lambda s: re.sub(r"\s+", " ", s)                                              # noqa: E731
    assert strip(enc).replace("uint16_t *d_words, ", "") == strip(siz)                    # the sizes entry has no d_words


@pytest.mark.parametrize("name", NAMES)
def test_argument_validation_of_the_mapped_batch_encoder(name):
    """Sizes and pointers are checked before any device work: callable on a CPU-only host."""
    import ctypes as C
    from vbq_amd import _lib, build
    build.build_hip()
    h = _lib.lib()
    one = C.c_void_p(8)                                           # a non-null pointer that a refused call never follows
    good = dict(d_idx=one, n_idx=100, d_cls=one, n_cls=50, d_files=one, n_files=1, d_palettes=one, n_palettes=1, max_classes=2,
                d_items=one, n_items=64, n_ch=2, seg=64, N=10, d_freq=one, n_tables=1, d_canon=None, d_words=one, d_sizes=one,
                M=4, d_status=None, stream=None)
    if name.endswith("sizes_files_u16"):
        del good["d_words"]
    pointers = [k for k in good if k.startswith("d_") and k not in ("d_canon", "d_status")]

    def call(**kw):
        a = dict(good, **kw)
        return getattr(h, name)(*[a[k] for k in good])

    for kw in [dict(n_items=63), dict(n_items=65), dict(n_palettes=0), dict(n_palettes=-1), dict(seg=65534), dict(seg=0),
               dict(N=11), dict(N=0), dict(n_files=65536), dict(n_ch=65536), dict(n_tables=0), dict(n_idx=-1), dict(n_cls=-1),
               dict(n_files=-1), dict(n_items=-64), dict(n_ch=-1), dict(M=-1), dict(max_classes=0), dict(max_classes=5)] + \
              [{k: None} for k in pointers]:
        assert call(**kw) == -1, kw
        assert name.encode() in h.vbq_last_error(), kw
    assert b"null pointer" in h.vbq_last_error()
    assert call(n_items=63) == -1 and b"multiple of 64" in h.vbq_last_error()
    assert call(n_palettes=0) == -1 and b"n_palettes=0" in h.vbq_last_error()
    assert call(n_files=0) == 0 and call(n_items=0) == 0 and call(n_ch=0) == 0
    assert call(n_files=0, **{k: None for k in pointers}) == 0
    assert call(n_cls=0, n_files=0) == 0


# ---------------------------------------------------------------------------------------------- the quantizer's own checks
N, C_ = 4, 3
LAMBS = [0.25, 0.5, 1.0, 2.0, 4.0]


@pytest.fixture(scope="module")
def quantizer():
    return WR.host_quantizer(C_, N, LAMBS)


def _pair(shape):
    return np.zeros(shape, np.float32), np.zeros(shape, np.float32)


def test_no_files_is_an_empty_list(quantizer):
    q = quantizer
    assert q.compress_latents_to_bytes_mapped_batch([], LAMBS[:2], []) == []
    assert q.compress_latents_to_bytes_mapped_batch([], [], []) == []
    assert q.compress_to_bytes_mapped_batch([], None, LAMBS[:2], []) == []
    assert q.coded_nbytes_mapped_batch([], LAMBS[:2], []) == []


def test_errors_are_raised_before_any_device_work(quantizer, monkeypatch):
    q = quantizer
    monkeypatch.setattr(type(q), "device", property(lambda self: pytest.fail("the device was asked for")))
    good, cls = _pair((1, 4, 5, C_)), np.zeros((1, 4, 5), np.int64)
    pal = LAMBS[:2]
    for call in (q.compress_latents_to_bytes_mapped_batch, q.coded_nbytes_mapped_batch):
        with pytest.raises(ValueError, match="file 1: a palette of 5 lambdas"):
            call([good, good], [pal, LAMBS], [cls, cls])
        with pytest.raises(ValueError, match="file 0: a palette of 5 lambdas"):
            call([good, good], LAMBS, [cls, cls])                 # one palette for all: the first file names it
        with pytest.raises(ValueError, match="file 1: repeated lambda"):
            call([good, good], [pal, [0.5, 0.5]], [cls, cls])
        with pytest.raises(ValueError, match=r"file 1: class outside \[0, 2\)"):
            call([good, good], pal, [cls, cls + 2])
        with pytest.raises(ValueError, match=r"file 0: class outside \[0, 2\)"):
            call([good, good], pal, [cls - 1, cls])
        with pytest.raises(ValueError, match="file 1: classes of shape"):
            call([good, good], pal, [cls, np.zeros((1, 4, 6), np.int64)])
        with pytest.raises(ValueError, match="file 1: classes must be integers"):
            call([good, good], pal, [cls, cls.astype(np.float32)])
        with pytest.raises(ValueError, match="1 class maps for 2 files"):
            call([good, good], pal, [cls])
        with pytest.raises(ValueError, match="one palette .* or a sequence of 2 palettes"):
            call([good, good], [pal], [cls, cls])
        with pytest.raises(ValueError, match="one palette .* or a sequence of 2 palettes"):
            call([good, good], [pal, 0.5], [cls, cls])
        with pytest.raises(KeyError, match="file 1: .*3.0"):
            call([good, good], [pal, [0.25, 3.0]], [cls, cls])
        with pytest.raises(KeyError, match="file 0: .*3.0"):
            call([good, good], [3.0], [cls, cls])
        with pytest.raises(ValueError, match="file 1: expected channel-last"):
            call([good, _pair((1, 4, 5, C_ + 1))], pal, [cls, cls])
        for segment in (0, 65534):
            with pytest.raises(ValueError, match="segment"):
                call([good], pal, [cls], segment=segment)
    with pytest.raises(ValueError, match="65536 files"):
        q.compress_latents_to_bytes_mapped_batch([good] * 65536, pal, [cls] * 65536)

    class Vae:
        def encode(self, X):
            return _pair((1, 2, 2, C_ + 1))
    with pytest.raises(ValueError, match="file 0: expected channel-last"):
        q.compress_to_bytes_mapped_batch([None], Vae(), pal, [np.zeros((1, 2, 2), np.int64)])
