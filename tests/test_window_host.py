"""The host side of the window decode, without a GPU: bitstream.region_box / region_boxes / box_segments against a brute force
over a boolean array, their refusals, and the argument checks of vbq_rans_decode_window_f32."""
import ctypes as C

import numpy as np
import pytest

from vbq_amd import bitstream as bs


def _brute(shape, region, segment):
    """(segments that hold a marked row, the marked rows, the extents): mark the region in a boolean array of the leading shape,
    flatten, integer-divide by the segment."""
    mark = np.zeros(shape, bool)
    mark[tuple(region)] = True
    rows = np.flatnonzero(mark.reshape(-1))
    return np.unique(rows // segment), rows, mark[tuple(region)].shape


def _box_rows(dims, lo, hi):
    i0, i1, i2 = np.meshgrid(*(np.arange(l, h) for l, h in zip(lo, hi)), indexing="ij")
    return ((i0 * dims[1] + i1) * dims[2] + i2).reshape(-1)


def _levels(shape, region):
    return len(bs._collapse(bs._region_axes(shape, region)))


S = slice
CASES = [  # leading shape, region, segment, levels, segments selected, segments per stream
    ((1, 17, 23), (S(None), S(5, 9)), 64, 1, 3, 7),
    ((1, 17, 23), (S(None), S(None), S(7, 12)), 64, 2, 6, 7),
    ((2, 17, 23), (S(None), S(1, 16), S(3, 20)), 64, 3, 12, 13),
    ((1, 25, 40), (S(None), S(2, 23), S(1, 39)), 7, None, 121, 143),
    ((1, 256, 256), (S(None), S(96, 160), S(96, 160)), 1024, None, 16, 64),
    ((1, 256, 256), (S(None), S(96, 160), S(96, 160)), 64, None, 128, 1024),
]


@pytest.mark.parametrize("shape,region,segment,levels,n_sel,nseg", CASES)
def test_box_and_segments_match_the_brute_force(shape, region, segment, levels, n_sel, nseg):
    want_segs, want_rows, want_ext = _brute(shape, region, segment)
    dims, lo, hi, extents = bs.region_box(shape, region)
    assert extents == want_ext and int(np.prod(dims)) == int(np.prod(shape))
    assert np.array_equal(_box_rows(dims, lo, hi), want_rows)                    # the same rows, in the same (row-major) order
    got = bs.box_segments(dims, lo, hi, segment)
    assert got.dtype == np.int32 and np.array_equal(got, want_segs)
    assert got.size == n_sel and (int(np.prod(shape)) + segment - 1) // segment == nseg
    if levels is not None:
        assert _levels(shape, region) == levels


def test_many_regions_against_the_brute_force():
    rng = np.random.default_rng(3)
    for _ in range(300):
        shape = tuple(int(d) for d in rng.integers(1, 7, rng.integers(1, 4)))
        region = []
        for d in shape[: rng.integers(0, len(shape) + 1)]:
            a, b = sorted(int(v) for v in rng.integers(-d - 1, d + 2, 2))
            region.append([S(None), S(a, b), S(a, None), S(None, b), S(b, a)][rng.integers(0, 5)])
        segment = int(rng.integers(1, 9))
        want_segs, want_rows, want_ext = _brute(shape, region, segment)
        dims, lo, hi, extents = bs.region_box(shape, tuple(region))
        assert extents == want_ext, (shape, region)
        if 0 in extents:
            assert bs.box_segments(dims, lo, hi, segment).size == 0
            continue
        assert np.array_equal(_box_rows(dims, lo, hi), want_rows), (shape, region)
        assert np.array_equal(bs.box_segments(dims, lo, hi, segment), want_segs), (shape, region, segment)


def test_four_axes_collapse_or_refuse():
    with pytest.raises(ValueError, match="4 nested levels"):
        bs.region_box((2, 3, 4, 5), (S(0, 2), S(1, 3), S(1, 3), S(1, 4)))
    region = (S(1, 2), S(1, 3), S(None), S(1, 4))
    assert _levels((2, 3, 4, 5), region) == 2
    dims, lo, hi, extents = bs.region_box((2, 3, 4, 5), region)
    assert dims == (1, 24, 5) and lo == (0, 16, 1) and hi == (1, 24, 4) and extents == (1, 2, 4, 3)
    assert np.array_equal(_box_rows(dims, lo, hi), _brute((2, 3, 4, 5), region, 1)[1])
    # no leading axes at all (a latent of shape [C]): one row
    assert bs.region_box((), ()) == ((1, 1, 1), (0, 0, 0), (1, 1, 1), ())
    assert bs.box_segments((1, 1, 1), (0, 0, 0), (1, 1, 1), 5).tolist() == [0]
    assert bs.region_box((4, 5), None)[:3] == ((1, 1, 20), (0, 0, 0), (1, 1, 20))
    assert bs.region_box((4, 5), S(1, 3)) == ((1, 1, 20), (0, 0, 5), (1, 1, 15), (2, 5))


def test_refusals():
    for region, what in (((S(None), 3), "not a slice"), ((S(None), S(0, 8, 2)), "step 2"), ((S(None), S(None, None, -1)), "step -1"),
                         ((S(None),) * 4, "4 slices for 3"), ((S(None), np.int64(2)), "not a slice"), ((True,), "not a slice"),
                         ((S(0.5),), "region entry 0")):
        with pytest.raises(ValueError, match=what):
            bs.region_box((1, 17, 23), region)
    with pytest.raises(ValueError, match="empty leading shape"):
        bs.region_box((1, 0, 3), ())
    for segment in (0, 65534):
        with pytest.raises(ValueError, match="segment"):
            bs.box_segments((1, 17, 23), (0, 0, 0), (1, 17, 23), segment)
    for lo, hi in (((0, 0, 0), (1, 18, 23)), ((0, -1, 0), (1, 17, 23)), ((0, 5, 0), (1, 4, 23)), ((0, 0), (1, 17))):
        with pytest.raises(ValueError, match="does not lie in"):
            bs.box_segments((1, 17, 23), lo, hi, 64)


def test_files_of_different_shapes_share_one_collapse():
    shapes = [(1, 17, 23), (1, 20, 30), (2, 9, 11)]
    regions = [(S(None), S(3, 11), S(5, 13)), (S(0, 1), S(12, 20), S(22, 30)), (S(1, 2), S(0, 8), S(2, 10))]
    boxes, extents = bs.region_boxes(shapes, regions)
    assert extents == (1, 8, 8)
    for (dims, lo, hi), shape, region in zip(boxes, shapes, regions):
        assert tuple(h - l for l, h in zip(lo, hi)) == (1, 8, 8)
        assert np.array_equal(_box_rows(dims, lo, hi), _brute(shape, region, 1)[1])
    # rows 5:9 in full collapse to one level alone, but not beside a file whose rows are wider than the region
    alone = bs.region_box((1, 17, 23), (S(None), S(5, 9)))
    assert alone[:3] == ((1, 1, 391), (0, 0, 115), (1, 1, 207))
    boxes, extents = bs.region_boxes([(1, 17, 23), (1, 20, 30)], [(S(None), S(5, 9)), (S(None), S(5, 9), S(0, 23))])
    assert extents == (1, 4, 23) and boxes[0] == ((1, 17, 23), (0, 5, 0), (1, 9, 23)) and boxes[1] == ((1, 20, 30), (0, 5, 0), (1, 9, 23))
    with pytest.raises(ValueError, match="file 1: a region of extents"):
        bs.region_boxes(shapes[:2], [regions[0], (S(None), S(0, 8), S(0, 7))])
    with pytest.raises(ValueError, match="file 1: a region of extents"):
        bs.region_boxes([(1, 17, 23), (17, 23)], [None, None])
    assert bs.region_boxes([], []) == ([], ())


def test_the_c_call_checks_its_arguments_before_any_device_work():
    from vbq_amd import _lib
    h = _lib.lib()
    p = C.c_void_p(64)                    # never dereferenced: every call below returns before any device work
    err = lambda: h.vbq_last_error().decode()                                # noqa: E731

    def win(payload=p, n_words=10, sizes=p, offs=p, M=4, files=p, F=1, segs=p, n_sel=1, ch=None, n_ch_sel=2, n_ch=2, seg=64,
            N=10, freq=p, n_tables=1, values=p, w=(1, 1, 1), out=None, st=None):
        return h.vbq_rans_decode_window_f32(payload, n_words, sizes, offs, M, files, F, segs, n_sel, ch, n_ch_sel, n_ch, seg, N,
                                            freq, n_tables, values, w[0], w[1], w[2], out, st, None)

    assert win() == -1 and "null pointer" in err()                           # the sizes pass: the pointers are next (out is NULL)
    for kw in (dict(F=65536), dict(F=-1), dict(ch=p, n_ch_sel=65536), dict(n_ch_sel=-1), dict(seg=0), dict(seg=65534), dict(N=0),
               dict(N=11), dict(n_words=-1), dict(M=-1), dict(n_sel=-1), dict(n_ch=0), dict(n_tables=0), dict(w=(-1, 1, 1)),
               dict(w=(1, -1, 1)), dict(w=(1, 1, -1))):
        assert win(out=p, **kw) == -1 and "bad sizes" in err(), (kw, err())
    assert win(F=65535, ch=p, n_ch_sel=65535, seg=65533) == -1 and "null pointer" in err()   # the limits themselves pass
    assert win(out=p, n_ch_sel=1) == -1 and "without d_channels" in err()
    assert win(ch=p, n_ch_sel=1) == -1 and "null pointer" in err()
    assert win(out=p, w=(1 << 31, 1 << 31, 1 << 31)) == -1 and "too large" in err()
    assert win(out=p, F=4, w=(1 << 20, 1 << 20, 1 << 18)) == -1 and "too large" in err()      # 2^63 bytes
    for kw in (dict(sizes=None), dict(offs=None), dict(files=None), dict(segs=None), dict(freq=None), dict(values=None)):
        assert win(out=p, **kw) == -1 and "null pointer" in err(), kw
    assert win(out=p, payload=None) == -1 and "null d_payload" in err()
    # nothing to do: VBQ_OK with no launch, whatever the pointers -- but the sizes are still checked
    nothing = dict(payload=None, sizes=None, offs=None, files=None, segs=None, freq=None, values=None)
    for kw in (dict(F=0), dict(n_sel=0), dict(ch=p, n_ch_sel=0), dict(n_ch_sel=0), dict(w=(0, 1, 1)), dict(w=(1, 0, 1)),
               dict(w=(1, 1, 0))):
        assert win(**nothing, **kw) == 0, kw
        assert win(**nothing, **kw, N=11) == -1 and "bad sizes" in err(), kw
    assert h.vbq_abi_version() == 5                                          # added without an ABI version bump
