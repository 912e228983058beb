"""The host side of the mapped window decode (decompress_latents_mapped_batch / decompress_latents_mapped_window), without a GPU:
the staging plan against a restatement from the documented layout, every refusal with its message and file index, and the
argument checks of vbq_rans_map_decode_window_f32.  The files are written on the host from the NumPy coder
(tests/mapped_window_reference.py)."""
import ctypes as C

import numpy as np
import pytest

import mapped_window_reference as MW
from vbq_amd import bitstream as bs

S = slice
N, C_ = 4, 3
LAMBS = [0.25, 1.0, 2.0, 8.0]
SEG = 7


@pytest.fixture(scope="module")
def world():
    """A host-only quantizer and five files of three latent shapes: palettes of 2, 4 and 3 lambdas, two files in segments."""
    q = MW.host_quantizer(C_, N, LAMBS)
    rng = np.random.default_rng(5)
    shapes = [(1, 6, 9, C_), (2, 5, 7, C_), (1, 8, 8, C_), (1, 6, 9, C_), (1, 5, 11, C_)]
    palettes = [[LAMBS[2], LAMBS[0]], [LAMBS[3]], [LAMBS[1], LAMBS[3], LAMBS[0], LAMBS[2]], [LAMBS[0]], [LAMBS[3], LAMBS[1], LAMBS[2]]]
    mapped = [True, False, True, False, True]
    files, classes = [], []
    for shape, pal, m in zip(shapes, palettes, mapped):
        B = int(np.prod(shape[:-1]))
        cls = rng.integers(0, len(pal), B).astype(np.uint8) if m else np.zeros(B, np.uint8)
        files.append(MW.write_file(q, shape, pal, cls, SEG, rng, mapped=m)[0])
        classes.append(cls)
    regions = [(S(None), S(1, 5), S(2, 7)), (S(1, 2), S(0, 4), S(2, 7)), (S(None), S(4, 8), S(3, 8)), (S(None), S(2, 6), S(4, 9)),
               (S(None), S(1, 5), S(6, 11))]
    return q, files, classes, shapes, palettes, mapped, regions


def _parts(plan):
    cut, F = plan.cut, plan.F
    host = plan.host
    desc = host[cut[0]:cut[1]].view(np.int64).reshape(F, 16)
    segs = host[cut[1]:cut[1] + 4 * F * plan.n_sel].view(np.int32).reshape(F, plan.n_sel)
    chans = host[cut[2]:cut[2] + 4 * plan.C_sel].view(np.int32) if cut[3] > cut[2] else None
    return desc, segs, chans, host[cut[3]:cut[4]].tobytes(), host[cut[4]:cut[5]].view(np.uint16), host[cut[5]:cut[6]].view(np.uint16)


@pytest.mark.parametrize("channels", [None, [2, 0, 2]])
def test_plan_matches_the_restatement(world, channels, monkeypatch):
    q, files, classes, shapes, palettes, mapped, regions = world
    monkeypatch.setattr(type(q), "device", property(lambda self: pytest.fail("the device was asked for")))
    plan = q._mapped_window_plan(files, regions, channels)
    want = MW.restated_plan(q, files, regions, channels)
    desc, segs, chans, cls, sizes, payload = _parts(plan)
    assert plan.shape == want["shape"] + (C_ if channels is None else 3,) and plan.box == (1, 4, 5)
    assert np.array_equal(desc, want["desc"]) and np.array_equal(segs, want["segs"])
    assert (chans is None) if channels is None else np.array_equal(chans, want["channels"])
    assert cls == want["cls"] and plan.cls_bytes == len(cls)
    assert np.array_equal(sizes, want["sizes"]) and np.array_equal(payload, want["payload"])
    assert [float(k) for k in plan.tables] == want["tables"] == sorted(LAMBS) and plan.max_P == want["max_P"] == 4
    assert plan.M == sizes.size and plan.n_words == payload.size and plan.segment == SEG
    # the fields one by one, against the inputs: P, the palette's rows in the distinct-lambda stack, the class blocks
    assert all(c % 8 == 0 for c in plan.cut[:5])                                   # the class area and the sizes start aligned
    offset = 0
    for f, (pal, m, cl) in enumerate(zip(palettes, mapped, classes)):
        assert desc[f, 7] == len(pal)
        assert desc[f, 8:12].tolist() == [sorted(LAMBS).index(l) for l in pal] + [0] * (4 - len(pal))
        assert desc[f, 13:].tolist() == [0, 0, 0]
        if not m:
            assert desc[f, 12] == -1
            continue
        block = bs.pack_classes(cl)
        assert desc[f, 12] == offset and offset % 8 == 0 and len(block) % 8 == 0
        assert cls[offset: offset + len(block)] == block                       # byte for byte the file's own
        assert block in bytes(files[f])
        assert np.array_equal(bs.unpack_classes(cls[offset: offset + len(block)], cl.size), cl)
        offset += len(block)
    assert offset == plan.cls_bytes


def test_plan_of_files_in_segments_alone_has_no_class_area(world):
    q, files, classes, shapes, palettes, mapped, regions = world
    plan = q._mapped_window_plan([files[1], files[3]], [regions[1], regions[3]], None)
    desc = _parts(plan)[0]
    assert plan.cls_bytes == 0 and plan.max_P == 1 and plan.cut[3] == plan.cut[4]
    assert desc[:, 7].tolist() == [1, 1] and desc[:, 12].tolist() == [-1, -1]
    assert desc[:, 8].tolist() == [1, 0] and [float(k) for k in plan.tables] == [LAMBS[0], LAMBS[3]]
    # the geometry fields are those of the plain plan
    plain = q._window_plan([files[1], files[3]], [regions[1], regions[3]], None)
    assert np.array_equal(desc[:, :7], plain.host[plain.cut[0]:plain.cut[1]].view(np.int64).reshape(2, 8)[:, :7])
    assert plan.n_sel == plain.n_sel and plan.box == plain.box and plan.shape == plain.shape


def test_nothing_to_decode_is_a_plan_without_a_buffer(world):
    q, files, *_ = world
    assert q._mapped_window_plan([], None, None).host is None
    p = q._mapped_window_plan([files[0]], [(S(None), S(2, 2))], None)
    assert p.host is None and p.shape == (1, 1, 0, 9, C_)
    assert q._mapped_window_plan([files[0]], None, []).shape == (1, 1, 6, 9, 0)


def test_expected_output_helper_slices_the_reference_decode(world):
    """The helper the GPU tests compare with: the NumPy coder's decode of the whole file equals the symbols the file was written
    from, and a window of it is a slice."""
    q, _, _, _, _, _, _ = world
    rng = np.random.default_rng(9)
    cls = rng.integers(0, 3, 54).astype(np.uint8)
    data, idx = MW.write_file(q, (1, 6, 9, C_), LAMBS[:3], cls, SEG, rng)
    full = MW.decode_file(q, data)
    assert full.shape == (1, 6, 9, C_) and full.dtype == np.float32
    assert np.array_equal(full, np.take_along_axis(q.code_points_by_channel, idx.astype(np.int64), axis=1).T.reshape(1, 6, 9, C_))
    region = (S(None), S(1, 4), S(2, 9))
    got = MW.expected(q, [data], [region], [2, 0])
    assert np.array_equal(got[0], full[region][..., [2, 0]])
    assert got.shape == q._mapped_window_plan([data], [region], [2, 0]).shape      # what the call returns has this shape


def test_refusals_name_the_file(world, monkeypatch):
    import dataclasses
    q, files, classes, shapes, palettes, mapped, regions = world
    monkeypatch.setattr(type(q), "device", property(lambda self: pytest.fail("the device was asked for")))
    rng = np.random.default_rng(11)
    good, region = files[0], regions[0]
    dig = q._coder_tables(q._lambda_key(LAMBS[0]))[1]
    hc = bs.CompactHeader(N=N, C=C_, shape=(2, 2, C_), lamb=LAMBS[0], digest=dig, n_words=128, part=64)
    compact = bs.write_compact(hc, np.full(hc.n_parts, 128), np.zeros(128, np.uint16))
    with pytest.raises(ValueError, match=r"file 1 is a compact file \(magic b'VBQc'\): its parts are not addressable"):
        q.decompress_latents_mapped_batch([good, compact], region)
    with pytest.raises(ValueError, match="file 0 is a compact file"):
        q.decompress_latents_mapped_window(compact, region)
    other = MW.write_file(q, shapes[0], palettes[0], classes[0], SEG + 1, rng)[0]
    with pytest.raises(ValueError, match=f"file 2 is in segments of {SEG + 1} symbols, file 0 in segments of {SEG}"):
        q.decompress_latents_mapped_batch([good, files[3], other], region)
    # another quantizer's models for ONE lambda: the digest of class 2 of the palette of file 2 alone differs
    q2 = MW.host_quantizer(C_, N, LAMBS)
    q2._code_counts = dict(q2._code_counts)
    q2._code_counts[LAMBS[0]] = q2._code_counts[LAMBS[0]] + 1
    assert palettes[2][2] == LAMBS[0]
    with pytest.raises(ValueError, match=r"file 1 was compressed with a different quantizer or entropy model "
                                         r"\(digest mismatch in class 2 of its palette\)"):
        q2.decompress_latents_mapped_batch([files[1], files[2]], [regions[1], regions[2]])
    with pytest.raises(ValueError, match=r"file 0 was compressed with a different quantizer or entropy model \(digest mismatch\)"):
        q2.decompress_latents_mapped_window(files[3], regions[3])
    assert q2._mapped_window_plan([files[1]], [regions[1]], None).F == 1           # (its other lambdas are q's)
    with pytest.raises(ValueError, match=f"file 0 is for N = {N}, C = {C_}; this quantizer has N = {N}, C = {C_ + 1}"):
        MW.host_quantizer(C_ + 1, N, LAMBS).decompress_latents_mapped_window(good, region)
    with pytest.raises(ValueError, match=f"file 0 is for N = {N}, C = {C_}; this quantizer has N = {N + 1}, C = {C_}"):
        MW.host_quantizer(C_, N + 1, LAMBS).decompress_latents_mapped_batch([files[3], good], region)
    with pytest.raises(ValueError, match="file 1: a region of extents"):
        q.decompress_latents_mapped_batch([good, good], [region, (S(None), S(1, 5), S(2, 8))])
    with pytest.raises(ValueError, match="file 1: a region of extents"):
        q.decompress_latents_mapped_batch([good, files[2]])                      # whole files of two shapes
    with pytest.raises(ValueError, match="2 regions for 1 files"):
        q.decompress_latents_mapped_batch([good], [region, region])
    with pytest.raises(ValueError, match="not a slice"):
        q.decompress_latents_mapped_window(good, (0, S(0, 4)))
    for channels in ([C_], [-1], [0.5]):
        with pytest.raises(ValueError, match=rf"channels must be integers in \[0, {C_}\)"):
            q.decompress_latents_mapped_window(good, region, channels=channels)
    with pytest.raises(ValueError, match="file 1: truncated"):
        q.decompress_latents_mapped_batch([good, good[:-2]], region)
    with pytest.raises(ValueError, match="file 0: not a VBQ bitstream"):
        q.decompress_latents_mapped_window(b"nope" + good[4:], region)
    bad_class = bytearray(good)                                                  # class 3 in a palette of 2
    bad_class[bs.parse_mapped(good)[0].nbytes] |= 3
    with pytest.raises(ValueError, match="file 1: class 3 at position 0 is not below P = 2"):
        q.decompress_latents_mapped_batch([good, bytes(bad_class)], region)
    with pytest.raises(KeyError):
        d = bytearray(good)
        d[24:32] = np.float64(3.0).tobytes()                                     # class 0 of the palette: no model for lambda 3
        q.decompress_latents_mapped_window(bytes(d), region)
    # the calls for files in segments alone still refuse a lambda-map file
    with pytest.raises(ValueError, match=r"file 0 is a lambda-map file \(magic b'VBQm'\): it has a table per symbol"):
        q.decompress_latents_window(good, region)


def test_the_entry_point_is_declared_exported_and_bound():
    import os
    import re
    import subprocess
    from vbq_amd import _lib, build
    name = "vbq_rans_map_decode_window_f32"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "vbq.h")).read()
    assert "Mapped window decode" in text
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", build.build_hip()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT " + name + r"\b", exported)
    decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
    assert len(_lib.SIGNATURES[name][1]) == decl.count(",") + 1 == 26
    assert _lib.lib().vbq_abi_version() == 5                                     # added without a bump


def test_the_c_call_checks_its_arguments_before_any_device_work():
    from vbq_amd import _lib
    h = _lib.lib()
    p = C.c_void_p(64)                    # never dereferenced: every call below returns before any device work
    err = lambda: h.vbq_last_error().decode()                                    # noqa: E731

    def win(payload=p, n_words=10, sizes=p, offs=p, M=4, files=p, F=1, segs=p, n_sel=1, ch=None, n_ch_sel=2, n_ch=2, seg=64,
            N=10, freq=p, n_tables=1, values=p, cls=p, cls_bytes=8, max_P=4, w=(1, 1, 1), out=None, st=None):
        return h.vbq_rans_map_decode_window_f32(payload, n_words, sizes, offs, M, files, F, segs, n_sel, ch, n_ch_sel, n_ch, seg,
                                                N, freq, n_tables, values, cls, cls_bytes, max_P, w[0], w[1], w[2], out, st, None)

    assert win() == -1 and "vbq_rans_map_decode_window_f32: null pointer" in err()     # the sizes pass: the pointers are next
    for kw in (dict(F=65536), dict(F=-1), dict(ch=p, n_ch_sel=65536), dict(n_ch_sel=-1), dict(seg=0), dict(seg=65534), dict(N=0),
               dict(N=11), dict(n_words=-1), dict(M=-1), dict(n_sel=-1), dict(n_ch=0), dict(n_tables=0), dict(w=(-1, 1, 1)),
               dict(w=(1, -1, 1)), dict(w=(1, 1, -1))):
        assert win(out=p, **kw) == -1 and "vbq_rans_map_decode_window_f32: bad sizes" in err(), (kw, err())
    for max_P in (0, 5, -1):
        assert win(out=p, max_P=max_P) == -1 and f"max_classes = {max_P} outside [1, 4]" in err()
    for cls_bytes in (-8, 4, 9):
        assert win(out=p, cls_bytes=cls_bytes) == -1 and "cls_bytes" in err() and "multiple of 8" in err()
    assert win(F=65535, ch=p, n_ch_sel=65535, seg=65533, max_P=1) == -1 and "null pointer" in err()   # the limits themselves pass
    assert win(out=p, n_ch_sel=1) == -1 and "without d_channels" in err()
    assert win(out=p, w=(1 << 31, 1 << 31, 1 << 31)) == -1 and "too large" in err()
    assert win(out=p, F=4, w=(1 << 20, 1 << 20, 1 << 18)) == -1 and "too large" in err()          # 2^63 bytes
    for kw in (dict(sizes=None), dict(offs=None), dict(files=None), dict(segs=None), dict(freq=None), dict(values=None)):
        assert win(out=p, **kw) == -1 and "null pointer" in err(), kw
    assert win(out=p, payload=None) == -1 and "null d_payload" in err()
    assert win(out=p, cls=None) == -1 and "null d_cls" in err()
    assert win(out=p, cls=C.c_void_p(68)) == -1 and "not aligned to 8 bytes" in err()
    # nothing to do: VBQ_OK with no launch, whatever the pointers -- but the sizes are still checked
    nothing = dict(payload=None, sizes=None, offs=None, files=None, segs=None, freq=None, values=None, cls=None)
    for kw in (dict(F=0), dict(n_sel=0), dict(ch=p, n_ch_sel=0), dict(n_ch_sel=0), dict(w=(0, 1, 1)), dict(w=(1, 0, 1)),
               dict(w=(1, 1, 0))):
        assert win(**nothing, **kw) == 0, kw
        assert win(**nothing, **kw, N=11) == -1 and "bad sizes" in err(), kw
        assert win(**nothing, **kw, max_P=5) == -1 and "max_classes" in err(), kw
    # every status bit the kernel can set has a message
    from vbq_amd import coder
    for bit in (1, 2, 4, 8, 16, 32, 64, 128):
        with pytest.raises(_lib.VBQError) as e:
            coder._raise_status(bit)
        assert str(e.value) != "rANS bitstream rejected: ", bit
