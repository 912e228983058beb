"""The host side of the compact batch calls (compress_latents_to_compact_batch / decompress_latents_compact_batch):
bitstream.compact_plan against a brute-force restatement, the argument validation of the three vbq_rans_il_*_files_u16 entry
points through the built library, and the quantizer's checks that raise before any device work.  No GPU is needed."""
import dataclasses

import numpy as np
import pytest

from vbq_amd import bitstream as bs


def brute_plan(rows, tables, parts, C, n_tables):
    """compact_plan restated with Python loops."""
    F = len(rows)
    n_parts = [-(-C * rows[f] // parts[f]) for f in range(F)]
    part_base, P_all, items = [], 0, []
    for f in range(F):
        part_base.append(P_all)
        P_all += n_parts[f]
        items += [(f, p) for p in range(n_parts[f])]
    row0, group_rows = [0] * F, [0] * n_tables
    for t in range(n_tables):
        for f in range(F):
            if tables[f] == t:
                row0[f] = group_rows[t]
                group_rows[t] += -(-rows[f] // 8) * 8
    group_row_base = [sum(group_rows[:t]) for t in range(n_tables)]
    files = [(C * group_row_base[tables[f]] + row0[f], group_rows[tables[f]], rows[f], part_base[f], tables[f], parts[f], 0, 0)
             for f in range(F)]
    return n_parts, part_base, P_all, row0, group_rows, group_row_base, files, items


def _cases():
    # files of 1 row, rows not a multiple of 8, a part larger than the file, part = 1, two tables in mixed order (table 2 unused)
    yield "mixed", [1, 13, 8, 100, 1, 77], [1, 0, 1, 0, 0, 1], [64, 1000, 1, 7, 1 << 24, 50], 3, 3
    yield "one-file", [5], [0], [4], 2, 1
    yield "part-1", [3, 1], [0, 0], [1, 1], 2, 1
    yield "no-files", [], [], [], 3, 0


@pytest.mark.parametrize("case", list(_cases()), ids=lambda c: c[0])
def test_compact_plan_matches_the_brute_force(case):
    _, rows, tables, parts, C, n_tables = case
    p = bs.compact_plan(rows, tables, parts, C, n_tables)
    n_parts, part_base, P_all, row0, group_rows, group_row_base, files, items = brute_plan(rows, tables, parts, C, n_tables)
    assert p.n_parts.tolist() == n_parts and p.part_base.tolist() == part_base and p.P_all == P_all
    assert p.row0.tolist() == row0 and p.group_rows.tolist() == group_rows and p.group_row_base.tolist() == group_row_base
    assert p.n_rows == sum(group_rows)
    assert p.files.dtype == np.int64 and p.files.shape == (len(rows), 8) and [tuple(r) for r in p.files.tolist()] == files
    assert p.items.dtype == np.int32 and p.items.shape == (len(items), 2) and [tuple(r) for r in p.items.tolist()] == items


def test_compact_plan_shares_the_row_layout_of_encode_plan():
    """The quantizer's staging helpers serve both plans: same rows in the same places, same first five descriptor fields but
    for part_base in the place of seg_base.  One part for all files may be given as a scalar."""
    _, rows, tables, _, C, n_tables = next(_cases())
    c = bs.compact_plan(rows, tables, 64, C, n_tables)
    e = bs.encode_plan(rows, tables, 64, C, n_tables)
    for name in ("row0", "group_rows", "group_row_base"):
        assert np.array_equal(getattr(c, name), getattr(e, name)), name
    assert c.n_rows == e.n_rows
    assert np.array_equal(c.files[:, [0, 1, 2, 4]], e.files[:, [0, 1, 2, 4]])
    assert c.files[:, 5].tolist() == [64] * len(rows)
    assert c.n_parts.tolist() == [-(-C * n // 64) for n in rows]
    # every (file, part) exactly once, in file order, no padding
    assert c.items.shape[0] == c.P_all and c.items[:, 0].tolist() == sorted(c.items[:, 0].tolist()) and int(c.items.min()) >= 0


def test_compact_plan_refusals():
    for rows, tables, parts, C, match in (([4], [0], 0, 2, "part 0"), ([4], [0], (1 << 24) + 1, 2, "part"),
                                          ([4, 4], [0, 0], [8, -1], 2, "part -1"), ([4], [0], [8, 8], 2, "parts for"),
                                          ([4], [0], 8, 0, "channels"), ([4, 0], [0, 0], 8, 2, "file 1 has no rows"),
                                          ([4], [0, 1], 8, 2, "tables for"), ([4], [-1], 8, 2, "table outside"),
                                          ([1] * 65536, [0] * 65536, 8, 1, "65536 files")):
        with pytest.raises(ValueError, match=match):
            bs.compact_plan(rows, tables, parts, C)
    with pytest.raises(ValueError, match="table outside"):
        bs.compact_plan([4], [2], 8, 2, n_tables=2)


NAMES = ("vbq_rans_il_sizes_files_u16", "vbq_rans_il_encode_files_u16", "vbq_rans_il_decode_files_u16")


def test_the_three_entry_points_are_declared_exported_and_bound():
    import os
    import re
    import subprocess
    from vbq_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "vbq.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", build.build_hip()], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert re.search(r"\bT " + name + r"\b", exported), name
        assert name in _lib.SIGNATURES
        # one ctypes argument per parameter of the declaration
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(_lib.SIGNATURES[name][1]) == decl.count(",") + 1, name
    assert _lib.lib().vbq_abi_version() == 5                      # added without a bump


def test_argument_validation_of_the_compact_batch_entry_points():
    """Sizes and pointers are checked before any device work: callable on a CPU-only host."""
    import ctypes as C
    from vbq_amd import _lib, build
    build.build_hip()
    h = _lib.lib()
    one = C.c_void_p(8)                                           # a non-null pointer that a refused call never follows
    head = dict(d_idx=one, n_idx=100, d_files=one, n_files=1, d_items=one, n_items=3, n_ch=2, N=10, d_freq=one, n_tables=1)
    good = {
        NAMES[0]: dict(head, d_canon=None, d_sizes=one, P_all=4, d_status=None, stream=None),
        NAMES[1]: dict(head, d_canon=None, d_sizes=one, d_offsets=one, P_all=4, d_payload=one, n_words=600, d_status=None,
                       stream=None),
        NAMES[2]: dict(d_payload=one, n_words=600, d_sizes=one, d_offsets=one, P_all=4, d_files=one, n_files=1, d_items=one,
                       n_items=3, n_ch=2, N=10, d_freq=one, n_tables=1, d_idx=one, n_idx=100, d_status=None, stream=None),
    }
    for name in NAMES:
        def call(**kw):
            a = dict(good[name], **kw)
            return getattr(h, name)(*[a[k] for k in good[name]])

        sizes = [dict(n_files=65536), dict(n_files=-1), dict(n_ch=0), dict(n_ch=65536), dict(N=0), dict(N=11), dict(n_tables=0),
                 dict(n_idx=-1), dict(n_items=-1), dict(P_all=-1), dict(n_items=1 << 31)]
        if "n_words" in good[name]:
            sizes.append(dict(n_words=-1))
        for kw in sizes:
            assert call(**kw) == -1, (name, kw)
            assert name.encode() in h.vbq_last_error() and b"null pointer" not in h.vbq_last_error(), (name, kw)
        may_be_null = {"d_canon", "d_status"}
        for k in good[name]:
            if k.startswith("d_") and k not in may_be_null:
                assert call(**{k: None}) == -1, (name, k)
                assert name.encode() in h.vbq_last_error() and b"null pointer" in h.vbq_last_error(), (name, k)
        # nothing to do: no launch, whatever the pointers
        assert call(n_files=0) == 0 and call(n_items=0) == 0, name
        assert call(n_files=0, **{k: None for k in good[name] if k.startswith("d_")}) == 0, name


# ---------------------------------------------------------------------------------------------- the quantizer's own checks
N, C_ = 4, 3
LAMBS = [0.25, 2.0]


def _quantizer(sigma):
    """Code points and entropy models installed from arrays: nothing here touches a device."""
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    q = ChannelwisePriorCDFQuantizer(C_, N)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C_), np.asarray(sigma)))
    T = q.quantization_levels
    rng = np.random.default_rng(0)
    counts = {lamb: rng.integers(0, 50, (C_, T)) for lamb in LAMBS}
    q._code_counts, q._add_n_smoothing = counts, 1
    q.entropy_models = {lamb: -np.log2((c + 1) / (c + 1).sum(axis=1, keepdims=True)).astype(np.float32) for lamb, c in counts.items()}
    return q


@pytest.fixture(scope="module")
def quantizer():
    return _quantizer([0.5, 1.0, 2.0])


def _pair(shape):
    return np.zeros(shape, np.float32), np.zeros(shape, np.float32)


def _file(q, cls=bs.CompactHeader, shape=(2, 2, C_), lamb=LAMBS[0], **unit):
    """A well-formed file of q written on the host: sizes of the smallest parts / segments and a payload of zeros (nothing
    here decodes it)."""
    dig = q._coder_tables(q._lambda_key(lamb))[1]
    if cls is bs.CompactHeader:
        h = cls(N=N, C=C_, shape=shape, lamb=lamb, digest=dig, n_words=0, **(unit or dict(part=5)))
        sizes = np.full(h.n_parts, 128)
        h = dataclasses.replace(h, n_words=int(sizes.sum()))
        return bs.write_compact(h, sizes, np.zeros(int(sizes.sum()), np.uint16))
    h = cls(N=N, C=C_, shape=shape, lamb=lamb, digest=dig, n_words=0, segment=8)
    sizes = np.full(h.n_sizes, 2)
    h = dataclasses.replace(h, n_words=int(sizes.sum()))
    return bs.write(h, sizes, np.zeros(int(sizes.sum()), np.uint16))


def test_no_files_is_an_empty_list(quantizer):
    assert quantizer.compress_latents_to_compact_batch([], LAMBS[0]) == []
    assert quantizer.compress_latents_to_compact_batch([], []) == []
    assert quantizer.compress_to_compact_batch([], None, LAMBS[0]) == []
    assert quantizer.decompress_latents_compact_batch([], stack=False) == []


def test_writer_errors_are_raised_before_any_device_work(quantizer, monkeypatch):
    q = quantizer
    monkeypatch.setattr(type(q), "device", property(lambda self: pytest.fail("the device was asked for")))
    good = _pair((1, 4, 5, C_))
    for bad, match in ((_pair((1, 4, 5, C_ + 1)), "file 1: expected channel-last"),
                       ((good[0], np.zeros((1, 4, 6, C_), np.float32)), "file 1: expected channel-last"),
                       (_pair(()), "file 1: expected channel-last"), ((good[0],), "file 1: expected a pair"),
                       (_pair((1, 0, 5, C_)), "file 1: empty latent shape")):
        with pytest.raises(ValueError, match=match):
            q.compress_latents_to_compact_batch([good, bad], LAMBS[0])
    for part in (0, -3, (1 << 24) + 1):
        with pytest.raises(ValueError, match="part"):
            q.compress_latents_to_compact_batch([good], LAMBS[0], part=part)
    with pytest.raises(ValueError, match="1 lambdas for 2 files"):
        q.compress_latents_to_compact_batch([good, good], [LAMBS[0]])
    with pytest.raises(ValueError, match="3 lambdas for 2 files"):
        q.compress_latents_to_compact_batch([good, good], LAMBS + LAMBS[:1])
    with pytest.raises(KeyError):
        q.compress_latents_to_compact_batch([good, good], [LAMBS[0], 3.0])

    class Vae:
        def encode(self, X):
            return _pair((1, 2, 2, C_ + 1))
    with pytest.raises(ValueError, match="file 0: expected channel-last"):
        q.compress_to_compact_batch([None], Vae(), LAMBS[1])
    # the segment batch calls still take no layout and no part
    with pytest.raises(TypeError):
        q.compress_latents_to_bytes_batch([good], LAMBS[0], layout="interleaved")


def test_reader_errors_are_raised_before_any_device_work(quantizer, monkeypatch):
    q = quantizer
    good = _file(q)
    other = _file(_quantizer([0.5, 1.0, 3.0]))
    monkeypatch.setattr(type(q), "device", property(lambda self: pytest.fail("the device was asked for")))
    segments = _file(q, bs.Header)
    mapped = bs.MAPPED_MAGIC + bytes(60)
    for files, match in (([good, segments], r"file 1 is a file in segments \(magic b'VBQb'\)"),
                         ([good, good, mapped], r"file 2 is a lambda-map file \(magic b'VBQm'\)"),
                         ([good, good[:-2]], "file 1: truncated"), ([good[:20]], "file 0: truncated"),
                         ([good, good + b"\0\0"], "file 1: 2 trailing bytes"),
                         ([good, b"nope" + good[4:]], "file 1: not a compact VBQ bitstream"),
                         ([good, other], "file 1 was compressed with a different quantizer"),
                         ([good, _file(q, shape=(4, C_))], r"file 1 has latent shape \(4, 3\), file 0 has \(2, 2, 3\)")):
        with pytest.raises(ValueError, match=match):
            q.decompress_latents_compact_batch(files)
    with pytest.raises(KeyError):
        q.decompress_latents_compact_batch([good, good[:16] + np.float64(3.0).tobytes() + good[24:]])     # lambda 3.0: no model
    # the batch calls for files in segments keep refusing a compact file in so many words
    with pytest.raises(ValueError, match="file 0 is a compact file"):
        q.decompress_latents_batch([good])
