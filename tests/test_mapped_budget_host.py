"""The host side of byte budgets over lambda maps: bitstream.palette_ladder and bitstream.candidate_chunks, every argument
error of coded_nbytes_mapped_palettes_batch / compress_latents_to_budget_mapped_batch / compress_latents_to_total_budget_mapped
and their one-file and image forms, raised with no device touched, and the ctypes signature and the refusals of
vbq_rans_map_rates_files_u16 through the built library.  No GPU is needed."""
import re

import numpy as np
import pytest

import mapped_window_reference as WR
from vbq_amd import bitstream as bs

NAME = "vbq_rans_map_rates_files_u16"


# ------------------------------------------------------------------------------------------------------------ palette_ladder
def test_palette_ladder_values():
    ladder = [0.25, 0.5, 1.0, 2.0, 4.0]
    assert bs.palette_ladder(ladder, [0, 2]) == [(0.25, 1.0), (0.5, 2.0), (1.0, 4.0)]
    assert bs.palette_ladder(ladder, [2, 0]) == [(1.0, 0.25), (2.0, 0.5), (4.0, 1.0)]            # class 0 the coarser one
    assert bs.palette_ladder(ladder, [0]) == [(l,) for l in ladder]
    assert bs.palette_ladder(ladder, [4]) == [(4.0,)]
    assert bs.palette_ladder(ladder, (1, 0, 4, 2)) == [(0.5, 0.25, 4.0, 1.0)]
    assert bs.palette_ladder(np.array(ladder), np.array([0, 1])) == [(a, b) for a, b in zip(ladder, ladder[1:])]
    out = bs.palette_ladder(range(1, 17), [0, 1])                 # the sixteen-lambda ladder of the issue: 15 candidates
    assert len(out) == 15 and out[0] == (1.0, 2.0) and out[-1] == (15.0, 16.0)
    assert all(isinstance(c, tuple) and all(isinstance(v, float) for v in c) for c in out)


def test_palette_ladder_errors():
    ladder = [0.25, 0.5, 1.0, 2.0, 4.0]
    for steps, match in [([0, 5], "no candidate"), ([5], "no candidate"), ([0, 0], "repeated step"), ([1, 2, 1], "repeated step"),
                         ([0, -1], "negative step"), ([], "0 steps"), ([0, 1, 2, 3, 4], "5 steps"), ([0, 1.5], "integers"),
                         ([0, True], "integers")]:
        with pytest.raises(ValueError, match=match):
            bs.palette_ladder(ladder, steps)
    with pytest.raises(ValueError, match="no candidate"):
        bs.palette_ladder([], [0])
    with pytest.raises(ValueError, match="ascending"):
        bs.palette_ladder([0.5, 0.25, 1.0], [0, 1])
    with pytest.raises(ValueError, match="ascending"):
        bs.palette_ladder([0.5, 0.5, 1.0], [0, 1])


# ---------------------------------------------------------------------------------------------------------- candidate_chunks
def _check_chunks(rows, cap):
    rows = np.asarray(rows)
    chunks = list(bs.candidate_chunks(rows, cap))
    assert [c[0] for c in chunks] == [0] + [c[1] for c in chunks[:-1]] and chunks[-1][1] == len(rows)   # once each, in order
    for k0, k1, tables in chunks:
        assert k1 > k0
        assert tables == sorted(set(rows[k0:k1].reshape(-1).tolist()))
        assert len(tables) <= cap or k1 == k0 + 1                # over the cap only as one candidate alone
    for (k0, k1, tables), nxt in zip(chunks, chunks[1:]):         # greedy: the next candidate did not fit
        assert len(set(tables) | set(rows[nxt[0]].tolist())) > cap
    return chunks


def test_candidate_chunks_cover_every_candidate_in_order():
    ladder2 = [[j, j + 1] for j in range(15)]
    assert _check_chunks(ladder2, 16) == [(0, 15, list(range(16)))]
    assert _check_chunks(ladder2, 1 << 40) == [(0, 15, list(range(16)))]
    assert [(a, b) for a, b, _ in _check_chunks(ladder2, 4)] == [(0, 3), (3, 6), (6, 9), (9, 12), (12, 15)]
    assert _check_chunks(ladder2, 4)[1][2] == [3, 4, 5, 6]
    assert [(a, b) for a, b, _ in _check_chunks(ladder2, 2)] == [(j, j + 1) for j in range(15)]
    # cap 1 with P = 2: a candidate alone brings two tables, and still every chunk holds one
    one = _check_chunks(ladder2, 1)
    assert [(a, b) for a, b, _ in one] == [(j, j + 1) for j in range(15)] and all(len(t) == 2 for _, _, t in one)
    assert _check_chunks(ladder2, 0) == one
    # candidates that share tables, (a, b) next to (b, a), P = 4, P = 1
    assert _check_chunks([[0, 1], [1, 0], [0, 1], [2, 3], [3, 2], [0, 3]], 2) == [(0, 3, [0, 1]), (3, 5, [2, 3]), (5, 6, [0, 3])]
    _check_chunks([[0, 1, 2, 3], [1, 2, 3, 4], [9, 8, 7, 6], [0, 9, 1, 8]], 5)
    assert _check_chunks([[3], [3], [1], [3]], 1) == [(0, 2, [3]), (2, 3, [1]), (3, 4, [3])]
    rng = np.random.default_rng(5)
    for cap in (1, 2, 3, 5, 8):
        _check_chunks(np.stack([rng.permutation(9)[:3] for _ in range(40)]), cap)
    assert list(bs.candidate_chunks(np.zeros((0, 2), np.int64), 4)) == []
    with pytest.raises(ValueError, match=r"\[K, P\]"):
        list(bs.candidate_chunks([0, 1, 2], 4))


# ------------------------------------------------------------------------------------------------------ the library's entry
def test_signature_agrees_with_the_header():
    """One ctypes argument per declared parameter, pointers where the header has pointers; the header has the section."""
    import ctypes as C
    import os
    from vbq_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vbq.h")).read()
    assert " * Mapped batch rates:" in text
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    params = [p.strip() for p in re.search(NAME + r"\s*\(([^)]*)\)", src).group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "d_idx", "n_idx", "lambda_stride", "d_cls", "n_cls", "d_files", "n_files", "d_palettes", "n_palettes", "max_classes",
        "d_items", "n_items", "n_ch", "seg", "N", "d_freq", "n_lambda", "d_canon", "d_totals", "d_status", "stream"]
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is C.c_int and len(argtypes) == len(params)
    for p, t in zip(params, argtypes):
        assert t is (C.c_void_p if "*" in p else kinds[p.split()[0]]), p


def test_argument_validation_of_the_rates_entry():
    """Sizes and pointers are checked before any device work: callable on a CPU-only host."""
    import ctypes as C
    from vbq_amd import _lib, build
    build.build_hip()
    h = _lib.lib()
    one = C.c_void_p(8)                                           # a non-null pointer that a refused call never follows
    good = dict(d_idx=one, n_idx=100, lambda_stride=50, d_cls=one, n_cls=50, d_files=one, n_files=1, d_palettes=one, n_palettes=3,
                max_classes=2, d_items=one, n_items=64, n_ch=2, seg=64, N=10, d_freq=one, n_lambda=2, d_canon=None, d_totals=one,
                d_status=None, stream=None)
    pointers = [k for k in good if k.startswith("d_") and k not in ("d_canon", "d_status")]
    assert pointers == ["d_idx", "d_cls", "d_files", "d_palettes", "d_items", "d_freq", "d_totals"]

    def call(**kw):
        a = dict(good, **kw)
        return getattr(h, NAME)(*[a[k] for k in good])

    for kw in [dict(n_items=63), dict(n_items=65), dict(n_items=-64), dict(n_palettes=0), dict(n_palettes=-1), dict(n_palettes=65536),
               dict(seg=65534), dict(seg=0), dict(N=11), dict(N=0), dict(n_files=65536), dict(n_files=-1), dict(n_ch=65536),
               dict(n_ch=-1), dict(n_lambda=0), dict(n_lambda=65536), dict(n_idx=-1), dict(n_cls=-1), dict(lambda_stride=-1),
               dict(max_classes=0), dict(max_classes=5),
               dict(lambda_stride=51), dict(n_lambda=3), dict(n_idx=99), dict(lambda_stride=1 << 62, n_lambda=4)] + \
              [{k: None} for k in pointers]:
        assert call(**kw) == -1, kw
        assert NAME.encode() in h.vbq_last_error(), kw
    assert b"null pointer" in h.vbq_last_error()
    assert call(n_items=63) == -1 and b"multiple of 64" in h.vbq_last_error()
    assert call(n_palettes=0) == -1 and b"n_palettes=0" in h.vbq_last_error()
    assert call(lambda_stride=51) == -1 and b"do not fit in n_idx=100" in h.vbq_last_error()
    # nothing to do: VBQ_OK without a launch, whatever the pointers
    assert call(n_files=0) == 0 and call(n_items=0) == 0 and call(n_ch=0) == 0
    assert call(n_files=0, **{k: None for k in pointers}) == 0
    assert call(n_palettes=65535, n_lambda=65535, n_idx=65535, lambda_stride=1, n_files=0) == 0


# ---------------------------------------------------------------------------------------------- the quantizer's own checks
N, C_ = 4, 3
LAMBS = [0.25, 0.5, 1.0, 2.0, 4.0]


@pytest.fixture(scope="module")
def quantizer():
    return WR.host_quantizer(C_, N, LAMBS)


def _pair(shape):
    return np.zeros(shape, np.float32), np.zeros(shape, np.float32)


class _Vae:
    """A stand-in encoder: `encode(shape)` returns zero latents of that shape."""
    def encode(self, X):
        return _pair(X)


def _forms(q):
    """The four batch-shaped calls as call(latents, palettes, classes, **kw), budgets filled in."""
    return [q.coded_nbytes_mapped_palettes_batch,
            lambda lat, pals, cls, **kw: q.compress_latents_to_budget_mapped_batch(lat, 1000, pals, cls, **kw),
            lambda lat, pals, cls, **kw: q.compress_latents_to_total_budget_mapped(lat, 1000, pals, cls, **kw),
            lambda lat, pals, cls, **kw: q.compress_to_budget_mapped_batch([p[0].shape for p in lat], _Vae(), 1000, pals, cls, **kw)]


def test_no_files(quantizer):
    q = quantizer
    pals = bs.palette_ladder(LAMBS, [0, 1])
    out = q.coded_nbytes_mapped_palettes_batch([], pals, [])
    assert isinstance(out, np.ndarray) and out.shape == (0, 4) and out.dtype == np.int64
    assert q.compress_latents_to_budget_mapped_batch([], 100, pals, []) == []
    assert q.compress_latents_to_budget_mapped_batch([], [], pals, []) == []
    assert q.compress_to_budget_mapped_batch([], None, 100, pals, []) == []
    with pytest.raises(ValueError, match="no files"):
        q.compress_latents_to_total_budget_mapped([], 100, pals, [])
    with pytest.raises(ValueError, match="1 budgets for 0 files"):
        q.compress_latents_to_budget_mapped_batch([], [5], pals, [])


def test_errors_are_raised_before_any_device_work(quantizer, monkeypatch):
    q = quantizer
    monkeypatch.setattr(type(q), "device", property(lambda self: pytest.fail("the device was asked for")))
    good, cls = _pair((1, 4, 5, C_)), np.zeros((1, 4, 5), np.int64)
    pals = [(0.25, 1.0), (0.5, 2.0), (2.0, 0.5)]
    for call in _forms(q):
        with pytest.raises(ValueError, match="palette 0: a palette of 5 lambdas"):
            call([good, good], [tuple(LAMBS), tuple(LAMBS[::-1])], [cls, cls])
        with pytest.raises(ValueError, match="palette 0: a palette of 0 lambdas"):
            call([good, good], [(), ()], [cls, cls])
        with pytest.raises(ValueError, match="palette 2: repeated lambda"):
            call([good, good], pals[:2] + [(0.5, 0.5)], [cls, cls])
        with pytest.raises(KeyError, match="palette 1: .*3.0"):
            call([good, good], [pals[0], (0.25, 3.0)], [cls, cls])
        with pytest.raises(ValueError, match="palette 2: 1 lambdas, palette 0 has 2"):
            call([good, good], pals[:2] + [(0.5,)], [cls, cls])
        with pytest.raises(ValueError, match="no candidate palette"):
            call([good, good], [], [cls, cls])
        with pytest.raises(ValueError, match="sequence of candidate palettes"):
            call([good, good], [0.25, 1.0], [cls, cls])           # one palette is not a list of candidates
        with pytest.raises(ValueError, match=r"file 1: class outside \[0, 2\)"):
            call([good, good], pals, [cls, cls + 2])
        with pytest.raises(ValueError, match=r"file 0: class outside \[0, 2\)"):
            call([good, good], pals, [cls - 1, cls])
        with pytest.raises(ValueError, match="file 1: classes of shape"):
            call([good, good], pals, [cls, np.zeros((1, 4, 6), np.int64)])
        with pytest.raises(ValueError, match="file 1: classes must be integers"):
            call([good, good], pals, [cls, cls.astype(np.float32)])
        with pytest.raises(ValueError, match="1 class maps for 2 files"):
            call([good, good], pals, [cls])
        with pytest.raises(ValueError, match="file 1: expected channel-last"):
            call([good, _pair((1, 4, 5, C_ + 1))], pals, [cls, cls])
        for segment in (0, 65534):
            with pytest.raises(ValueError, match="segment"):
                call([good], pals, [cls], segment=segment)
    with pytest.raises(ValueError, match="file 1: expected a pair"):
        q.coded_nbytes_mapped_palettes_batch([good, 5], pals, [cls, cls])
    with pytest.raises(ValueError, match="65536 files"):
        q.coded_nbytes_mapped_palettes_batch([good] * 65536, pals, [cls] * 65536)
    # the budgets
    for bad, exc in [(0, ValueError), (-3, ValueError), (2.5, TypeError), (True, TypeError), ([100, 0], ValueError),
                     ([100, 2.5], TypeError)]:
        with pytest.raises(exc, match="max_bytes"):
            q.compress_latents_to_budget_mapped_batch([good, good], bad, pals, [cls, cls])
    with pytest.raises(ValueError, match="3 budgets for 2 files"):
        q.compress_latents_to_budget_mapped_batch([good, good], [100, 100, 100], pals, [cls, cls])
    for bad, exc in [(0, ValueError), (2.5, TypeError), ([100, 100], TypeError)]:
        with pytest.raises(exc, match="max_bytes"):
            q.compress_latents_to_total_budget_mapped([good, good], bad, pals, [cls, cls])
        with pytest.raises(exc, match="max_bytes"):
            q.compress_latents_to_budget_mapped(good[0], good[1], bad, pals, cls)
        with pytest.raises(exc, match="max_bytes"):
            q.compress_to_budget_mapped((1, 4, 5, C_), _Vae(), bad, pals, cls)
    # the one-file and image forms are the F = 1 case: the same errors, file 0
    for call in (lambda p, c: q.coded_nbytes_mapped_palettes(good[0], good[1], p, c),
                 lambda p, c: q.compress_latents_to_budget_mapped(good[0], good[1], 100, p, c),
                 lambda p, c: q.compress_to_budget_mapped((1, 4, 5, C_), _Vae(), 100, p, c)):
        with pytest.raises(ValueError, match="palette 1: repeated lambda"):
            call([pals[0], (1.0, 1.0)], cls)
        with pytest.raises(KeyError, match="palette 0: .*3.0"):
            call([(3.0, 1.0)], cls)
        with pytest.raises(ValueError, match=r"file 0: class outside \[0, 2\)"):
            call(pals, cls + 2)
        with pytest.raises(ValueError, match="no candidate palette"):
            call([], cls)
    with pytest.raises(ValueError, match="file 0: expected channel-last"):
        q.compress_to_budget_mapped((1, 2, 2, C_ + 1), _Vae(), 100, pals, np.zeros((1, 2, 2), np.int64))
