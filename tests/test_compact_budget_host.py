"""The host side of the byte-budget calls over compact batches: bitstream.compact_file_words against a plain loop, and the
declaration, export, binding and argument validation of vbq_rans_il_rates_files_u16 through the built library.  No GPU is
needed."""
import numpy as np
import pytest

from vbq_amd import bitstream as bs

NAME = "vbq_rans_il_rates_files_u16"


def loop_words(sizes, plan):
    """compact_file_words restated with Python loops."""
    sizes = np.asarray(sizes)
    out = np.zeros(sizes.shape[:-1] + (len(plan.n_parts),), np.int64)
    for lead in np.ndindex(*sizes.shape[:-1]):
        for f in range(len(plan.n_parts)):
            p0 = int(plan.part_base[f])
            out[lead + (f,)] = sum(int(s) for s in sizes[lead][p0:p0 + int(plan.n_parts[f])])
    return out


@pytest.mark.parametrize("rows,parts,C", [([5], 1 << 17, 3),                         # one file of one part
                                          ([100, 777, 1], [1000, 64, 64], 3),         # differing parts: 1, 37 and 1 parts
                                          ([13, 8, 1, 77], 50, 4)],
                         ids=["one-part", "parts-differ", "same-part"])
def test_compact_file_words_matches_a_plain_loop(rows, parts, C):
    plan = bs.compact_plan(rows, [0] * len(rows), parts, C, 1)
    rng = np.random.default_rng(len(rows))
    for lead in ((), (3,), (2, 3)):                               # no lambda axis, one, and two leading axes
        # sizes near 2^32 / 4: the sums of a file's parts leave u32, so the result must be taken in int64
        sizes = rng.integers(128, 1 << 30, lead + (plan.P_all,), dtype=np.uint32)
        got = bs.compact_file_words(sizes, plan)
        assert got.dtype == np.int64 and got.shape == lead + (len(rows),)
        assert np.array_equal(got, loop_words(sizes, plan))
    if len(rows) == 1:
        assert plan.P_all == 1 and bs.compact_file_words(np.array([131], np.uint32), plan).tolist() == [131]
    if isinstance(parts, list):
        assert plan.n_parts.tolist() == [1, 37, 1]
        ones = bs.compact_file_words(np.ones((2, plan.P_all), np.uint32), plan)
        assert ones.tolist() == [[1, 37, 1]] * 2


def test_compact_file_words_refuses_sizes_of_another_plan():
    plan = bs.compact_plan([100, 777], [0, 0], 64, 3, 1)
    for bad in (np.zeros(plan.P_all + 1, np.uint32), np.zeros((plan.P_all, 2), np.uint32), np.zeros(plan.P_all, np.float32),
                np.uint32(3)):
        with pytest.raises(ValueError, match="sizes must be an integer array"):
            bs.compact_file_words(bad, plan)


def test_the_entry_point_is_declared_exported_and_bound():
    import os
    import re
    import subprocess
    from vbq_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "vbq.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", build.build_hip()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\b" + NAME + r"\s*\(", header)
    assert re.search(r"\bT " + NAME + r"\b", exported)
    assert NAME in _lib.SIGNATURES
    decl = re.search(r"\b" + NAME + r"\s*\(([^;]*)\)\s*;", header).group(1)
    assert len(_lib.SIGNATURES[NAME][1]) == decl.count(",") + 1 == 16     # one ctypes argument per parameter
    assert _lib.lib().vbq_abi_version() == 5                      # added without a bump


def test_argument_validation_of_the_entry_point():
    """Sizes and pointers are checked before any device work: callable on a CPU-only host."""
    import ctypes as C
    from vbq_amd import _lib, build
    build.build_hip()
    h = _lib.lib()
    one = C.c_void_p(8)                                           # a non-null pointer that a refused call never follows
    good = dict(d_idx=one, n_idx=100, lambda_stride=25, d_files=one, n_files=1, d_items=one, n_items=3, n_ch=2, N=10,
                d_freq=one, n_lambda=4, d_canon=None, d_sizes=one, P_all=4, d_status=None, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return getattr(h, NAME)(*[a[k] for k in good])

    def refused(what, **kw):
        assert call(**kw) == -1, kw
        msg = h.vbq_last_error()
        assert NAME.encode() in msg and (what in msg), (kw, msg)
        assert (b"null pointer" in msg) == (what == b"null pointer"), (kw, msg)

    for k in good:                                                # a null pointer
        if k.startswith("d_") and k not in ("d_canon", "d_status"):
            refused(b"null pointer", **{k: None})
    refused(b"n_lambda=0", n_lambda=0)
    refused(b"n_lambda=65536", n_lambda=65536, n_idx=1 << 40)
    refused(b"n_lambda=-1", n_lambda=-1)
    refused(b"lambda_stride=-1", lambda_stride=-1)
    # n_lambda * lambda_stride > n_idx: by one, and a pair whose product overflows int64 (4 * 2^62 wraps to 0 <= n_idx)
    refused(b"do not fit", lambda_stride=26)
    refused(b"do not fit", n_lambda=5)
    refused(b"do not fit", n_lambda=4, lambda_stride=1 << 62)
    assert 4 * (1 << 62) % (1 << 64) == 0
    refused(b"do not fit", n_lambda=65535, lambda_stride=(1 << 63) - 1)
    # n_lambda * P_all sizes must be addressable
    refused(b"too many", n_lambda=65535, lambda_stride=0, P_all=1 << 61)
    # what the compact batch checks
    for kw in (dict(n_files=65536), dict(n_files=-1), dict(n_ch=0), dict(n_ch=65536), dict(N=0), dict(N=11), dict(n_idx=-1),
               dict(n_items=-1), dict(P_all=-1), dict(n_items=1 << 31)):
        refused(NAME.encode(), **kw)
    # nothing to do: no launch, whatever the pointers (the planes of `good` fill the array exactly: 4 * 25 == 100)
    assert call(n_files=0) == 0 and call(n_items=0) == 0
    assert call(n_files=0, **{k: None for k in good if k.startswith("d_")}) == 0
    assert call(n_items=0, **{k: None for k in good if k.startswith("d_")}) == 0


def test_the_rate_inputs_keep_their_default(monkeypatch):
    """_rate_batch_inputs gained a layout: without it a segment is checked as before, with "interleaved" a part."""
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    q = ChannelwisePriorCDFQuantizer(3, 4)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(3), np.ones(3)))
    monkeypatch.setattr(type(q), "device", property(lambda self: pytest.fail("the device was asked for")))
    with pytest.raises(ValueError, match="segment"):
        q._rate_batch_inputs([], None, 65534)
    assert q._rate_batch_inputs([], None, 65534, "interleaved") == ([], [], [], 65534)
    with pytest.raises(ValueError, match="part"):
        q._rate_batch_inputs([], None, (1 << 24) + 1, "interleaved")
    assert q.coded_nbytes_compact_batch([]) == [] and q.compress_latents_to_compact_budget_batch([], 100) == []
    assert q.compress_to_compact_budget_batch([], None, []) == []
    with pytest.raises(ValueError, match="no files"):
        q.compress_latents_to_compact_total_budget([], 100)
    with pytest.raises(ValueError, match="1 budgets for 0 files"):
        q.compress_latents_to_compact_budget_batch([], [100])
    with pytest.raises(ValueError, match="at least one byte"):
        q.compress_latents_to_compact_budget_batch([], 0)
