"""The host side of rate control for batches (coded_nbytes_batch, compress_latents_to_budget_batch,
compress_latents_to_total_budget): the argument validation of vbq_rans_sizes_files_u16 through the built library,
bitstream.smallest_rates_within against the loop of smallest_rate_within, and the quantizer's checks that raise before any
device work.  No GPU is needed."""
import numpy as np
import pytest

from vbq_amd import bitstream as bs


def test_argument_validation_of_the_batch_sizes_call():
    """Sizes and pointers are checked before any device work: callable on a CPU-only host."""
    import ctypes as C
    from vbq_amd import _lib, build
    build.build_hip()
    h = _lib.lib()
    one = C.c_void_p(8)                                           # a non-null pointer that a refused call never follows
    good = dict(d_idx=one, n_idx=300, lambda_stride=100, d_files=one, n_files=1, d_items=one, n_items=64, n_ch=2, seg=64, N=10,
                d_freq=one, n_lambda=3, d_canon=None, d_totals=one, d_status=None, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return h.vbq_rans_sizes_files_u16(*[a[k] for k in good])

    for kw in (dict(n_files=65536), dict(n_ch=65536), dict(seg=0), dict(seg=65534), dict(N=0), dict(N=11), dict(n_lambda=0),
               dict(n_lambda=65536, lambda_stride=0), dict(n_lambda=-1), dict(lambda_stride=-1), dict(n_idx=-1), dict(n_files=-1),
               dict(n_items=-64), dict(n_ch=-1), dict(n_items=63), dict(n_items=65),
               dict(lambda_stride=101), dict(n_idx=299), dict(n_lambda=4), dict(lambda_stride=1 << 62), dict(n_idx=0),
               dict(d_idx=None), dict(d_files=None), dict(d_items=None), dict(d_freq=None), dict(d_totals=None)):
        assert call(**kw) == -1, kw
        assert b"vbq_rans_sizes_files_u16" in h.vbq_last_error(), kw
    assert b"null pointer" in h.vbq_last_error()
    assert call(n_items=63) == -1 and b"multiple of 64" in h.vbq_last_error()
    assert call(lambda_stride=101) == -1 and b"do not fit in n_idx" in h.vbq_last_error()
    # the empty calls: nothing to do, no pointer is looked at
    assert call(n_files=0) == 0 and call(n_items=0) == 0 and call(n_ch=0) == 0
    assert call(n_files=0, d_idx=None, d_files=None, d_items=None, d_freq=None, d_totals=None) == 0
    assert call(n_items=0, d_idx=None, d_files=None, d_items=None, d_freq=None, d_totals=None) == 0
    assert call(n_lambda=65535, lambda_stride=0, n_items=0) == 0                      # the largest n_lambda is accepted


# ------------------------------------------------------------------------------------------------ smallest_rates_within
def _loop(nbytes, budgets, rates):
    return [rates.index(bs.smallest_rate_within(dict(zip(rates, row.tolist())), b)) for row, b in zip(nbytes, budgets)]


def test_smallest_rates_within_equals_the_loop_of_the_one_file_rule():
    rng = np.random.default_rng(5)
    rates = [float(r) for r in 2.0 ** np.arange(-3, 4)]
    for trial in range(30):
        F = int(rng.integers(1, 9))
        nbytes = rng.integers(50, 500, (F, len(rates))).astype(np.int64)                  # no monotone rows at all
        if trial % 2:
            nbytes = -np.sort(-nbytes, axis=1)                                            # falling with the rate, ties included
        lo = nbytes.min(axis=1)
        budgets = [int(b) for b in lo + rng.integers(0, 200, F)]                          # every file has a fit
        got = bs.smallest_rates_within(nbytes, budgets)
        assert got.dtype == np.int64 and got.tolist() == _loop(nbytes, budgets, rates)
        scalar = int(lo.max() + rng.integers(0, 100))
        assert bs.smallest_rates_within(nbytes, scalar).tolist() == _loop(nbytes, [scalar] * F, rates)
        assert bs.smallest_rates_within(nbytes, np.int64(scalar)).tolist() == _loop(nbytes, [scalar] * F, rates)
    # a row that is not monotone: the first column that fits, not the last and not the one with the smallest file
    assert bs.smallest_rates_within(np.array([[90, 40, 70, 30]]), 75).tolist() == [1]
    # a budget equal to a length fits; one byte less does not
    assert bs.smallest_rates_within(np.array([[90, 80, 70]]), 80).tolist() == [1]
    assert bs.smallest_rates_within(np.array([[90, 80, 70]]), 79).tolist() == [2]
    assert bs.smallest_rates_within(np.array([[90, 80, 70], [10, 9, 8]]), [70, 1 << 70]).tolist() == [2, 0]
    assert bs.smallest_rates_within(np.zeros((0, 3), np.int64), 5).tolist() == []
    assert bs.smallest_rates_within(np.zeros((0, 3), np.int64), []).tolist() == []


def test_smallest_rates_within_names_the_first_file_without_a_fit():
    nbytes = np.array([[90, 80, 70], [60, 50, 55], [30, 20, 20], [9, 9, 9]])
    with pytest.raises(ValueError, match=r"file 1: no lambda fits in 49 bytes: the smallest file is 50 bytes, at lambda = column 1"):
        bs.smallest_rates_within(nbytes, [100, 49, 19, 100])
    with pytest.raises(ValueError, match=r"file 2: .* in 19 bytes: the smallest file is 20 bytes, at lambda = 0\.5"):
        bs.smallest_rates_within(nbytes, [100, 50, 19, 1], rates=[0.25, 0.5, 1.0])       # (of equal lengths the smaller rate)
    with pytest.raises(ValueError, match=r"file 0: .* the smallest file is 70 bytes"):
        bs.smallest_rates_within(nbytes, 8)
    # the one-file rule words the same failure the same way
    with pytest.raises(ValueError, match=r"no lambda fits in 49 bytes: the smallest file is 50 bytes, at lambda = 0\.5"):
        bs.smallest_rate_within({0.25: 60, 0.5: 50, 1.0: 55}, 49)


def test_smallest_rates_within_checks_budgets_as_check_budget_does():
    nbytes = np.array([[90, 80, 70], [60, 50, 55]])
    for bad in (80.0, True, "80", None, [80, 80.0], [80, True], [np.float32(80), 80]):
        with pytest.raises(TypeError, match="max_bytes must be an integer"):
            bs.smallest_rates_within(nbytes, bad)
    for bad in (0, -5, [80, 0], [-1, 80]):
        with pytest.raises(ValueError, match="at least one byte"):
            bs.smallest_rates_within(nbytes, bad)
    with pytest.raises(ValueError, match="3 budgets for 2 files"):
        bs.smallest_rates_within(nbytes, [80, 80, 80])
    with pytest.raises(ValueError, match="1 budgets for 2 files"):
        bs.smallest_rates_within(nbytes, [80])
    with pytest.raises(ValueError, match="no candidate lambda"):
        bs.smallest_rates_within(np.zeros((2, 0), np.int64), 80)
    with pytest.raises(ValueError, match=r"integer array \[F, L\]"):
        bs.smallest_rates_within(np.array([90, 80, 70]), 80)
    with pytest.raises(ValueError, match=r"integer array \[F, L\]"):
        bs.smallest_rates_within(np.array([[90.0, 80.0]]), 80)


# ---------------------------------------------------------------------------------------------- the quantizer's own checks
N, C_ = 4, 3
LAMBS = [0.25, 2.0]


@pytest.fixture(scope="module")
def quantizer():
    """Code points and entropy models installed from arrays (as tests/test_encode_files_host.py installs them): nothing here
    touches a device."""
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
    q = quantizer
    assert q.coded_nbytes_batch([]) == [] and q.coded_nbytes_batch([], LAMBS, segment=64) == []
    assert q.compress_latents_to_budget_batch([], 100) == [] and q.compress_latents_to_budget_batch([], [], LAMBS[:1]) == []
    assert q.compress_to_budget_batch([], None, 100) == []
    assert ChannelwisePriorCDFQuantizer(C_, N).coded_nbytes_batch([]) == []              # (no models: nothing to look up)
    with pytest.raises(ValueError, match="no files"):
        q.compress_latents_to_total_budget([], 100)


def test_errors_are_raised_before_any_device_work(quantizer, monkeypatch):
    q = quantizer
    monkeypatch.setattr(type(q), "device", property(lambda self: pytest.fail("the device was asked for")))
    good = _pair((1, 4, 5, C_))
    calls = (lambda lat, **kw: q.coded_nbytes_batch(lat, **kw),
             lambda lat, **kw: q.compress_latents_to_budget_batch(lat, 1000, **kw),
             lambda lat, **kw: q.compress_latents_to_budget_batch(lat, [1000] * len(lat), **kw),
             lambda lat, **kw: q.compress_latents_to_total_budget(lat, 1000, **kw))
    for call in calls:
        for bad, match in ((_pair((1, 4, 5, C_ + 1)), "file 1: expected channel-last"),
                           ((good[0], np.zeros((1, 4, 6, C_), np.float32)), "file 1: expected channel-last"),
                           (_pair(()), "file 1: expected channel-last"), ((good[0],), "file 1: expected a pair"),
                           (_pair((1, 0, 5, C_)), "file 1: empty latent shape")):
            with pytest.raises(ValueError, match=match):
                call([good, bad])
        for segment in (0, -3, 65534):
            with pytest.raises(ValueError, match="segment"):
                call([good], segment=segment)
        with pytest.raises(KeyError):
            call([good, good], lambs=[LAMBS[0], 3.0])
        with pytest.raises(KeyError):
            call([good], lambs=[3.0])
    # the budgets
    with pytest.raises(ValueError, match="1 budgets for 2 files"):
        q.compress_latents_to_budget_batch([good, good], [1000])
    with pytest.raises(ValueError, match="3 budgets for 2 files"):
        q.compress_latents_to_budget_batch([good, good], [1000, 1000, 1000])
    for bad in (1000.0, True, "1000", [1000, 1000.0], [True, 1000]):
        with pytest.raises(TypeError, match="max_bytes must be an integer"):
            q.compress_latents_to_budget_batch([good, good], bad)
    for bad in (1000.0, True, [1000, 1000]):
        with pytest.raises(TypeError, match="max_bytes must be an integer"):
            q.compress_latents_to_total_budget([good, good], bad)
    for bad in (0, [1000, -1]):
        with pytest.raises(ValueError, match="at least one byte"):
            q.compress_latents_to_budget_batch([good, good], bad)
    with pytest.raises(ValueError, match="at least one byte"):
        q.compress_latents_to_total_budget([good], 0)

    class Vae:
        def encode(self, X):
            return _pair((1, 2, 2, C_ + 1))
    with pytest.raises(ValueError, match="file 0: expected channel-last"):
        q.compress_to_budget_batch([None], Vae(), 1000)
    with pytest.raises(TypeError, match="max_bytes must be an integer"):
        q.compress_to_budget_batch([None], Vae(), 1000.0)


def test_the_batch_calls_take_no_layout(quantizer):
    good = _pair((1, 4, 5, C_))
    for call in (quantizer.coded_nbytes_batch, lambda lat, **kw: quantizer.compress_latents_to_budget_batch(lat, 100, **kw),
                 lambda lat, **kw: quantizer.compress_latents_to_total_budget(lat, 100, **kw)):
        with pytest.raises(TypeError, match="layout"):
            call([good], layout="interleaved")
