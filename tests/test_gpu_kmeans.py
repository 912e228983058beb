"""The exact 1-D k-means library (include/vbq_kmeans.h, vbq_amd/kmeans) on the device.

vbqk_kmeans1d_f64 against the NumPy restatement tests/kmeans_reference.py ON THE SAME PREFIX SUMS: segment starts, code points,
counts and the whole sse curve by np.array_equal on values or bit patterns.  vbqk_nearest_code_channels_f64 against a loop of
vbq_nearest_code_f64 over the channels, bit for bit.  The two new quantizer classes against the existing wrapper.  The one
comparison with a tolerance (the sum of squares recomputed from the samples) derives it where it stands."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import footprint as FP  # noqa: E402
import kmeans_reference as KR  # noqa: E402
import stream_order as SO  # noqa: E402

gpu = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


@pytest.fixture(scope="module")
def spin():
    _need_gpu()
    sp, notes = SO.calibrate()
    print(f"\n[test_gpu_kmeans] {sp}: {notes}")
    return sp


def _cuda(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------ the references
@functools.lru_cache(maxsize=None)
def _channel(n, c, name=None):
    """(sorted f32 [n], shift, S1, S2) of channel c at size n: family c mod 5 unless named, its own seed; read-only."""
    name = name or KR.FAMILIES[c % len(KR.FAMILIES)]
    x = np.sort(KR.family(name, np.random.default_rng([n, c]), n))
    shift, S1, S2 = KR.sums_of(x)
    for a in (x, S1, S2):
        a.setflags(write=False)
    return x, shift, S1, S2


@functools.lru_cache(maxsize=None)
def _solved(n, c, Kmax, name=None):
    """(sse [Kmax], A) of the restatement; a smaller Kmax is a prefix of a larger one's layers, so tests share the largest."""
    _, _, S1, S2 = _channel(n, c, name)
    sse, A = KR.dp_levels(S1, S2, Kmax)
    sse.setflags(write=False)
    A.setflags(write=False)
    return sse, A


def _want(n, c, Kmax, levels, top=None, name=None):
    x, shift, S1, S2 = _channel(n, c, name)
    sse, A = _solved(n, c, top or Kmax, name)
    return {k: KR.walk(A, S1, S2, shift, k) for k in levels}, sse[:Kmax]


def _inputs(n, C, name=None):
    chans = [_channel(n, c, name) for c in range(C)]
    return (np.stack([ch[2] for ch in chans]), np.stack([ch[3] for ch in chans]), np.array([ch[1] for ch in chans], np.float64))


def _run(S1, S2, shift, levels, **kw):
    from vbq_amd import kmeans1d
    status = torch.zeros(1, dtype=torch.uint32, device="cuda")
    starts, codes, counts, sse = kmeans1d.kmeans1d_dp(_cuda(S1), _cuda(S2), _cuda(shift), levels, status=status, **kw)
    host = lambda ts: [t.cpu().numpy() for t in ts]
    return host(starts), host(codes), host(counts), sse.cpu().numpy(), int(status.cpu().view(torch.int32).item())


def _check(n, C, Kmax, levels, top=None, name=None, **kw):
    S1, S2, shift = _inputs(n, C, name)
    starts, codes, counts, sse, status = _run(S1, S2, shift, levels, **kw)
    assert status == 0 and sse.shape == (C, Kmax)
    for c in range(C):
        want, want_sse = _want(n, c, Kmax, levels, top, name)
        what = f"n={n} C={C} Kmax={Kmax} levels={levels} channel {c}"
        assert np.array_equal(_u64(sse[c]), _u64(want_sse)), what
        for s, k in enumerate(levels):
            assert starts[s].shape == (C, k) and starts[s].dtype == np.int32 and counts[s].dtype == np.int64
            assert np.array_equal(starts[s][c], want[k][0]), what
            assert np.array_equal(_u64(codes[s][c]), _u64(want[k][1])), what
            assert np.array_equal(counts[s][c], want[k][2]), what


def _level_lists(Kmax):
    """A single entry, all of 1..Kmax (at most 64 entries), and a sparse list that ends at Kmax."""
    lists = [[Kmax], list(range(1, Kmax + 1))]
    sparse = sorted({1, max(1, Kmax // 3), max(1, Kmax - 1), Kmax})
    return lists + ([sparse] if sparse not in lists else [])


# ------------------------------------------------------------------------------------------------------------------ the DP
@gpu
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257, 1000])
def test_the_c_call_equals_the_restatement_on_the_same_sums(n):
    """np.cumsum prefix sums in, starts / code points / counts / sse out: the same bits as tests/kmeans_reference.py.  Every
    channel holds another family (normal, quarters with many duplicates, Student-t, all equal, normal + 1000)."""
    _need_gpu()
    top = min(n, 64)
    for Kmax in sorted({k for k in (1, 2, 3, 16, top) if k <= n}):
        for C in (1, 3, 5):
            for levels in _level_lists(Kmax):
                _check(n, C, Kmax, levels, top)


@gpu
@pytest.mark.parametrize("n", [126, 128, 130, KR.ROWS_IN_LDS_MAX_N - 1, KR.ROWS_IN_LDS_MAX_N, KR.ROWS_IN_LDS_MAX_N + 1])
def test_one_below_at_and_one_above_each_threshold_of_the_plan(n):
    """The root of layer 2 scans 63 / 64 / 65 candidates at n = 126 / 128 / 130: by its lane, and from 64 by a whole wave.  The
    value rows and the sums live in LDS up to n = 4862 and in the workspace slice above."""
    _need_gpu()
    assert [KR.root_scan_len(2, m) for m in (126, 128, 130)] == [KR.WAVE_SCAN - 1, KR.WAVE_SCAN, KR.WAVE_SCAN + 1]
    assert KR.rows_in_lds(KR.ROWS_IN_LDS_MAX_N) and not KR.rows_in_lds(KR.ROWS_IN_LDS_MAX_N + 1) and KR.ROWS_IN_LDS_MAX_N == 4862
    from vbq_amd import _lib_kmeans
    assert _lib_kmeans.lib().vbqk_kmeans1d_workspace_bytes(n, 1, 3) == KR.slice_bytes(n, 3)
    if n < 1000:
        _check(n, 3, 4, [1, 2, 4])
    else:
        _check(n, 2, 3, [1, 3])


@gpu
def test_more_long_scans_in_a_round_than_the_queue_holds():
    """Uniform samples, n = 600 000, two levels: depth 12 of layer 2 has 4096 nodes of which more than 2048 scan 64 candidates or
    more.  The nodes the queue does not take are scanned by their lanes, with the same bits."""
    _need_gpu()
    n = 600_000
    x = np.sort(np.random.default_rng(5).uniform(-1, 1, n).astype(np.float32))
    shift, S1, S2 = KR.sums_of(x)
    stats = []
    sse, A = KR.dp_levels(S1, S2, 2, stats=stats)
    assert max(s[3] for s in stats) > KR.QUEUE, max(s[3] for s in stats)
    starts, codes, counts, got_sse, status = _run(S1[None], S2[None], np.array([shift]), [1, 2])
    assert status == 0 and np.array_equal(_u64(got_sse[0]), _u64(sse))
    for s, k in enumerate((1, 2)):
        want = KR.walk(A, S1, S2, shift, k)
        assert np.array_equal(starts[s][0], want[0]) and np.array_equal(_u64(codes[s][0]), _u64(want[1]))
        assert np.array_equal(counts[s][0], want[2])


@gpu
@pytest.mark.parametrize("n", [257, KR.ROWS_IN_LDS_MAX_N + 1])
def test_a_workspace_of_exactly_one_slice_gives_the_same_bits(n):
    """C = 5 channels through one slice: one workgroup takes them one after the other."""
    _need_gpu()
    from vbq_amd import _lib_kmeans
    C, Kmax = 5, 16 if n < 1000 else 3
    h = _lib_kmeans.lib()
    one = h.vbqk_kmeans1d_workspace_bytes(n, 1, Kmax)
    assert one == KR.slice_bytes(n, Kmax) and h.vbqk_kmeans1d_workspace_bytes(n, C, Kmax) == C * one
    ws = FP.guarded_workspace(one, "cuda")
    _check(n, C, Kmax, [1, 2, Kmax], workspace=ws.view)
    torch.cuda.synchronize()
    ws.assert_outside_intact("one-slice workspace")


@gpu
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_channel_with_a_nan_or_an_infinity_sets_status_and_leaves_its_neighbours_exact(bad):
    _need_gpu()
    n, C, Kmax, levels = 257, 3, 16, [1, 5, 16]
    S1, S2, shift = (a.copy() for a in _inputs(n, C))
    x = _channel(n, 1)[0].copy()
    x[100] = bad
    shift[1], S1[1], S2[1] = KR.sums_of(np.sort(x))
    assert not np.isfinite(S2[1, n])
    starts, codes, counts, sse, status = _run(S1, S2, shift, levels)
    assert status == 1
    for c in (0, 2):
        want, want_sse = _want(n, c, Kmax, levels)
        assert np.array_equal(_u64(sse[c]), _u64(want_sse))
        for s, k in enumerate(levels):
            assert np.array_equal(starts[s][c], want[k][0]) and np.array_equal(_u64(codes[s][c]), _u64(want[k][1]))
            assert np.array_equal(counts[s][c], want[k][2])
    for s, k in enumerate(levels):                                    # unspecified, but within bounds
        assert starts[s][1].min() >= 1 and starts[s][1].max() <= n and counts[s][1].min() >= 1 and counts[s][1].max() <= n


# ------------------------------------------------------------------------------------------------------------------ the Python layer
def _samples(B, C, seed=3):
    rng = np.random.default_rng(seed)
    return np.stack([KR.family(KR.FAMILIES[c % 5], rng, B) for c in range(C)], axis=1)


@gpu
@pytest.mark.parametrize("on_device", [False, True])
def test_fit_channels_equals_the_restatement_on_the_sums_it_made(on_device):
    """prefix_sums on the device, read back; the restatement run on exactly those sums; levels out of order with a repeat."""
    _need_gpu()
    from vbq_amd import kmeans1d
    B, C, levels = 300, 5, [6, 2, 17, 2, 1]
    x = _samples(B, C)
    xs, shift, S1, S2 = (t.cpu().numpy() for t in kmeans1d.prefix_sums(_cuda(x) if on_device else x))
    assert np.array_equal(xs, np.sort(x.T, axis=1)) and np.array_equal(shift, xs[:, B // 2].astype(np.float64))
    assert S1.shape == (C, B + 1) and (S1[:, 0] == 0).all() and (S2[:, 0] == 0).all()
    fits = kmeans1d.fit_channels(_cuda(x) if on_device else x, levels, add_n_smoothing=1.0)
    assert len(fits) == len(levels)
    curve = kmeans1d.sse_curve(x, 17)
    for c in range(C):
        sse, A = KR.dp_levels(S1[c], S2[c], 17)
        assert np.array_equal(_u64(curve[c]), _u64(sse))
        for fit, k in zip(fits, levels):
            _, codes, counts = KR.walk(A, S1[c], S2[c], shift[c], k)
            assert fit.code_points.shape == (C, k) and fit.counts.dtype == np.int64
            assert np.array_equal(_u64(fit.code_points[c]), _u64(codes)) and np.array_equal(fit.counts[c], counts)
            assert np.array_equal(_u64(fit.code_lengths[c]), _u64(-np.log2(counts / B)))
    with pytest.raises(ValueError, match="infs or NaNs"):
        bad = x.copy()
        bad[7, 2] = np.nan
        kmeans1d.fit_channels(bad, [2])


@gpu
def test_the_sum_of_squares_recomputed_from_the_samples_agrees_with_sse():
    """Nearest assignment of the f64 samples to the returned code points, squared distances summed in f64 on the host, against
    sse[k - 1], within 4 n eps S2[n]: the rounding of the prefix sums the DP's value carries (derived in
    tests/test_kmeans_host.py).  A sample exactly between two code points may go to either without changing the sum.  Every
    figure is printed before it is held against the bound."""
    _need_gpu()
    from vbq_amd import kmeans1d
    B, C = 1000, 5
    x = _samples(B, C, seed=11)
    levels = [1, 2, 7, 32]
    fits = kmeans1d.fit_channels(x, levels)
    curve = kmeans1d.sse_curve(x, 32)
    _, _, _, S2 = (t.cpu().numpy() for t in kmeans1d.prefix_sums(x))
    for c in range(C):
        xc = x[:, c].astype(np.float64)
        for fit, k in zip(fits, levels):
            d = (xc[:, None] - fit.code_points[c][None, :]) ** 2
            direct = float(np.sort(d.min(axis=1)).sum())
            bound = KR.objective_bound(S2[c], B)
            print(f"channel {c} k={k}: sse {curve[c, k - 1]!r} direct {direct!r} bound {bound!r}")
            assert abs(direct - curve[c, k - 1]) <= bound


# ------------------------------------------------------------------------------------------------------------------ nearest code
def _code_rows(rng, C, k):
    """Code rows on a grid of eighths: sorted in even channels, shuffled in odd ones, with repeated values once k allows."""
    rows = np.sort(rng.integers(-4 * max(2, k // 2), 4 * max(2, k // 2), (C, k)), axis=1) / 8.0
    for c in range(1, C, 2):
        rng.shuffle(rows[c])
    return rows


@gpu
@pytest.mark.parametrize("k", [1, 2, 255, 256, 1024])
def test_nearest_code_of_all_channels_equals_the_loop_over_channels(k):
    """Samples exactly on midpoints of neighbouring codes (a grid of sixteenths, exact in f32), repeated code values, unsorted
    rows, counts added onto counts that are not zero."""
    _need_gpu()
    from vbq_amd import _lib, kmeans1d, ops
    rng = np.random.default_rng(k)
    for B in (1, 63, 64, 65, 1000):
        for C in (1, 3, 64, 65):
            codes = _code_rows(rng, C, k)
            x = (rng.standard_normal((B, C)) * k / 16).astype(np.float32)
            srt = np.sort(codes, axis=1)
            mid = rng.random((B, C)) < 0.4
            at = rng.integers(0, max(1, k - 1), (B, C))
            ch = np.broadcast_to(np.arange(C), (B, C))
            mids = ((srt[ch, at] + srt[ch, np.minimum(at + 1, k - 1)]) / 2).astype(np.float32)
            x = np.where(mid, mids, x)
            dx, dc = _cuda(x), _cuda(codes)
            start = rng.integers(1, 1000, (C, k)).astype(np.int64)
            counts = _cuda(start)
            I, q = kmeans1d.nearest_code_channels(dx, dc, counts=counts)
            want_counts = _cuda(start)
            for c in range(C):
                col = dx[:, c].contiguous()
                wi = torch.empty(B, dtype=torch.int32, device="cuda")
                wq = torch.empty(B, dtype=torch.float64, device="cuda")
                _lib.check(_lib.lib().vbq_nearest_code_f64(ops._ptr(col), B, ops._ptr(dc[c]), k, ops._ptr(wi), ops._ptr(wq),
                                                           ops._ptr(want_counts[c]), ops._stream(col)), "vbq_nearest_code_f64")
                assert torch.equal(I[:, c], wi) and torch.equal(q[:, c].view(torch.int64), wq.view(torch.int64)), (B, C, k, c)
            assert torch.equal(counts, want_counts) and int((counts - _cuda(start)).sum()) == B * C
    assert mid.any() and (k < 255 or (np.diff(srt, axis=1) == 0).any())


# ------------------------------------------------------------------------------------------------------------------ the quantizers
class _StubVAE:
    """Identity-like: the latents are an affine image of X and decode inverts it."""

    def encode(self, X):
        return (np.asarray(X, np.float32) * np.float32(4) - np.float32(2)), None

    def decode(self, Z):
        return (np.asarray(Z, np.float64) + 2) / 4


@gpu
def test_the_wrapper_equals_the_channelwise_wrapper_of_optimal_quantizers():
    _need_gpu()
    import vbq_amd
    from vbq_amd import baselines
    C, levels = 3, [2, 4, 6]
    rng = np.random.default_rng(9)
    X = rng.random((2, 8, 8, C)).astype(np.float32)
    X[0, 0, 0] = [0.5, 1.25, -0.25]                                   # outside [0, 1] after the round trip: clip matters
    vae = _StubVAE()
    new = vbq_amd.ChannelwiseOptimalKmeansWrapper(C, levels)
    old = baselines.ChannelwiseSimpleQuantizerWrapper(vbq_amd.OptimalKmeansQuantizer, C, levels)
    new.fit(X, vae, 1.0)
    old.fit(X, vae, 1.0)
    for l, q in zip(levels, old._quantizers):
        assert np.array_equal(_u64(new.code_points[l]), _u64(q.code_points)) and new.code_points[l].shape == (C, l)
        assert np.array_equal(_u64(new.code_lengths[l]), _u64(q.code_lengths))
    X2 = rng.random((2, 8, 8, C)).astype(np.float32)
    for clip in (True, False):
        a, b = new.compress(X2, vae, levels, clip=clip), old.compress(X2, vae, levels, clip=clip)
        assert sorted(a) == sorted(b) == ["X_hat", "Z_hat", "num_bits"]
        for field in b:
            assert list(a[field]) == list(b[field]) == levels
            for l in levels:
                assert a[field][l].dtype == b[field][l].dtype and a[field][l].shape == b[field][l].shape, (field, l)
                assert a[field][l].tobytes() == b[field][l].tobytes(), (field, l, clip)
    # a single OptimalKmeansQuantizer: the reference's fit / quantize contract, and the optimum is no worse than any other book
    one = vbq_amd.OptimalKmeansQuantizer(4)
    s = vae.encode(X)[0].reshape(-1, C)[:, 1]
    one.fit(s)
    qz, I, nb = one.quantize(s)
    assert qz.shape == I.shape == nb.shape == s.shape and np.array_equal(qz, one.code_points[I])
    assert np.array_equal(nb, one.code_lengths[I]) and (np.diff(one.code_points) > 0).all()


# ------------------------------------------------------------------------------------------------------------------ footprint
@gpu
@pytest.mark.parametrize("offset", [0, 1])
def test_write_footprint(offset):
    """Every output and an exactly sized workspace between canaries, aligned and one element off; a refused call writes nothing."""
    _need_gpu()
    from vbq_amd import _lib_kmeans, ops
    h = _lib_kmeans.lib()
    for n, C, levels in ((65, 3, [1, 4, 9]), (KR.ROWS_IN_LDS_MAX_N + 1, 2, [2, 3])):
        Kmax, S, total = levels[-1], len(levels), C * sum(levels)
        S1, S2, shift = _inputs(n, C)
        d_S1, d_S2, d_shift = (FP.shifted(a, offset, "cuda") for a in (S1, S2, shift))
        wsb = h.vbqk_kmeans1d_workspace_bytes(n, C, Kmax)
        assert wsb == C * KR.slice_bytes(n, Kmax)

        def outputs():
            return [FP.Guarded((total,), torch.int32, "cuda", offset), FP.Guarded((total,), torch.float64, "cuda", offset),
                    FP.Guarded((total,), torch.int64, "cuda", offset), FP.Guarded((C, Kmax), torch.float64, "cuda", offset)]
        g = outputs()
        g_ws = FP.guarded_workspace(wsb, "cuda")
        arr = (ops.C.c_int32 * S)(*levels)
        rc = h.vbqk_kmeans1d_f64(ops._ptr(d_S1), ops._ptr(d_S2), ops._ptr(d_shift), n, C, arr, S, g[0].ptr, g[1].ptr, g[2].ptr,
                                 g[3].ptr, None, g_ws.ptr, wsb, ops._stream(d_S1))
        assert rc == 0, h.vbqk_last_error()
        torch.cuda.synchronize()
        for x, what in zip(g + [g_ws], ("starts", "codes", "counts", "sse", "workspace")):
            x.assert_outside_intact(what)
        for x in g:
            assert (x.bits() != FP.canary(x.dtype)).all(), "an output element was not written"
        at = 0
        for k in levels:
            for c in range(C):
                want, want_sse = _want(n, c, Kmax, levels)
                assert np.array_equal(g[0].host()[at:at + k], want[k][0]) and np.array_equal(g[2].host()[at:at + k], want[k][2])
                assert np.array_equal(_u64(g[1].host()[at:at + k]), _u64(want[k][1]))
                assert np.array_equal(_u64(g[3].host()[c]), _u64(want_sse))
                at += k
        fresh = outputs()
        bad = (ops.C.c_int32 * S)(*([levels[-1]] + levels[1:]))
        rc = h.vbqk_kmeans1d_f64(ops._ptr(d_S1), ops._ptr(d_S2), ops._ptr(d_shift), n, C, bad, S, fresh[0].ptr, fresh[1].ptr,
                                 fresh[2].ptr, fresh[3].ptr, None, g_ws.ptr, wsb, ops._stream(d_S1))
        assert rc == -1 and (S == 1 or b"strictly ascending" in h.vbqk_last_error())
        torch.cuda.synchronize()
        for x in fresh:
            x.assert_untouched("refused fit")
    # the nearest code of all channels: index, value and counts that are added to
    rng = np.random.default_rng(1)
    for B, C, k in ((65, 3, 9), (130, 65, 256)):
        x, codes = rng.standard_normal((B, C)).astype(np.float32), _code_rows(rng, C, k)
        dx, dc = FP.shifted(x, offset, "cuda"), FP.shifted(codes, offset, "cuda")
        gi, gq = FP.Guarded((B, C), torch.int32, "cuda", offset), FP.Guarded((B, C), torch.float64, "cuda", offset)
        gc = FP.Guarded((C, k), torch.int64, "cuda", offset).fill(np.full((C, k), 5, np.int64))
        rc = h.vbqk_nearest_code_channels_f64(ops._ptr(dx), B, C, ops._ptr(dc), k, gi.ptr, gq.ptr, gc.ptr, ops._stream(dx))
        assert rc == 0, h.vbqk_last_error()
        torch.cuda.synchronize()
        for x_, what in ((gi, "index"), (gq, "value"), (gc, "counts")):
            x_.assert_outside_intact(what)
        want_i = np.stack([np.argmin((x[:, c].astype(np.float64)[:, None] - codes[c][None]) ** 2, axis=1) for c in range(C)], 1)
        assert np.array_equal(gi.host(), want_i) and np.array_equal(gq.host(), codes[np.arange(C)[None], want_i])
        assert np.array_equal(gc.host(), 5 + np.stack([np.bincount(want_i[:, c], minlength=k) for c in range(C)]))
        fresh = [FP.Guarded((B, C), torch.int32, "cuda", offset), FP.Guarded((B, C), torch.float64, "cuda", offset)]
        assert h.vbqk_nearest_code_channels_f64(ops._ptr(dx), B, C, ops._ptr(dc), 1025, fresh[0].ptr, fresh[1].ptr, None,
                                                ops._stream(dx)) == -1
        torch.cuda.synchronize()
        for x_ in fresh:
            x_.assert_untouched("refused nearest code")


# ------------------------------------------------------------------------------------------------------------------ stream order
@gpu
def test_fit_channels_is_ordered_on_the_callers_stream(spin):
    """Late samples on a side stream, the exact answer.  Blocking: fit_channels reads its status word and hands out NumPy
    arrays; the sort, the sums and the DP are enqueued while the delay runs."""
    _need_gpu()
    from vbq_amd import kmeans1d

    def late(seed):
        return [_cuda(np.random.default_rng(seed).standard_normal((200, 3)).astype(np.float32))]
    SO.run_late(lambda b: tuple(kmeans1d.fit_channels(b[0], [2, 5, 3])), late(7), late(SO.STALE_SEED), blocking=True, spin=spin,
                name="fit_channels")


@gpu
def test_the_wrappers_compress_is_ordered_on_the_callers_stream(spin):
    """The images arrive late on a side stream as device tensors; the stub VAE hands them through as the latents."""
    _need_gpu()
    import vbq_amd

    class Through:
        def encode(self, X):
            return X, None

        def decode(self, Z):
            return Z
    levels, C = [2, 4], 3
    w = vbq_amd.ChannelwiseOptimalKmeansWrapper(C, levels)
    w.fit_latents(np.random.default_rng(1).standard_normal((128, C)).astype(np.float32), 1.0)

    def late(seed):
        return [_cuda(np.random.default_rng(seed).standard_normal((2, 8, 8, C)).astype(np.float32))]
    SO.run_late(lambda b: w.compress(b[0], Through(), levels, clip=False), late(7), late(SO.STALE_SEED), blocking=True, spin=spin,
                name="ChannelwiseOptimalKmeansWrapper.compress")
