"""f3: the comparison quantizers against golden vectors produced by the reference's own classes
(tests/golden/make_golden.py g9)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def test_uniform_and_kmeans_quantizers_golden(golden):
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    from vbq_amd.baselines import ChannelwiseSimpleQuantizer, KmeansQuantizer, UniformQuantizer
    g = golden("g9_baselines.npz")
    x = g["x"]
    for K in (4, 16, 61):
        u = UniformQuantizer(K)
        u.fit(x, add_n_smoothing=1)
        assert u.min == g[f"u{K}_min"] and u.delta == g[f"u{K}_delta"]
        assert np.array_equal(u.code_points, g[f"u{K}_code_points"])
        assert np.array_equal(u.code_lengths, g[f"u{K}_code_lengths"])
        q, I, nb = u.quantize(x)
        assert q.dtype == np.float32 and np.array_equal(q, g[f"u{K}_q"])
        assert np.array_equal(I, g[f"u{K}_I"]) and np.array_equal(nb, g[f"u{K}_bits"])
    k = KmeansQuantizer(12)
    k.code_points = g["k_centers"]
    k.code_lengths = -np.log2(np.full(12, 1 / 12.0))
    q, I, nb = k.quantize(x)
    assert np.array_equal(q, g["k_q"]) and np.array_equal(I, g["k_I"])
    # channel-wise wrapper plumbing
    cq = ChannelwiseSimpleQuantizer(UniformQuantizer, 3, 8)
    lat = np.stack([x[:900], 2 * x[900:1800], x[1800:2700] - 1], axis=1).reshape(1, 30, 30, 3)
    cq.fit_latents(lat, 1)
    out = cq.compress_latents(lat)
    assert out["Z_hat"].shape == lat.shape and out["num_bits"].shape == lat.shape
    u0 = UniformQuantizer(8)
    u0.fit(lat.reshape(-1, 3)[:, 1], 1)
    assert np.array_equal(out["Z_hat"].reshape(-1, 3)[:, 1], u0.quantize(lat.reshape(-1, 3)[:, 1])[0])


# ---- edges of the two kernels, against the reference's own arithmetic -----------------------------------------------

def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _edges(mn, delta, levels):
    """Every bin edge mn + k delta (k = 0..levels) in float32 arithmetic, and its nextafter on both sides."""
    e = (np.float32(mn) + np.arange(levels + 1, dtype=np.float32) * np.float32(delta)).astype(np.float32)
    return np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))])


def _uniform_check(u, fit, x):
    from oracle import vbq_oracle as O
    q, I, nb = u.quantize(x)
    with np.errstate(over="ignore", invalid="ignore"):
        wq, wI, wnb = O.uniform_quantize(x, fit)
    assert q.dtype == np.float32 and I.dtype == np.float32
    assert np.array_equal(I, wI) and np.array_equal(q, wq) and np.array_equal(nb, wnb)


@pytest.mark.parametrize("levels", [1, 2, 3, 255, 256, 4096, 65536])
@pytest.mark.parametrize("span", ["unit", "tiny", "huge"])
def test_uniform_quantizer_bin_edges(levels, span):
    """Bit for bit the reference's float32 NumPy arithmetic (vbq_oracle.uniform_fit / uniform_quantize) on every bin edge
    and one ulp either side, below min, above max, +-inf and -0.0; the fused bincount of fit through the code lengths."""
    _need_gpu()
    from oracle import vbq_oracle as O
    from vbq_amd.baselines import UniformQuantizer
    rng = np.random.default_rng(levels)
    lo, hi = {"unit": (-0.75, 1.25), "tiny": (1.0, float(np.float32(1.0) + 5 * np.spacing(np.float32(1.0)))),
              "huge": (-1e38, 1e38)}[span]
    fit_x = np.concatenate([rng.uniform(lo, hi, 20000), [lo, hi]]).astype(np.float32)
    if span == "tiny":
        fit_x = (np.float32(1.0) + rng.integers(0, 6, 20000) * np.spacing(np.float32(1.0))).astype(np.float32)
        fit_x[:2] = [lo, hi]
    u = UniformQuantizer(levels)
    u.fit(fit_x, add_n_smoothing=1)
    with np.errstate(over="ignore"):
        fit = O.uniform_fit(fit_x, levels)
    assert u.min == fit["min"] and u.delta == fit["delta"] and u.delta.dtype == np.float32
    assert np.array_equal(u.code_points, fit["code_points"]) and np.array_equal(u.code_lengths, fit["code_lengths"])
    x = np.concatenate([_edges(u.min, u.delta, levels), fit_x[:5000],
                        [np.float32(-np.inf), np.float32(np.inf), np.float32(-0.0), np.float32(0.0),
                         np.nextafter(u.min, np.float32(-np.inf)), np.float32(-3e38), np.float32(3e38)]]).astype(np.float32)
    _uniform_check(u, fit, x)
    # the fused counts of the kernel against np.bincount of the reference's bins, directly
    _, _, counts = u._run(x, True)
    with np.errstate(over="ignore", invalid="ignore"):
        wI = O.uniform_quantize(x, fit)[1]
    assert np.array_equal(counts.cpu().numpy(), np.bincount(wI.astype(np.int32), minlength=levels))


@pytest.mark.parametrize("n", [1, 257, 2 ** 20 + 3, 5_000_000])
def test_uniform_quantizer_sizes(n):
    """5e6 samples run the grid-stride loop (4096 x 256 threads)."""
    _need_gpu()
    from oracle import vbq_oracle as O
    from vbq_amd.baselines import UniformQuantizer
    rng = np.random.default_rng(n)
    x = rng.standard_normal(max(n, 2)).astype(np.float32)[:max(n, 2)]
    for levels in (7, 256):
        u = UniformQuantizer(levels)
        u.fit(x, add_n_smoothing=1)
        fit = O.uniform_fit(x, levels)
        assert np.array_equal(u.code_lengths, fit["code_lengths"])
        _uniform_check(u, fit, x[:n])
        t = torch.from_numpy(x[:n]).cuda()                       # device tensor in
        q, I, nb = u.quantize(t)
        assert np.array_equal(I, O.uniform_quantize(x[:n], fit)[1])


def _vq_ref(x, codes):
    from scipy.cluster import vq
    I, _ = vq.vq(np.asarray(x), np.asarray(codes))
    return I


def _nearest_raw(x, codes):
    """vbq_nearest_code_f64 through ctypes: index, value and the fused counts."""
    import ctypes as C
    from vbq_amd import _lib, ops
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    cd = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.float64)).cuda()
    I = torch.empty(xd.numel(), dtype=torch.int32, device=xd.device)
    q = torch.empty(xd.numel(), dtype=torch.float64, device=xd.device)
    counts = torch.zeros(cd.numel(), dtype=torch.int64, device=xd.device)
    _lib.check(_lib.lib().vbq_nearest_code_f64(ops._ptr(xd), xd.numel(), ops._ptr(cd), cd.numel(), ops._ptr(I), ops._ptr(q),
                                               ops._ptr(counts), ops._stream(xd)), "vbq_nearest_code_f64")
    return I.cpu().numpy(), q.cpu().numpy(), counts.cpu().numpy()


def test_nearest_code_ties_and_duplicates():
    """Samples exactly halfway between two code points return the first minimum in code-book order -- also when the
    book is unsorted and the tied partner comes first -- and duplicated code points return the first copy."""
    _need_gpu()
    from vbq_amd.baselines import KmeansQuantizer
    rng = np.random.default_rng(1)
    sorted_book = np.arange(12, dtype=np.float64) / 8.0 - 0.5
    mids = ((np.arange(11) + 0.5) / 8.0 - 0.5).astype(np.float32)        # exact midpoints: equal f64 squared distances
    for book in (sorted_book, sorted_book[::-1].copy(), rng.permutation(sorted_book),
                 np.array([1.0, 0.0, 1.0, 0.5, 0.0, 0.5]), np.array([0.25, 0.25, 0.25])):
        x = np.concatenate([mids, np.repeat(mids, 3), book.astype(np.float32), rng.uniform(-1, 1.5, 3000).astype(np.float32)])
        want = _vq_ref(x, book)
        I, q, counts = _nearest_raw(x, book)
        assert np.array_equal(I, want) and np.array_equal(q, book[want])
        assert np.array_equal(counts, np.bincount(want, minlength=len(book)))
        k = KmeansQuantizer(len(book))
        k.code_points = book
        k.code_lengths = np.arange(len(book), dtype=np.float64)
        qq, II, nb = k.quantize(x)
        assert np.array_equal(II, want) and np.array_equal(qq, book[want]) and np.array_equal(nb, k.code_lengths[want])
    # the tie is real: a later book entry at the same distance, never picked
    I, _, _ = _nearest_raw(np.array([1.5], np.float32), np.array([2.0, 1.0]))
    assert I[0] == 0


@pytest.mark.parametrize("K", [1, 2, 12, 255, 256, 257, 4096, 8192])
def test_nearest_code_book_sizes(K):
    """Up to K = 8192, the largest book the entry point takes (64 KB of dynamic LDS)."""
    _need_gpu()
    rng = np.random.default_rng(K)
    book = rng.normal(0, 1, K)
    if K >= 4:
        book[K // 2] = book[1]                                           # a duplicate
    n = 100_000 if K >= 4096 else 300_000
    x = np.concatenate([rng.normal(0, 1.2, n), book[:50], [1e30, -1e30, 0.0]]).astype(np.float32)
    want = _vq_ref(x, book)
    I, q, counts = _nearest_raw(x, book)
    assert np.array_equal(I, want) and np.array_equal(q, book[want])
    assert np.array_equal(counts, np.bincount(want, minlength=K))


def test_nearest_code_grid_stride_and_refusal():
    _need_gpu()
    from vbq_amd._lib import VBQError
    rng = np.random.default_rng(2)
    book = np.array([0.5, -1.0, 2.0, 0.0, -0.25, 1.0, 3.0, -2.0])
    x = rng.normal(0, 1.5, 3_000_000).astype(np.float32)                 # > 4096 x 256: the grid-stride loop
    x[::1000] = 0.75                                                     # ties between 0.5 and 1.0
    want = _vq_ref(x, book)
    I, q, counts = _nearest_raw(x, book)
    assert np.array_equal(I, want) and np.array_equal(counts, np.bincount(want, minlength=len(book)))
    with pytest.raises(VBQError, match="8192"):
        _nearest_raw(x[:10], np.zeros(8193))


# ---- non-finite samples are refused, as the reference refuses them --------------------------------------------------

def _channelwise(qtype, levels, lat):
    from vbq_amd.baselines import ChannelwiseSimpleQuantizer, ChannelwiseSimpleQuantizerWrapper
    cq = ChannelwiseSimpleQuantizer(qtype, lat.shape[-1], levels)
    w = ChannelwiseSimpleQuantizerWrapper(qtype, lat.shape[-1], [levels])
    return cq, w


def test_kmeans_quantizer_refuses_nan_and_inf():
    """scipy.cluster.vq.vq raises ValueError on NaN or +-inf; k_nearest_code would return index 0."""
    _need_gpu()
    from vbq_amd.baselines import ChannelwiseSimpleQuantizer, KmeansQuantizer
    book = np.array([0.5, -1.0, 2.0])
    k = KmeansQuantizer(3)
    k.code_points, k.code_lengths = book, np.ones(3)
    x = np.linspace(-2, 3, 50).astype(np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[17] = bad
        with pytest.raises(ValueError):
            _vq_ref(y, book)                                             # the reference
        with pytest.raises(ValueError):
            k.quantize(y)
        with pytest.raises(ValueError):
            k.quantize(torch.from_numpy(y).cuda())
        with pytest.raises(ValueError):
            k.quantize(torch.from_numpy(y))
        cq = ChannelwiseSimpleQuantizer(KmeansQuantizer, 2, 3)
        for q in cq._quantizers:
            q.code_points, q.code_lengths = book, np.ones(3)
        with pytest.raises(ValueError):
            cq.compress_latents(np.stack([x, y], axis=1).reshape(1, 5, 10, 2))
    assert np.array_equal(k.quantize(x)[1], _vq_ref(x, book))


def test_uniform_quantizer_refuses_nan_keeps_inf():
    """floor(NaN) cast to int32 is INT_MIN, which np.bincount (fit) and np.take (quantize) refuse; k_uniform_quantize
    would put NaN in bin 0 (fmaxf(NaN, 0) = 0) and fit would count it there.  +-inf clip to an edge bin, as in NumPy."""
    _need_gpu()
    from oracle import vbq_oracle as O
    from vbq_amd.baselines import ChannelwiseSimpleQuantizer, ChannelwiseSimpleQuantizerWrapper, UniformQuantizer
    rng = np.random.default_rng(4)
    x = rng.standard_normal(1000).astype(np.float32)
    y = x.copy()
    y[3] = np.nan
    with pytest.raises(ValueError), np.errstate(invalid="ignore"):
        O.uniform_fit(y, 8)                                              # the reference
    u = UniformQuantizer(8)
    for bad in (y, torch.from_numpy(y), torch.from_numpy(y).cuda()):
        with pytest.raises(ValueError):
            u.fit(bad)
    u.fit(x)
    fit = O.uniform_fit(x, 8)
    for bad in (y, torch.from_numpy(y).cuda()):
        with pytest.raises(ValueError):
            u.quantize(bad)
    lat = np.stack([x, y], axis=1).reshape(1, 20, 50, 2)
    with pytest.raises(ValueError):
        ChannelwiseSimpleQuantizer(UniformQuantizer, 2, 8).fit_latents(lat, 1)
    cq = ChannelwiseSimpleQuantizer(UniformQuantizer, 2, 8)
    good = np.stack([x, x], axis=1).reshape(1, 20, 50, 2)
    cq.fit_latents(good, 1)
    with pytest.raises(ValueError):
        cq.compress_latents(lat)

    class _Identity:
        def encode(self, X):
            return X, None

        def decode(self, Z):
            return Z
    w = ChannelwiseSimpleQuantizerWrapper(UniformQuantizer, 2, [8])
    with pytest.raises(ValueError):
        w.fit(lat, _Identity(), 1)
    w.fit(good, _Identity(), 1)
    with pytest.raises(ValueError):
        w.compress(lat, _Identity(), [8])
    # +-inf stay fine and clip to the edge bins
    z = np.concatenate([x, np.array([np.inf, -np.inf], np.float32)])
    _uniform_check(u, fit, z)
    _, I, _ = u.quantize(z)
    assert I[-2] == 7 and I[-1] == 0
