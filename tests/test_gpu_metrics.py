"""The image-metric kernels (vbq_metrics.hip) against the high-precision reference oracle/metrics_f64.py, which does not
share their method: one MS-SSIM scale at a time (both outputs), the 2 x 2 decimation, the full ms_ssim at Kodak size,
mse / psnr, and the refusals.  Every bounded comparison prints its worst error next to its bound (run with -s);
oracle/metrics_f64.ssim_scale_error_bound derives the bound."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import metrics_f64 as R  # noqa: E402
from oracle import vbq_oracle as O  # noqa: E402

U = 2.0 ** -53
FS, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _scale_gpu(x, y, max_val=255, filter_size=FS):
    from vbq_amd import metrics
    s, c = metrics._ssim_for_multiscale(_dev(x), _dev(y), max_val, filter_size, SIGMA, K1, K2)
    return s.cpu().numpy(), c.cpu().numpy()


def _check_scale(name, x, y, max_val=255, filter_size=FS):
    """GPU ssim / cs of one scale against the long double reference within the derived bound; returns the worst
    err / bound of the two."""
    B, H, W, C = x.shape
    size = min(filter_size, H, W)
    s, c = _scale_gpu(x, y, max_val, filter_size)
    rs, rc = R.ssim_scale_ld(x, y, max_val=max_val, filter_size=filter_size)
    Ho, Wo = H - size + 1, W - size + 1
    M = max(float(np.abs(x).max()), float(np.abs(y).max()), 1e-300)
    bs, bc = R.ssim_scale_error_bound(size, M, max_val, K1, K2, n_per_image=Ho * Wo * C,
                                      n_partials=C * -(-Ho // 16) * -(-Wo // 16))
    assert bs < 1e-9 and bc < 1e-9
    es, ec = np.abs(s - rs), np.abs(c - rc)
    assert np.all(es <= bs), f"{name}: ssim err {es.max():.3g} > bound {bs:.3g}"
    assert np.all(ec <= bc), f"{name}: cs err {ec.max():.3g} > bound {bc:.3g}"
    return max(es.max() / bs, ec.max() / bc)


def _report(name, worst):
    print(f"\nBOUND {name}: worst err/bound {worst:.3g}")


def _noisy(rng, x, amp):
    return np.clip(x.astype(np.int64) + rng.integers(-amp, amp + 1, x.shape), 0, 255).astype(np.uint8)


# ---- one scale ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", range(1, 12))
def test_scale_valid_sizes_and_windows(size):
    """Ho, Wo in {1, 15, 16, 17, 33}: one tile, a tile short by one, a full tile, one past, two full plus one."""
    _need_gpu()
    rng = np.random.default_rng(size)
    worst = 0.0
    for Ho in (1, 15, 16, 17, 33):
        for Wo in (1, 15, 16, 17, 33):
            shape = (1, Ho + size - 1, Wo + size - 1, 3)
            x = rng.integers(0, 256, shape).astype(np.uint8)
            y = _noisy(rng, x, 40)
            worst = max(worst, _check_scale(f"size {size} {Ho}x{Wo}", x, y, filter_size=size))
    _report(f"scale size={size}", worst)


@pytest.mark.parametrize("B,C", [(1, 1), (5, 2), (1, 3), (5, 4), (70, 7), (70, 1), (1, 7)])
def test_scale_batch_and_channels(B, C):
    _need_gpu()
    rng = np.random.default_rng(B * 10 + C)
    x = rng.integers(0, 256, (B, 27, 42, C)).astype(np.uint8)
    y = _noisy(rng, x, 25)
    _report(f"scale B={B} C={C}", _check_scale(f"B={B} C={C}", x, y))


@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (9, 1), (4, 6), (7, 7), (10, 13), (8, 40)])
def test_scale_small_images_shrink_the_window(H, W):
    """Images smaller than the window: size = min(11, H, W), sigma scaled with it (:124-128)."""
    _need_gpu()
    rng = np.random.default_rng(H * 100 + W)
    x = rng.integers(0, 256, (3, H, W, 2)).astype(np.uint8)
    _report(f"scale small {H}x{W}", _check_scale(f"{H}x{W}", x, _noisy(rng, x, 30)))


def test_scale_image_kinds():
    """Constant images, a 0/255 checkerboard (s11 = E[x^2] - mu^2 with every pixel at the extremes), independent
    random pairs (cs near 0), all-0 against all-255, and identical pairs (exactly 1)."""
    _need_gpu()
    rng = np.random.default_rng(7)
    shape = (2, 40, 45, 3)
    yy, xx = np.mgrid[0:shape[1], 0:shape[2]]
    checker = np.broadcast_to((((yy + xx) % 2) * 255).astype(np.uint8)[None, :, :, None], shape).copy()
    const = np.full(shape, 255, np.uint8)
    rand = rng.integers(0, 256, shape).astype(np.uint8)
    cases = {
        "const vs noisy": (const, _noisy(rng, const, 3)),
        "const 255 vs const 254": (const, const - 1),
        "checker vs noisy checker": (checker, _noisy(rng, checker, 2)),
        "checker vs shifted checker": (checker, 255 - checker),
        "checker vs random": (checker, rand),
        "random vs random": (rand, rng.integers(0, 256, shape).astype(np.uint8)),
        "zeros vs 255": (np.zeros(shape, np.uint8), const),
    }
    worst = 0.0
    for size in (11, 6, 3):
        for name, (x, y) in cases.items():
            worst = max(worst, _check_scale(f"{name} fs={size}", x, y, filter_size=size))
        for x in (rand, checker, const, np.zeros(shape, np.uint8)):
            s, c = _scale_gpu(x, x, filter_size=size)
            assert np.array_equal(s, np.ones(2)) and np.array_equal(c, np.ones(2)), "identical pair must give exactly 1"
    _report("scale image kinds", worst)


def test_scale_float_images_max_val_1():
    _need_gpu()
    rng = np.random.default_rng(9)
    x = rng.random((3, 30, 35, 3))
    y = np.clip(x + rng.normal(0, 0.05, x.shape), 0, 1)
    worst = max(_check_scale("unit f64", x, y, max_val=1),
                _check_scale("unit f32", x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64),
                             max_val=1, filter_size=7))
    _report("scale float max_val=1", worst)


# ---- decimation -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 1), (2, 3), (3, 3), (7, 10), (33, 47), (64, 2), (5, 1)])
def test_downsample_bit_exact_on_u8_pyramids(H, W):
    """u8-derived values are dyadic rationals of < 20 bits, so ndimage.convolve's sum and the kernel's are both
    exact: bit for bit at every level of the pyramid, down to 1 x 1."""
    _need_gpu()
    from vbq_amd import metrics
    rng = np.random.default_rng(H * 1000 + W)
    im = rng.integers(0, 256, (3, H, W, 2)).astype(np.float64)
    d = _dev(im)
    for _ in range(7):
        want = R.downsample2_ndimage(im)
        d = metrics._downsample(d)
        got = d.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want)
        im = want


def test_downsample_arbitrary_f64():
    """Arbitrary non-negative f64 pixels: bit for bit the kernel's documented order 0.25 * ((a + b) + (c + d))
    (vbq_oracle.downsample2), and within the rounding of a two-level sum, 2u (a + b + c + d) / 4, of the exact mean
    next to ndimage.convolve's sequential sum.  (1 ulp is not a bound for either order: two different 4-term orders
    differ by 2 ulp on about one block in 10^3.)"""
    _need_gpu()
    from vbq_amd import metrics
    rng = np.random.default_rng(13)
    for shape in [(2, 33, 47, 3), (1, 64, 2, 2), (3, 5, 1, 1)]:
        for im in (rng.random(shape), np.exp(rng.normal(0, 3, shape))):
            got = metrics._downsample(_dev(im)).cpu().numpy()
            assert np.array_equal(got, O.downsample2(im))
            exact = O.downsample2(im.astype(np.longdouble))          # 64-bit significands: exact to ~2^-64
            mag = O.downsample2(np.abs(im))
            assert np.all(np.abs(got - exact) <= 2 * U * mag * (1 + 1e-3))
            assert np.all(np.abs(R.downsample2_ndimage(im) - exact) <= 3 * U * mag * (1 + 1e-3))


# ---- full ms_ssim ---------------------------------------------------------------------------------------------------

def _product_bound(mssim, mcs, weights, bounds):
    """Relative bound on prod(cs_i^w_i) * ssim_L^w_L from the per-scale absolute bounds (first order), plus the
    host's power / product roundings."""
    w = np.asarray(weights)
    L = len(w)
    rel = sum(w[i] * bounds[i][1] / np.abs(mcs[i]) for i in range(L - 1)) + w[L - 1] * bounds[L - 1][0] / np.abs(mssim[L - 1])
    return rel * 1.01 + 4 * L * U


def _gpu_pyramid(x, y, weights, max_val=255):
    """Every scale's (ssim, cs) of the GPU's own pyramid, as ms_ssim computes them."""
    from vbq_amd import metrics
    a, b = _dev(x), _dev(y)
    out = []
    for i in range(len(weights)):
        s, c = metrics._ssim_for_multiscale(a, b, max_val, FS, SIGMA, K1, K2)
        out.append((s.cpu().numpy(), c.cpu().numpy()))
        if i + 1 < len(weights):
            a, b = metrics._downsample(a), metrics._downsample(b)
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def _check_ms_ssim(name, x, y, weights, max_val=255, got=None):
    from vbq_amd import metrics
    w = list(weights) if weights else list(R.DEFAULT_WEIGHTS)
    value, rs, rc = R.ms_ssim_f64(x, y, max_val=max_val, weights=w)
    gs, gc = _gpu_pyramid(x, y, w, max_val)
    bounds, worst, im = [], 0.0, np.asarray(x, np.float64)
    for i in range(len(w)):
        H, W, C = im.shape[1:]
        size = min(FS, H, W)
        Ho, Wo = H - size + 1, W - size + 1
        M = max(float(np.abs(x).max()), float(np.abs(y).max()))
        bs, bc = R.ssim_scale_error_bound(size, M, max_val, n_per_image=Ho * Wo * C,
                                          n_partials=C * -(-Ho // 16) * -(-Wo // 16))
        assert np.all(np.abs(gs[i] - rs[i]) <= bs), f"{name} scale {i} ssim"
        assert np.all(np.abs(gc[i] - rc[i]) <= bc), f"{name} scale {i} cs"
        worst = max(worst, np.abs(gs[i] - rs[i]).max() / bs, np.abs(gc[i] - rc[i]).max() / bc)
        bounds.append((bs, bc))
        im = im[:, ::2, ::2]
    got = metrics.ms_ssim(x, y, max_val=max_val, weights=weights) if got is None else got
    rel = _product_bound(rs, rc, w, bounds)
    err = np.abs(got - value) / np.abs(value)
    assert np.all(err <= rel), f"{name}: ms_ssim rel err {err.max():.3g} > {rel.max():.3g}"
    return max(worst, float((err / rel).max()))


def test_ms_ssim_kodak_all_scales():
    """512 x 768 x 3, B = 2: every scale's ssim and cs, not only the product (scale 0's cs enters it with weight
    0.0448 only; the ssim of scales 0-3 not at all)."""
    _need_gpu()
    rng = np.random.default_rng(24)
    yy, xx = np.mgrid[0:512, 0:768]
    base = 128 + 100 * np.sin(yy / 23.0)[None, :, :, None] * np.cos(xx[..., None] / 17.0 + np.arange(3))[None]
    x = np.clip(base + rng.normal(0, 8, (2, 512, 768, 3)), 0, 255).astype(np.uint8)
    y = np.clip(x + rng.normal(0, 1, x.shape) * np.array([4.0, 20.0])[:, None, None, None], 0, 255).astype(np.uint8)
    _report("ms_ssim kodak", _check_ms_ssim("kodak", x, y, None))


@pytest.mark.parametrize("levels", range(1, 7))
def test_ms_ssim_weights_lengths(levels):
    """H = 20 goes 20, 10, 5, 3, 2, 1 over six scales."""
    _need_gpu()
    rng = np.random.default_rng(levels)
    w = list(rng.uniform(0.05, 0.4, levels))
    x = rng.integers(0, 256, (3, 20, 37, 3)).astype(np.uint8)
    _report(f"ms_ssim levels={levels}", _check_ms_ssim(f"levels={levels}", x, _noisy(rng, x, 12), w))


def test_ms_ssim_input_types_max_val_1():
    """Float images in [0, 1] with max_val=1: NumPy f32 / f64, device f32 / f64; u8 device tensors with max_val=255."""
    _need_gpu()
    from vbq_amd import metrics
    rng = np.random.default_rng(31)
    x = rng.random((2, 48, 56, 3))
    y = np.clip(x + rng.normal(0, 0.03, x.shape), 0, 1)
    worst = 0.0
    for dt in (np.float64, np.float32):
        xa, ya = x.astype(dt), y.astype(dt)
        want = metrics.ms_ssim(xa, ya, max_val=1)
        worst = max(worst, _check_ms_ssim(f"numpy {dt.__name__}", xa.astype(np.float64), ya.astype(np.float64), None,
                                          max_val=1, got=want))
        tdt = torch.float64 if dt is np.float64 else torch.float32
        got = metrics.ms_ssim(torch.from_numpy(xa).cuda(), torch.from_numpy(ya).to("cuda", tdt), max_val=1)
        assert np.array_equal(got, want)
    xu = (x * 255).astype(np.uint8)
    yu = (y * 255).astype(np.uint8)
    want = metrics.ms_ssim(xu, yu)
    assert np.array_equal(metrics.ms_ssim(torch.from_numpy(xu).cuda(), torch.from_numpy(yu).cuda()), want)
    worst = max(worst, _check_ms_ssim("u8", xu, yu, None, got=want))
    _report("ms_ssim input types", worst)


def test_ms_ssim_luma_chroma_slices():
    """Non-contiguous x[..., :1] and x[..., 1:], as evaluate_compression_* passes them, NumPy and device."""
    _need_gpu()
    from vbq_amd import metrics
    rng = np.random.default_rng(41)
    x = rng.integers(0, 256, (2, 64, 72, 3)).astype(np.uint8)
    y = _noisy(rng, x, 15)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    worst = 0.0
    for sl in (np.s_[..., :1], np.s_[..., 1:]):
        assert not x[sl].flags.c_contiguous and not xt[sl].is_contiguous()
        got = metrics.ms_ssim(x[sl], y[sl])
        assert np.array_equal(metrics.ms_ssim(xt[sl], yt[sl]), got)
        worst = max(worst, _check_ms_ssim(f"slice {sl}", np.ascontiguousarray(x[sl]), np.ascontiguousarray(y[sl]), None,
                                          got=got))
        mse = metrics.mse(x[sl], y[sl])
        assert np.array_equal(metrics.mse(xt[sl], yt[sl]), mse)
        d = x[sl].astype(np.int64) - y[sl]
        assert np.array_equal(mse, np.sum(d * d, axis=(1, 2, 3)) / d[0].size)
    _report("ms_ssim slices", worst)


# ---- mse / psnr -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 1), (300, 9, 7, 3), (2, 2048, 2048, 3), (3, 1023, 1025, 1)])
def test_mse_psnr_u8_exact(B, H, W, C):
    """The integer sum of squares, exactly, divided by n -- including 12 Mi bytes per image, past the 1024-workgroup
    cap of k_sqerr_u8 (grid-stride loop), and 300 images."""
    _need_gpu()
    from vbq_amd import metrics
    rng = np.random.default_rng(B + H)
    x = rng.integers(0, 256, (B, H, W, C)).astype(np.uint8)
    y = rng.integers(0, 256, (B, H, W, C)).astype(np.uint8)
    if B > 1:
        y[1] = x[1]                                          # mse 0: psnr inf
    d = x.astype(np.int64) - y
    want = np.sum(d * d, axis=(1, 2, 3)) / (H * W * C)
    got = metrics.mse(x, y)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    with np.errstate(divide="ignore"):
        assert np.array_equal(metrics.psnr(x, y), 20 * np.log10(255) - 10 * np.log10(want))
    assert np.array_equal(metrics.mse(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()), want)


def test_mse_float_against_long_double():
    _need_gpu()
    from vbq_amd import metrics
    rng = np.random.default_rng(3)
    for shape in [(4, 100, 130, 3), (1, 1, 1, 1), (2, 512, 768, 1)]:
        x = rng.random(shape)
        y = np.clip(x + rng.normal(0, 1e-3, shape), 0, 1)
        want = R.mse_ld(x, y)
        for a, b in ((x, y), (x.astype(np.float32), y.astype(np.float32)), (torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())):
            got = metrics.mse(a, b)
            ref = want if not (isinstance(a, np.ndarray) and a.dtype == np.float32) else \
                R.mse_ld(x.astype(np.float32), y.astype(np.float32))
            # one rounded difference and square per pixel (3u relative), a reduction over n terms (log2 n u)
            assert np.all(np.abs(got - ref) <= (3 + np.log2(x[0].size) + 2) * U * ref)


# ---- refusals -------------------------------------------------------------------------------------------------------

def test_refusals():
    _need_gpu()
    from vbq_amd import metrics
    from vbq_amd._lib import VBQError
    x = np.zeros((1, 16, 16, 1), np.uint8)
    with pytest.raises(VBQError):
        metrics.ms_ssim(x, x, filter_size=12)
    with pytest.raises(VBQError):
        metrics.ms_ssim(x, x, filter_size=0)
    with pytest.raises(VBQError):
        metrics._ssim_for_multiscale(_dev(x), _dev(x), 255, 12, SIGMA, K1, K2)
    with pytest.raises(RuntimeError, match="same shape"):
        metrics.ms_ssim(x, np.zeros((1, 16, 15, 1), np.uint8))
    with pytest.raises(RuntimeError, match="same shape"):
        metrics.mse(x, np.zeros((1, 16, 15, 1), np.uint8))
    with pytest.raises(RuntimeError, match="four dimensions"):
        metrics.ms_ssim(x[0], x[0])
    with pytest.raises(RuntimeError, match="four dimensions"):
        metrics.mse(x[..., None], x[..., None])
