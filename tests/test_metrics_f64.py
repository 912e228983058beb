"""The high-precision metric reference (oracle/metrics_f64.py) pinned on the CPU before any GPU test leans on it:
against the separable NumPy restatement (vbq_oracle), against the reference's own fftconvolve arithmetic, against the
reference module's outputs (g11), and its decimation against vbq_oracle.downsample2 bit for bit."""
import numpy as np
import pytest

from oracle import metrics_f64 as R
from oracle import vbq_oracle as O


def _pair(rng, shape, noise=20):
    x = rng.integers(0, 256, shape).astype(np.uint8)
    y = np.clip(x.astype(np.int64) + rng.integers(-noise, noise + 1, shape), 0, 255).astype(np.uint8)
    return x, y


def _bound(im, size):
    B, H, W, C = im.shape
    return R.ssim_scale_error_bound(size, 255.0, n_per_image=(H - size + 1) * (W - size + 1) * C)


def test_window_is_one_normalised_2d_gaussian():
    for size in range(1, 12):
        sigma = size * 1.5 / 11
        g = R.window2d(size, sigma)
        assert g.shape == (size, size) and g.dtype == np.longdouble
        assert abs(g.sum() - 1) < 1e-17 and np.array_equal(g, g.T) and np.array_equal(g, g[::-1, ::-1])
        sep = O._gauss_window_1d(size, sigma)
        assert np.abs(np.outer(sep, sep) - g.astype(np.float64)).max() < 1e-15
    # even sizes sit on the half-integer grid: four equal centre taps
    g = R.window2d(4, 1.0)
    assert g[1, 1] == g[1, 2] == g[2, 1] == g[2, 2] and g[1, 1] > g[0, 1] > g[0, 0]


@pytest.mark.parametrize("shape", [(2, 23, 31, 3), (1, 24, 30, 2), (3, 1, 17, 1), (2, 19, 1, 2), (1, 12, 12, 4)])
def test_scale_against_separable_and_fft(shape):
    rng = np.random.default_rng(sum(shape))
    x, y = _pair(rng, shape)
    worst = 0.0
    for fs in range(1, 12):
        size = min(fs, shape[1], shape[2])
        bs, bc = _bound(x, size)
        assert bs < 1e-9 and bc < 1e-9
        s, c = R.ssim_scale_ld(x, y, filter_size=fs)
        so, co = O.ssim_scale(x.astype(np.float64), y.astype(np.float64), filter_size=fs)
        sf, cf = R.ssim_scale_fft(x, y, filter_size=fs)
        for got_s, got_c in ((so, co), (sf, cf)):
            assert np.all(np.abs(got_s - s) <= bs) and np.all(np.abs(got_c - c) <= bc)
            worst = max(worst, np.abs(got_s - s).max() / bs, np.abs(got_c - c).max() / bc)
    print(f"\nBOUND cpu scale {shape}: worst err/bound {worst:.3g}")


def test_identical_and_extreme_pairs():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (2, 20, 21, 3)).astype(np.uint8)
    s, c = R.ssim_scale_ld(x, x)
    assert np.array_equal(s, np.ones(2)) and np.array_equal(c, np.ones(2))
    zero, full = np.zeros((1, 16, 16, 1), np.uint8), np.full((1, 16, 16, 1), 255, np.uint8)
    s, c = R.ssim_scale_ld(zero, full)
    c1 = (0.01 * 255) ** 2
    assert abs(c[0] - 1) < 1e-15 and abs(s[0] - c1 / (255.0 ** 2 + c1)) < 1e-15


@pytest.mark.parametrize("shape", [(2, 37, 50, 3), (1, 64, 64, 1), (2, 1, 9, 2), (1, 9, 1, 1), (1, 2, 3, 1)])
def test_downsample_matches_oracle_bit_for_bit(shape):
    """u8-derived pyramids hold dyadic rationals of < 20 bits: every order of the four-term sum is exact."""
    rng = np.random.default_rng(shape[1] * 100 + shape[2])
    im = rng.integers(0, 256, shape).astype(np.float64)
    for _ in range(6):
        a, b = R.downsample2_ndimage(im), O.downsample2(im)
        assert a.shape == b.shape == (shape[0], (im.shape[1] + 1) // 2, (im.shape[2] + 1) // 2, shape[3])
        assert np.array_equal(a, b)
        im = a


@pytest.mark.parametrize("weights", [None, [1.0], [0.3, 0.7], [0.1, 0.2, 0.3, 0.2, 0.1, 0.1]])
def test_ms_ssim_against_oracle_and_fft(weights):
    rng = np.random.default_rng(11)
    x, y = _pair(rng, (2, 44, 52, 3), noise=40)
    v, ms, mc = R.ms_ssim_f64(x, y, weights=weights)
    vf, msf, mcf = R.ms_ssim_f64(x, y, weights=weights, scale_fn=R.ssim_scale_fft)
    levels = len(weights) if weights else 5
    assert ms.shape == mc.shape == (levels, 2)
    im = x.astype(np.float64)
    for i in range(levels):
        bs, bc = _bound(im, min(11, im.shape[1], im.shape[2]))
        assert np.all(np.abs(msf[i] - ms[i]) <= bs) and np.all(np.abs(mcf[i] - mc[i]) <= bc)
        im = O.downsample2(im)
    if weights is None:
        assert np.allclose(O.ms_ssim(x, y), v, rtol=1e-12, atol=0)
    assert np.allclose(vf, v, rtol=1e-9, atol=0)


def test_reproduces_g11(golden):
    g = golden("g11_image_metrics.npz")
    for name in "abc":
        x, y = g[f"{name}_x"], g[f"{name}_y"]
        v, _, _ = R.ms_ssim_f64(x, y)
        assert np.allclose(v, g[f"{name}_msssim"], rtol=1e-9, atol=0)
        assert np.array_equal(R.mse_ld(x, y), g[f"{name}_mse"])
