"""High-precision reference for the image metrics (img-compression/img_comparison_metrics.py), test-only.

It deliberately does NOT share the method of the kernels (vbq_metrics.hip) or of the NumPy restatement
(vbq_oracle.ssim_scale), which both filter separably with an outer product of normalised 1-D factors:

    window2d(size, sigma)        one 2-D Gaussian normalised by its own sum (:70-81), even sizes on the
                                 half-integer grid, in long double
    ssim_scale_ld(...)           one scale of _SSIMForMultiScale (:84-157): the five filtered planes as a
                                 NON-separable 2-D 'valid' correlation accumulated in long double, the ssim
                                 and cs maps and their per-image means in long double; float64 out
    ssim_scale_fft(...)          the same scale with scipy.signal.fftconvolve(mode='valid'): the reference's
                                 own float64 arithmetic (not bit-reproducible; agrees to ~1e-12)
    downsample2_ndimage(im)      scipy.ndimage.convolve(im, ones((1, 2, 2, 1)) / 4, mode='reflect')[:, ::2, ::2, :]
    ms_ssim_f64(...)             :160-220 on top of either scale function; returns the product and the
                                 per-scale ssim / cs
    mse_ld(a, b)                 :6-16 as a long double mean

NumPy in, NumPy (float64) out.
"""
from __future__ import annotations

import numpy as np
from scipy import ndimage, signal

LD = np.longdouble
DEFAULT_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window2d(size, sigma, dtype=LD):
    """_FSpecialGauss: exp(-(x^2 + y^2) / (2 sigma^2)) on the (size x size) grid centred on 0 (offset 0.5 for even
    sizes), divided by its own sum."""
    radius = size // 2
    offset = 0.5 if size % 2 == 0 else 0.0
    t = np.arange(size, dtype=dtype) - dtype(radius) + dtype(offset)
    x, y = t[:, None], t[None, :]
    g = np.exp(-((x * x + y * y) / (dtype(2) * dtype(sigma) * dtype(sigma))))
    return g / g.sum()


def _correlate_valid_ld(x, g):
    """'valid' 2-D correlation of [B, H, W, C] with the (s x s) window g, every tap accumulated in long double (the
    window is symmetric, so correlation and convolution agree)."""
    s = g.shape[0]
    B, H, W, C = x.shape
    Ho, Wo = H - s + 1, W - s + 1
    acc = np.zeros((B, Ho, Wo, C), dtype=LD)
    tmp = np.empty_like(acc)
    for i in range(s):
        for j in range(s):
            np.multiply(x[:, i:i + Ho, j:j + Wo, :], g[i, j], out=tmp)
            acc += tmp
    return acc


def _size_sigma(H, W, filter_size, filter_sigma):
    size = min(filter_size, H, W)
    return size, size * filter_sigma / filter_size


def _maps(mu1, mu2, s11, s22, s12, c1, c2):
    """:141-156 in the precision of the inputs; returns the per-image means of the ssim and cs maps."""
    mu11, mu22, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11 = s11 - mu11
    s22 = s22 - mu22
    s12 = s12 - mu12
    v1 = 2 * s12 + c2
    v2 = s11 + s22 + c2
    ssim = ((2 * mu12 + c1) * v1) / ((mu11 + mu22 + c1) * v2)
    cs = v1 / v2
    return ssim.mean(axis=(1, 2, 3)), cs.mean(axis=(1, 2, 3))


def ssim_scale_ld(im1, im2, max_val=255, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
    """One scale, non-separable long double direct sums.  Returns (ssim [B], cs [B]) float64."""
    x, y = np.asarray(im1).astype(LD), np.asarray(im2).astype(LD)
    _, H, W, _ = x.shape
    size, sigma = _size_sigma(H, W, filter_size, filter_sigma)
    g = window2d(size, sigma)
    planes = [_correlate_valid_ld(p, g) for p in (x, y, x * x, y * y, x * y)]
    c1, c2 = (LD(k1) * LD(max_val)) ** 2, (LD(k2) * LD(max_val)) ** 2
    ssim, cs = _maps(*planes, c1, c2)
    return ssim.astype(np.float64), cs.astype(np.float64)


def ssim_scale_fft(im1, im2, max_val=255, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
    """One scale with the reference's float64 fftconvolve."""
    x, y = np.asarray(im1, np.float64), np.asarray(im2, np.float64)
    _, H, W, _ = x.shape
    size, sigma = _size_sigma(H, W, filter_size, filter_sigma)
    g = window2d(size, sigma, np.float64).reshape(1, size, size, 1)
    planes = [signal.fftconvolve(p, g, mode="valid") for p in (x, y, x * x, y * y, x * y)]
    return _maps(*planes, (k1 * max_val) ** 2, (k2 * max_val) ** 2)


def downsample2_ndimage(im):
    """The reference's decimation between scales (:214-216)."""
    filtered = ndimage.convolve(np.asarray(im, np.float64), np.ones((1, 2, 2, 1)) / 4.0, mode="reflect")
    return filtered[:, ::2, ::2, :]


def ms_ssim_f64(img1, img2, max_val=255, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, weights=None,
                scale_fn=ssim_scale_ld):
    """:160-220.  Returns (ms_ssim [B], mssim [levels, B], mcs [levels, B]), float64."""
    w = np.array(weights if weights else DEFAULT_WEIGHTS, dtype=np.float64)
    levels = w.size
    im1, im2 = np.asarray(img1, np.float64), np.asarray(img2, np.float64)
    mssim, mcs = [], []
    for i in range(levels):
        s, c = scale_fn(im1, im2, max_val=max_val, filter_size=filter_size, filter_sigma=filter_sigma, k1=k1, k2=k2)
        mssim.append(s)
        mcs.append(c)
        if i + 1 < levels:
            im1, im2 = downsample2_ndimage(im1), downsample2_ndimage(im2)
    mssim, mcs = np.array(mssim), np.array(mcs)
    value = np.prod(mcs[:levels - 1] ** w[:levels - 1, None], axis=0) * (mssim[levels - 1] ** w[levels - 1])
    return value, mssim, mcs


def mse_ld(img1, img2):
    """:6-16 as a long double mean over (H, W, C); float64 [B]."""
    a, b = np.asarray(img1).astype(LD), np.asarray(img2).astype(LD)
    d = a - b
    return (d * d).mean(axis=(1, 2, 3)).astype(np.float64)


def ssim_scale_error_bound(size, M, max_val=255, k1=0.01, k2=0.03, n_per_image=1, n_partials=1):
    """Absolute bound on |ssim - ssim_ref| and |cs - cs_ref| for one scale computed in float64 by direct sums -- the
    kernel's separable fma chains, or vbq_oracle's separable NumPy sums -- with pixels |x|, |y| <= M.  u = 2^-53.

      window        each 1-D factor e_i / sum(e) is off by <= (size + 3) u relative, a 2-D tap by <= (2 size + 7) u
      planes        2 size rounded products / adds (fma: one rounding per tap; NumPy: two), weights summing to 1:
                    E_mu <= (6 size + 8) u M, and E_sq <= (6 size + 8) u M^2 for x^2, y^2, xy
      sigma         s = E[xy] - mu1 mu2:  E_s <= E_sq + 2 M E_mu + 2 u M^2
      cs            v1 = 2 s12 + c2, v2 = s11 + s22 + c2 >= c2 and |v1| <= v2:  |d cs| <= 4 E_s / c2 + 4 u
      ssim          A = 2 mu12 + c1, D = mu11 + mu22 + c1 >= c1, |A| <= D:
                    |d ssim| <= (8 M E_mu + 4 u M^2) / c1 + 6 u + |d cs|
      means         |maps| <= 1; a tree over 256 lanes of each 16 x 16 tile, a fixed-order sum of n_partials tile partials
                    (pairwise in NumPy): (ceil(log2 n) + 20 + n_partials / 256) u

    The reference's own error (long double, u = 2^-64) is below 1e-3 of this.  Both quotients are bounded by 1 in
    magnitude and can be near 0, so the bound is absolute; with the default constants it stays below 1e-9."""
    u = 2.0 ** -53
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    e_mu = (6 * size + 8) * u * M
    e_sq = (6 * size + 8) * u * M * M
    e_s = e_sq + 2 * M * e_mu + 2 * u * M * M
    mean = (np.ceil(np.log2(max(n_per_image, 2))) + 20 + n_partials / 256.0) * u
    b_cs = 4 * e_s / c2 + 4 * u + mean
    b_ssim = (8 * M * e_mu + 4 * u * M * M) / c1 + 6 * u + b_cs + mean
    return b_ssim, b_cs
