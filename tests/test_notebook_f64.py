"""The checker of the notebook solve against what the notebook runs.

tests/test_gpu_notebook_variants.py compares every kernel of vbq_quantize_notebook_f64 with the C brute force
`oracle.c_oracle.compress_coordinates` -- the only reference fast enough for millions of elements.  Here that C code is
pinned to NumPy (`oracle.vbq_oracle.compress_coordinates[_idx]`, ipynb:429-443 as written) on the input classes the GPU
tests use: every bit depth 4..10, the adversarial means and sigmas, non-finite and out-of-range means and sigmas, and
negative / zero / tiny / huge betas.  Where the two disagreed NumPy would be right."""
import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import notebook_cases as NC

BETAS = [1.0, 0.01, 1e5, 0.0, -0.5, -1e4, 1e-13, 1e19, 1e-30, 3e38, 1e39, -1e39]


def test_builders_hold_what_they_promise():
    rng = np.random.default_rng(1)
    pts, lens, means, stds, scale = NC.case(rng, 500, 6)
    T = 2 ** 7 - 1
    assert pts.shape == (T,) and lens.shape == (T,) and pts.dtype == np.float64
    assert means.dtype == np.float32 and stds.dtype == np.float32 and means.shape == stds.shape
    assert means.size == T + (T - 1) + 3 + 500 + NC.nonfinite(rng, pts, scale)[0].size
    for c in np.sort(pts):
        assert np.float32(c) in means
    nan_s, nan_m = np.isnan(stds), np.isnan(means)
    assert np.signbit(stds[nan_s]).any() and not np.signbit(stds[nan_s]).all()              # NaN of both signs
    assert np.signbit(means[nan_m]).any() and not np.signbit(means[nan_m]).all()
    assert (nan_s & nan_m).any() and (np.isinf(stds) & np.isinf(means)).any()               # the cross product
    for v in NC.special_sigmas(scale):
        assert np.isnan(v) or (stds == v).sum() >= 6
    for v in NC.special_means():
        assert np.isnan(v) or ((means == v) & (np.signbit(means) == np.signbit(v))).sum() >= 6
    with np.errstate(all="ignore"):
        var = stds * stds
    assert var.dtype == np.float32
    assert np.isfinite(var[stds == np.float32(1e19)]).all()                                  # 1e38: the largest finite class
    assert np.isinf(var[stds == np.float32(2e19)]).all()                                     # the f32 square overflows
    sub = var[stds == np.float32(1e-20)]
    assert (sub > 0).all() and (sub < np.finfo(np.float32).tiny).all()                       # subnormal sigma^2
    assert (var[stds == NC.SUBNORMAL_MIN] == 0).all()
    # both sides of both bounds of the threshold kernel, for the notebook's sweep
    lo, hi = NC.hull_var_bounds(NC.NB50)
    assert lo == np.float32(1e-30) and hi == np.float32(1e30)
    assert (var < lo).any() and (var >= lo).any() and (var > hi).any() and (var <= hi).any()


@pytest.mark.parametrize("N", [4, 5, 6, 7, 8, 9, 10])
def test_c_brute_force_is_numpy_on_adversarial_and_nonfinite_inputs(N):
    rng = np.random.default_rng(100 + N)
    pts, lens, means, stds, scale = NC.case(rng, 1500 if N < 10 else 600, N)
    for beta in BETAS:
        slot, val, pen_dtype = NC.numpy_reference(means, stds, beta, pts, lens)
        assert pen_dtype == np.float32, "(2 beta) sigma^2 must stay f32, as under NumPy 1.17"
        assert val.dtype == np.float32
        cval, cslot = CO.compress_coordinates(means, stds, beta, pts, lens, threads=4)
        bad = np.flatnonzero(cslot != slot)
        assert bad.size == 0, (N, beta, bad[:5], means[bad[:5]], stds[bad[:5]], slot[bad[:5]], cslot[bad[:5]])
        assert np.array_equal(cval.view(np.uint32), val.view(np.uint32)), (N, beta)
        assert np.array_equal(pts[slot].astype(np.float32), val)


def test_nan_rule_of_the_reference():
    """np.argmin returns the first NaN.  The penalty of slot 0 is w * 0, which is NaN for w = +-inf or NaN, so every element
    whose (2 beta) sigma^2 is not finite -- and every NaN mean -- gets slot 0 (the root); the kernels must do the same."""
    rng = np.random.default_rng(3)
    pts, lens, _, _, scale = NC.adversarial(rng, 10, 10)
    m = np.float32([0.3, 0.3, 0.3, 0.3, np.nan, np.inf, -np.inf, 0.3]) * scale
    s = np.float32([np.inf, 2e19, np.nan, 3e38, 1.0, 1.0, 1.0, 0.0])
    for beta in (1.0, -1.0):
        slot, _, _ = NC.numpy_reference(m, s, beta, pts, lens)
        _, cslot = CO.compress_coordinates(m, s, beta, pts, lens)
        assert np.array_equal(slot[:7], np.zeros(7, np.int64)) and np.array_equal(cslot, slot)
        assert slot[7] == np.argmin((pts - np.float64(m[7])) ** 2)                          # sigma = 0: the nearest point
