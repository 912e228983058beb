"""Input builders for the tests of the notebook solve (compress_coordinates, ipynb:429-443), shared by the CPU test of the
reference (tests/test_notebook_f64.py) and the GPU tests of the kernels (tests/test_gpu_notebook_variants.py), so that
the reference is pinned to NumPy on the very input classes it is then trusted on."""
import numpy as np

from . import vbq_oracle as O

F32 = np.float32
NB50 = [float(b) for b in np.exp(np.linspace(np.log(0.01), np.log(1e5), 50))]          # ipynb cell 32
NAN_NEG = np.array([0xFFC00000], np.uint32).view(F32)[0]                                 # a quiet NaN with the sign bit set
SUBNORMAL_MIN = np.array([1], np.uint32).view(F32)[0]                                    # 2^-149


def log_sweep(count, lo=0.01, hi=1e5):
    """`count` betas log-spaced over the notebook's range."""
    return [float(b) for b in np.exp(np.linspace(np.log(lo), np.log(hi), count))]


def adversarial(rng, n, N):
    """_notebook_case of tests/test_gpu_twopass.py for any bit depth: every code point as a mean, every mid-point of sorted
    neighbours (as f32), points 40 scales outside the code book, 0.0, n heavy-tailed random means; sigmas log-normal with
    planted 0.99999994 * scale, 1e-6 * scale and 1e4 * scale.  Returns (pts f64 [T], lens int [T], means f32, stds f32, scale)."""
    scale = F32(np.exp(rng.uniform(np.log(0.2), np.log(5.0))))
    pts, lens = O.notebook_code_book(scale, N)
    srt = np.sort(pts)
    mids = (0.5 * (srt[:-1] + srt[1:])).astype(F32)
    means = np.concatenate([srt.astype(F32), mids, F32([srt[0] - 40 * scale, srt[-1] + 40 * scale, 0.0]),
                            (scale * rng.standard_t(4, n)).astype(F32)]).astype(F32)
    stds = (np.exp(rng.normal(-2, 1.5, means.size)) * scale).astype(F32)
    stds[::7] = F32(0.99999994) * scale
    stds[3::101] = F32(1e-6) * scale
    stds[5::103] = F32(1e4) * scale
    return pts, lens, means, stds, scale


def special_sigmas(scale):
    """sigma = 0, negative, squares that are subnormal / zero / below and above the hull kernel's range (1e19 squared is
    1e38: still finite), squares that overflow f32 (2e19, 3e38), inf, NaN of both signs, the smallest subnormal."""
    with np.errstate(over="ignore"):
        return np.array([0.0, -float(scale), 1e-23, 1e-20, 1e-16, 1e15, 1e19, 2e19, 3e38, np.inf, np.nan, NAN_NEG, SUBNORMAL_MIN],
                        dtype=F32)


def special_means():
    return np.array([np.nan, NAN_NEG, np.inf, -np.inf, 3e38, -3e38, -0.0], dtype=F32)


def nonfinite(rng, pts, scale, reps=6):
    """Elements of their own (to be appended to ordinary ones): every special sigma under `reps` ordinary means (the first a
    code point, the second a mid-point), every special mean under `reps` ordinary sigmas, and the cross product of the two
    once.  Returns (means f32, stds f32)."""
    ss, sm = special_sigmas(scale), special_means()
    srt = np.sort(pts)

    def ordinary_means(k):
        m = (scale * rng.standard_t(4, k)).astype(F32)
        j = int(rng.integers(0, srt.size - 1))
        m[0] = F32(srt[j])
        if k > 1:
            m[1] = F32(0.5 * (srt[j] + srt[j + 1]))
        return m
    means, stds = [], []
    for s in ss:
        means.append(ordinary_means(reps))
        stds.append(np.full(reps, s, F32))
    for m in sm:
        means.append(np.full(reps, m, F32))
        stds.append((np.exp(rng.normal(-2, 1.5, reps)) * scale).astype(F32))
    means.append(np.repeat(sm, ss.size))
    stds.append(np.tile(ss, sm.size))
    return np.concatenate(means).astype(F32), np.concatenate(stds).astype(F32)


def case(rng, n, N, shuffle=True):
    """adversarial + nonfinite elements in one array, shuffled so that special elements share waves with ordinary ones.
    Returns (pts, lens, means, stds, scale)."""
    pts, lens, means, stds, scale = adversarial(rng, n, N)
    m2, s2 = nonfinite(rng, pts, scale)
    means, stds = np.concatenate([means, m2]), np.concatenate([stds, s2])
    if shuffle:
        p = rng.permutation(means.size)
        means, stds = means[p], stds[p]
    return pts, lens, np.ascontiguousarray(means), np.ascontiguousarray(stds), scale


def hull_var_bounds(betas):
    """[var_lo, var_hi] of the threshold kernel for a sweep, in the f32 arithmetic of its launcher: sigma^2 outside takes
    the literal scan for the whole element."""
    b = np.sort((2.0 * np.asarray(betas, np.float64)).astype(F32))
    with np.errstate(over="ignore", under="ignore"):
        lo = np.maximum(F32(4e-38) / b[0], F32(1e-30))
        hi = np.minimum(F32(1e38) / b[-1], F32(1e30))
    return F32(lo), F32(hi)


def numpy_reference(means, stds, beta, pts, lens):
    """What the notebook runs: (slot int64, value f32) from NumPy itself, and the dtype of (2 beta) s^2 (must be f32)."""
    m, s = np.ascontiguousarray(means, F32), np.ascontiguousarray(stds, F32)
    with np.errstate(all="ignore"):
        pen_dtype = ((2 * float(beta)) * s[:4] ** 2).dtype
        slot = O.compress_coordinates_idx(m, s, float(beta), pts, lens)
        val = O.compress_coordinates(m, s, float(beta), pts, lens)
    return slot, val, pen_dtype
