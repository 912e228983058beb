"""The xi-space encoder's two kernels (vbq_xi.hip) at their edges: vbq_xi_intervals_f64 bit for bit against a plain
float64 restatement of the reference's numba loop (utils.py:215-260) and the closed form of vbq_oracle, plus an exact
property check with fractions.Fraction; vbq_xi_select_f64 against a NumPy restatement of the selection tail of
encode_vectorized (utils.py:288-303), ties, infinities and NaN included."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import vbq_oracle as O  # noqa: E402

gpu = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _intervals_loop(x, N):
    """utils.get_all_N_bit_intervals, the bit-by-bit truncation loop, one Python float64 operation per numba one."""
    K = len(x)
    left, right = np.empty((N + 1, K)), np.empty((N + 1, K))
    for k in range(K):
        for n in range(N + 1):
            if n == 0:
                left[n, k] = right[n, k] = 0.5
                continue
            x_k = float(x[k])
            width = 2.0 ** (-n)
            offset = width * 0.5
            lo, hi = offset, 1.0 - offset
            if x_k < lo:
                l = r = lo
            elif x_k > hi:
                l = r = hi
            else:
                shifted = x_k - offset
                rem = shifted
                for i in range(1, n + 1):
                    diff = rem - 2.0 ** (-i)
                    if diff >= 0.0:
                        rem = diff
                l = (shifted - rem) + offset
                r = l + width
            left[n, k], right[n, k] = l, r
    return left, right


def _edge_xs():
    """Every n-bit grid point for n <= 8 (all multiples of 2^-9) and its two neighbours, 0, 1, offset and 1 - offset
    for every n <= 52, subnormals, values outside [0, 1], +-inf and NaN."""
    g = np.arange(0, 513) / 512.0
    offs = 2.0 ** -np.arange(1, 54, dtype=np.float64)
    base = np.concatenate([g, offs, 1 - offs, [0.0, -0.0, 1.0, 5e-324, 2.2e-308, 1e-310, -5e-324, -1e-3, -1.0, 1.0 + 2e-16,
                                                 1.5, 2.0, 1e300, -np.inf, np.inf, np.nan, 0.3, 1 / 3.0, 0.7]])
    fin = base[np.isfinite(base)]
    return np.concatenate([base, np.nextafter(fin, -np.inf), np.nextafter(fin, np.inf)])


def _gpu_intervals(x, N):
    from vbq_amd import utils
    left, right = np.empty((N + 1, len(x))), np.empty((N + 1, len(x)))
    utils.get_all_N_bit_intervals(x, N, left, right)
    return left, right


def _same(a, b):
    """Identical float64 arrays: equal values, NaN where the other has NaN, and the same sign on zeros."""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def test_closed_form_equals_the_loop():
    """CPU: vbq_oracle.xi_intervals (closed form) and the loop agree bit for bit on the edge inputs."""
    x = _edge_xs()
    for N in (0, 1, 16, 52):
        L, R = _intervals_loop(x, N)
        l2, r2 = O.xi_intervals(x, N)
        assert np.array_equal(L, l2, equal_nan=True) and np.array_equal(R, r2, equal_nan=True)


def test_interval_properties_exact():
    """CPU, exact rationals: for finite x in (0, 1) and every n >= 1 the endpoints are both the rim grid point
    2^-(n+1) or 1 - 2^-(n+1) (x outside them), or an odd multiple of 2^-(n+1) and right - left = 2^-n exactly (except the
    one right endpoint 1 + 2^-53, which float64 rounds)."""
    x = _edge_xs()
    x = x[np.isfinite(x) & (x > 0) & (x < 1)]
    N = 52
    L, R = _intervals_loop(x, N)
    for k, xk in enumerate(x):
        for n in range(1, N + 1):
            l, r = Fraction(L[n, k]), Fraction(R[n, k])
            off = Fraction(1, 2 ** (n + 1))
            if Fraction(float(xk)) < off or Fraction(float(xk)) > 1 - off:
                assert l == r and l in (off, 1 - off)
            elif n == 52 and r == 1:
                assert l == 1 - off          # left + 2^-52 = 1 + 2^-53 is not a double: the reference rounds it to 1
            else:
                assert r - l == Fraction(1, 2 ** n)
                m = l * 2 ** (n + 1)
                assert m.denominator == 1 and m.numerator % 2 == 1


@gpu
@pytest.mark.parametrize("N", [0, 1, 16, 31, 52])
def test_intervals_edges_bit_exact(N):
    _need_gpu()
    x = _edge_xs()
    L, R = _gpu_intervals(x, N)
    WL, WR = _intervals_loop(x, N)
    assert _same(L, WL) and _same(R, WR)                  # NaN in -> NaN out, as in the reference
    nan = np.isnan(x)
    assert np.all(np.isnan(L[1:, nan])) and np.all(L[0, nan] == 0.5)


@gpu
def test_intervals_refuse_N53_and_grid_stride():
    _need_gpu()
    from vbq_amd._lib import VBQError
    with pytest.raises(VBQError):
        _gpu_intervals(np.array([0.3]), 53)
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.random(1_200_000), _edge_xs()])        # > 4096 x 256 coordinates: the grid-stride loop
    L, R = _gpu_intervals(x, 10)
    WL, WR = O.xi_intervals(x, 10)
    assert np.array_equal(L, WL, equal_nan=True) and np.array_equal(R, WR, equal_nan=True)


# ---- selection ------------------------------------------------------------------------------------------------------

def _select_ref(F, ends, unsq, lamb):
    """utils.py:288-303 as written (NumPy's argmax: the first maximum, and the first NaN if there is one)."""
    N1, K = F.shape[1], F.shape[2]
    cols = np.arange(K)
    argmax = np.argmax(F, axis=0)
    idx = (argmax, np.arange(N1)[:, None], cols[None, :])
    F_max = F[idx]
    with np.errstate(invalid="ignore"):
        reg = F_max - lamb * np.arange(N1)[:, None]
    nb = np.argmax(reg, axis=0)
    return dict(z_hat=unsq[idx][nb, cols], xi_hat=ends[idx][nb, cols], num_bits=nb, f_z_hat=reg[nb, cols])


def _select_gpu(F, ends, unsq, lamb):
    from vbq_amd import _lib, ops
    K, N = F.shape[2], F.shape[1] - 1
    Fd, ed, ud = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in (F, ends, unsq))
    z = torch.empty(K, dtype=torch.float64, device=Fd.device)
    xi = torch.empty_like(z)
    fz = torch.empty_like(z)
    nb = torch.empty(K, dtype=torch.int64, device=Fd.device)
    _lib.check(_lib.lib().vbq_xi_select_f64(ops._ptr(Fd), ops._ptr(ed), ops._ptr(ud), K, N, C.c_double(lamb), ops._ptr(z),
                                            ops._ptr(nb), ops._ptr(xi), ops._ptr(fz), ops._stream(Fd)), "vbq_xi_select_f64")
    return dict(z_hat=z.cpu().numpy(), xi_hat=xi.cpu().numpy(), num_bits=nb.cpu().numpy(), f_z_hat=fz.cpu().numpy())


def _check_select(F, ends, unsq, lamb):
    got, want = _select_gpu(F, ends, unsq, lamb), _select_ref(F, ends, unsq, lamb)
    for key in ("z_hat", "xi_hat", "num_bits", "f_z_hat"):
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    return got


def _setup(K, N, seed):
    rng = np.random.default_rng(seed)
    xi = rng.random(K)
    L, R = O.xi_intervals(xi, N)
    ends = np.stack([L, R])
    unsq = np.log(ends / (1 - ends))                             # a logit "unsquash": distinct values per endpoint
    return rng, xi, ends, unsq


@gpu
@pytest.mark.parametrize("lamb", [0.0, 0.05, -0.3, np.inf])
def test_select_ties_and_infinities(lamb):
    """Equal F at two distinct endpoints (np.argmax keeps the left one), equal regularised F across n (the smaller
    budget), -inf entries and whole -inf columns; lamb = 0, > 0, < 0 and inf (inf * 0 is NaN at n = 0)."""
    _need_gpu()
    K, N = 4000, 16
    rng, xi, ends, unsq = _setup(K, N, 3)
    z = np.log(xi / (1 - xi))
    F = -(unsq - z) ** 2                                         # a smooth objective with its mode at z
    distinct = ends[0] != ends[1]
    tie = distinct & (rng.random((N + 1, K)) < 0.3)
    F[1][tie] = F[0][tie]                                        # left / right ties at distinct endpoints
    # equal regularised F across n: F_max = c + lamb * n on a run of budgets
    cols = rng.random(K) < 0.2
    if np.isfinite(lamb):
        flat = np.maximum(F[0], F[1])[0] + 1.0
        for n in (3, 7, 11):
            F[:, n, cols] = flat[cols] + lamb * n
    F[0][rng.random((N + 1, K)) < 0.05] = -np.inf
    F[1][rng.random((N + 1, K)) < 0.05] = -np.inf
    F[:, :, 5] = -np.inf
    F[:, :, 6] = np.inf
    got = _check_select(F, ends, unsq, lamb)
    assert np.any(tie)
    assert np.any(got["num_bits"] > 0) if np.isfinite(lamb) else np.all(got["num_bits"] == 0)   # inf * 0: NaN at n = 0
    # the public path: the same selection through encode_vectorized, score included
    from vbq_amd import utils
    out = utils.encode_vectorized(lambda zs: F, xi, lamb, squash=lambda v: v, unsquash=lambda e: np.log(e / (1 - e)),
                                  max_bits_per_coord=N)
    want = _select_ref(F, ends, unsq, lamb)
    assert np.array_equal(out["num_bits"], want["num_bits"]) and np.array_equal(out["z_hat"], want["z_hat"])
    assert np.array_equal(out["xi_hat"], want["xi_hat"])
    assert np.array_equal(out["score"], np.sum(want["f_z_hat"]), equal_nan=True)


@gpu
def test_select_left_right_tie_at_distinct_endpoints():
    """fun symmetric about its mode, the mode halfway between two grid points: equal F on both sides at that budget,
    and the left endpoint wins (np.argmax's first maximum)."""
    _need_gpu()
    from vbq_amd import utils
    N = 12
    xi = np.arange(1, 512) / 512.0                                # multiples of 2^-9: midpoints of the 9-bit grid
    out = utils.encode_vectorized(lambda e: -np.abs(e - xi), xi, 0.0, squash=lambda v: v, unsquash=lambda e: e,
                                  max_bits_per_coord=N)
    L, R = O.xi_intervals(xi, N)
    ends = np.stack([L, R])
    want = _select_ref(-np.abs(ends - xi), ends, ends, 0.0)
    assert np.array_equal(out["xi_hat"], want["xi_hat"]) and np.array_equal(out["num_bits"], want["num_bits"])
    got = _check_select(-np.abs(ends - xi), ends, ends, 0.0)
    assert np.array_equal(got["xi_hat"], out["xi_hat"])
    # at n = 9, left and right are equally far from xi; a budget-9 tie must resolve to the left end
    F = np.full_like(ends, -1.0)
    F[:, 9] = 0.0
    got = _check_select(F, ends, ends, 0.0)
    assert np.all(got["num_bits"] == 9) and np.array_equal(got["xi_hat"], L[9])


@gpu
@pytest.mark.parametrize("lamb", [0.0, 0.1])
def test_select_nan_follows_numpy_argmax(lamb):
    """NaN in F at a left endpoint, at a right endpoint and at one budget n: np.argmax returns the first NaN, over the
    pair and over n, so z_hat / xi_hat / num_bits / f_z_hat follow it and the score is NaN."""
    _need_gpu()
    K, N = 3000, 16
    rng, xi, ends, unsq = _setup(K, N, 8)
    F = -(unsq - np.log(xi / (1 - xi))) ** 2
    F[0][rng.random((N + 1, K)) < 0.02] = np.nan                  # left endpoints
    F[1][rng.random((N + 1, K)) < 0.02] = np.nan                  # right endpoints
    F[:, 9, 100:200] = np.nan                                     # one budget, both endpoints
    F[1, 4, 300:400] = np.nan                                     # a right endpoint only, at one budget
    got = _check_select(F, ends, unsq, lamb)
    assert np.all(got["num_bits"][100:200] <= 9) and np.all(np.isnan(got["f_z_hat"][100:200]))
    assert np.all(got["num_bits"][300:400] <= 4) and np.all(np.isnan(got["f_z_hat"][300:400]))
    from vbq_amd import utils
    out = utils.encode_vectorized(lambda zs: F, xi, lamb, squash=lambda v: v, unsquash=lambda e: np.log(e / (1 - e)),
                                  max_bits_per_coord=N)
    assert np.isnan(out["score"]) and np.array_equal(out["num_bits"], got["num_bits"])


@gpu
def test_select_grid_stride_and_large_N():
    _need_gpu()
    K, N = 1_100_000, 20                                         # > 4096 x 256 coordinates
    rng, xi, ends, unsq = _setup(K, N, 12)
    F = -(unsq - np.log(xi / (1 - xi))) ** 2
    _check_select(F, ends, unsq, 0.02)
    rng, xi, ends, unsq = _setup(500, 52, 13)
    with np.errstate(divide="ignore"):
        F = -(unsq - np.log(xi / (1 - xi))) ** 2
    _check_select(F, ends, unsq, 1e-3)
