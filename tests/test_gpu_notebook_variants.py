"""Every kernel that vbq_quantize_notebook_f64 can route to, against the f64 brute force of the notebook's own arithmetic.

The entry point picks one of fourteen kernels per bit depth from its arguments (vbq_amd/csrc/vbq_notebook.hip):

    k_quant_notebook<N>                  a beta outside [1e-12, 1e18], or a negative beta among 1-2 betas  ("literal")
    k_quant_notebook_fast<N>             3-5 betas, or N != 10, or a sweep the threshold kernel refuses     ("fast")
    k_quant_notebook_pruned<N, 1|2, V>   1 or 2 non-negative betas                                          ("pruned", K1np)
    k_quant_notebook_hull<V, CW, NF, BUF>  N = 10, 6-64 eligible betas, eight instances                     ("hull", K1nt)

in chunks of 64 betas, on a persistent grid, with a paired-load path, and with per-element escapes inside the hull kernel.
The rule for all of them is bit-for-bit equality, index and value planes, with compress_coordinates (ipynb:429-443: f64 scan
of all 2^(N+1)-1 code points, first minimum wins), here `oracle.c_oracle.compress_coordinates`, which
tests/test_notebook_f64.py pins to NumPy on the same inputs (oracle/notebook_cases.py): exact code-point hits, mid-points,
means far outside, extreme sigmas, and the non-finite / out-of-range classes (sigma 0, negative, subnormal or overflowing
squares, inf, NaN; mean NaN, +-inf, +-3e38, -0.0) shuffled among ordinary elements."""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import c_oracle as CO
from oracle import notebook_cases as NC
from oracle import vbq_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
THREADS = 8
W = 4000                                                     # brute-force window of the multi-million-element cases


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    from vbq_amd import ops as _ops
    t0 = time.perf_counter()
    yield _ops
    print(f"\n[test_gpu_notebook_variants] {time.perf_counter() - t0:.1f} s")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


class Case:
    """One input array on host and device, its code book, and the brute force per beta (computed once, sliced after)."""

    def __init__(self, seed, n_random, N):
        rng = np.random.default_rng(seed)
        self.N = N
        self.pts, self.lens, means, stds, self.scale = NC.case(rng, n_random, N)
        if means.size % 2:
            means, stds = means[:-1], stds[:-1]                # even length: the slices below then fix parity and alignment
        self.means, self.stds = means, stds
        self.n = means.size
        self.d_means, self.d_stds, self.d_pts = dev(means), dev(stds), dev(self.pts)
        assert self.d_means.data_ptr() % 8 == 0 and self.d_stds.data_ptr() % 8 == 0
        self.r2s = O.level_major_to_rank(N)
        self._ref = {}

    def ref(self, beta):
        """(rank int64 [n], value f32 [n]) of the 2^(N+1)-1 point brute force."""
        beta = float(beta)
        if beta not in self._ref:
            v, slot = CO.compress_coordinates(self.means, self.stds, beta, self.pts, self.lens, threads=THREADS)
            self._ref[beta] = (self.r2s[slot], v)
        return self._ref[beta]

    def check(self, ops, betas, sl=slice(None), want_values=True, out_idx=None):
        m, s = self.d_means[sl], self.d_stds[sl]
        idx, val = ops.quantize_notebook(m, s, self.d_pts, betas, N=self.N, want_values=want_values, out_idx=out_idx)
        torch.cuda.synchronize()
        assert tuple(idx.shape) == (len(betas), m.numel()) and (val is None) == (not want_values)
        idx_h = idx.cpu().numpy().astype(np.int64)
        val_h = val.cpu().numpy() if want_values else None
        for i, b in enumerate(betas):
            rank, v = self.ref(b)
            rank, v = rank[sl], v[sl]
            bad = np.flatnonzero(idx_h[i] != rank)
            assert bad.size == 0, (
                f"N={self.N} {len(betas)} betas, plane {i} (beta {b!r}), slice {sl}, values {want_values}: {bad.size} of "
                f"{rank.size} indices differ; first at {bad[:4]}: mean {self.means[sl][bad[:4]]} sigma {self.stds[sl][bad[:4]]} "
                f"got {idx_h[i][bad[:4]]} want {rank[bad[:4]]}")
            if want_values:
                assert np.array_equal(val_h[i].view(np.uint32), v.view(np.uint32)), (self.N, len(betas), i, b, sl)
        return idx, val


# slices of an even-length, 8-byte aligned array: even / odd length, base pointer on / half a pair off
EVEN, ODD, OFF_ODD, OFF_EVEN = slice(None), slice(None, -1), slice(1, None), slice(1, -1)


@pytest.fixture(scope="module")
def case10():
    return Case(seed=2024, n_random=2000, N=10)


def _refusal_sweeps():
    """The shapes the threshold kernel hands back (tests/test_gpu_twopass.py::test_notebook_threshold_kernel_sweeps)."""
    return [NC.NB50[:5],                                              # too short
            [1.0, 1.0, 2.0, 3.0, 5.0, 9.0, 17.0],                     # repeated value
            [1.0, 1.0 + 2.0 ** -9, 2.0, 4.0, 8.0, 16.0],              # two betas in one bucket
            [1e-7, 1e-3, 1.0, 1e3, 1e6, 1e9, 1e12]]                   # more than 24 octaves


def test_inputs_reach_the_hull_kernels_escapes(case10):
    """The planted sigmas fall on both sides of both bounds of the threshold kernel's sigma^2 range, for every sweep
    length it takes here: the whole-element escape is exercised, not hoped for."""
    with np.errstate(all="ignore"):
        var = case10.stds * case10.stds
    assert var.dtype == np.float32
    for L in (6, 31, 32, 33, 47, 48, 50, 55, 56, 64):
        lo, hi = NC.hull_var_bounds(NC.log_sweep(L))
        assert (var < lo).any() and (var >= lo).any() and (var > hi).any() and (var <= hi).any(), (L, lo, hi)
        inside = (var >= lo) & (var <= hi) & np.isfinite(case10.means)
        assert inside.sum() > 0.9 * var.size                                   # ... and the hull path itself does the bulk
    assert np.isnan(var).any() and np.isinf(var).any() and (var == 0).any()
    assert ((var > 0) & (var < np.finfo(np.float32).tiny)).any()               # subnormal sigma^2


# one row of the routing table per entry: (name, betas)
def _routing_lists():
    ls = NC.log_sweep
    out = [("pruned<1>", [0.7]), ("pruned<1> zero beta", [0.0]), ("literal, one negative beta", [-1e4]),
           ("pruned<2>", [0.02, 30.0]), ("pruned<2> other order", [30.0, 0.02]), ("pruned<2> one zero", [0.0, 3.0]),
           ("literal, one of two negative", [-0.5, 3.0]), ("literal, one of two negative, other order", [3.0, -0.5]),
           ("pruned<2> tiny and huge beta", [1e-13, 1e19]),
           ("fast, 3", ls(3)), ("fast, 5", ls(5))]
    for L in (6, 31, 32, 33, 47, 48, 50, 55, 56, 64):
        out.append((f"hull, {L}", ls(L)))
    out.append(("literal, many betas with 1e-13 and 1e19", ls(12) + [1e-13, 1e19]))
    out.append(("literal, many betas with negative ones and zero", ls(7) + [-1e4, 0.0, -1e-3]))
    for i, sw in enumerate(_refusal_sweeps()):
        out.append((f"fast, refused sweep {i}", sw))
    return out


@pytest.mark.parametrize("name,betas", _routing_lists(), ids=[n for n, _ in _routing_lists()])
def test_routing_matrix_n10(ops, case10, name, betas):
    """Each row of the routing table at N = 10: odd and even n, base pointer on and one element off, with and without the
    value plane; sweeps also reversed and permuted."""
    for want_values in (True, False):
        for sl in (EVEN, ODD, OFF_ODD, OFF_EVEN):
            case10.check(ops, betas, sl, want_values)
    if len(betas) >= 3:
        rng = np.random.default_rng(len(betas))
        for order in (betas[::-1], [betas[i] for i in rng.permutation(len(betas))]):
            for want_values in (True, False):
                case10.check(ops, order, EVEN, want_values)
                case10.check(ops, order, OFF_ODD, want_values)


@pytest.mark.parametrize("count", [65, 66, 70, 96, 128, 130])
def test_beta_chunks(ops, count):
    """More than 64 betas: chunks of 64 (the last one a pruned call for 65 / 66 / 130, a hull call for 70 / 96 / 128; with
    odd n the second chunk's value plane is 4-byte but not 8-byte aligned).  Every plane is checked, and a canary row after
    the last plane of a caller-supplied out_idx stays untouched."""
    case = Case(seed=65, n_random=300, N=10)
    betas = NC.log_sweep(count)
    for sl in (EVEN, ODD):
        n = case.d_means[sl].numel()
        for want_values in (True, False):
            buf = torch.full((count + 1, n), -21555, dtype=torch.int16, device="cuda").view(torch.uint16)
            idx, _ = case.check(ops, betas, sl, want_values, out_idx=buf[:count])
            assert idx.data_ptr() == buf.data_ptr()
            assert bool((buf[count].view(torch.int16) == -21555).all()), "canary row after the last plane was written"


@pytest.mark.parametrize("N", [4, 5, 6, 7, 8, 9])
def test_every_bit_depth(ops, N):
    """N = 4..9 through the literal kernel (negative beta, out-of-range beta), the fast kernel (3 betas; 50 betas, which at
    N != 10 stay with `fast` in one chunk) and the pruned kernel (1 and 2 betas), values both ways, odd and even n."""
    case = Case(seed=40 + N, n_random=3000, N=N)
    lists = [[-0.5], [3.0, -1e4], NC.log_sweep(4) + [1e19, -2.0], NC.log_sweep(3), NC.NB50, [0.3], [0.0], [0.02, 30.0], [30.0, 0.0]]
    for betas in lists:
        for want_values in (True, False):
            for sl in (EVEN, OFF_ODD):
                case.check(ops, betas, sl, want_values)


def _big_inputs(n, seed, plant_at):
    """Ordinary elements with the adversarial + non-finite set planted at the given starts (host arrays)."""
    rng = np.random.default_rng(seed)
    pts, lens, am, asd, scale = NC.case(rng, 500, 10)
    means = (scale * rng.standard_normal(n, dtype=np.float32) * np.float32(1.2)).astype(np.float32)
    stds = (np.exp(rng.standard_normal(n, dtype=np.float32) * np.float32(1.5) - np.float32(2.0)) * scale).astype(np.float32)
    k = min(am.size, W)
    for s in plant_at:
        s = int(min(max(0, s), n - k))
        means[s:s + k], stds[s:s + k] = am[:k], asd[:k]
    return pts, lens, means, stds


@pytest.mark.timeout(900)
def test_past_one_trip_of_the_persistent_grid(ops):
    """n = 3 000 001: every workgroup of the capped grids takes a second trip (and most a third).  The brute force on
    windows at the start, the end and across cap * 512 and 2 * cap * 512 elements; the full planes through independent
    paths: the index plane of a sweep equals the plane the one-beta pruned call gives for the same beta, and the value
    plane equals the code book read at the index."""
    N, n = 10, 3_000_001
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    caps = {"pruned": cus * 12, "hull, values": cus * 2 * 2, "hull, <= 32 betas": cus * 4 * 2, "hull, > 32 betas": cus * 3 * 2}
    assert all(n > c * 512 for c in caps.values()), (cus, caps)
    marks = sorted({m * c * 512 - W // 2 for c in caps.values() for m in (1, 2) if m * c * 512 + W < n})
    assert len(marks) >= 4
    starts = sorted({0, n - W, *marks})
    pts, lens, means, stds = _big_inputs(n, 5, starts)
    dm, ds, dp = dev(means), dev(stds), dev(pts)
    r2s = O.level_major_to_rank(N)
    s_of_r = np.empty_like(r2s)
    s_of_r[r2s] = np.arange(r2s.size)
    by_rank = torch.from_numpy(pts[s_of_r].astype(np.float32)).cuda()              # f32 code point of every rank
    sweep50, sweep32 = NC.NB50, NC.log_sweep(32)

    def brute(idx, val, betas, which):
        for s in starts:
            for k in which:
                v, slot = CO.compress_coordinates(means[s:s + W], stds[s:s + W], betas[k], pts, lens, threads=THREADS)
                got = idx[k, s:s + W].cpu().numpy().astype(np.int64)
                assert np.array_equal(got, r2s[slot]), (len(betas), k, s, int((got != r2s[slot]).sum()))
                if val is not None:
                    assert np.array_equal(val[k, s:s + W].cpu().numpy().view(np.uint32), v.view(np.uint32)), (len(betas), k, s)

    def values_follow_indices(idx, val):
        for k in range(idx.shape[0]):
            assert torch.equal(by_rank[idx[k].to(torch.int64)].view(torch.int32), val[k].view(torch.int32)), k

    # K1np, one beta, with values
    single = {}
    for k in (0, 12, 25, 37, 49):
        i1, v1 = ops.quantize_notebook(dm, ds, dp, [sweep50[k]], N=N)
        brute(i1, v1, [sweep50[k]], [0])
        values_follow_indices(i1, v1)
        single[k] = i1[0].clone()
    # K1nt, 50 betas with values
    idx, val = ops.quantize_notebook(dm, ds, dp, sweep50, N=N)
    brute(idx, val, sweep50, (0, 12, 25, 37, 49))
    values_follow_indices(idx, val)
    for k, want in single.items():
        assert torch.equal(idx[k].view(torch.int16), want.view(torch.int16)), k
    del val
    # K1nt, 50 and 32 betas without values
    idx2, none = ops.quantize_notebook(dm, ds, dp, sweep50, N=N, want_values=False)
    assert none is None and torch.equal(idx2.view(torch.int16), idx.view(torch.int16))
    del idx, idx2
    idx3, _ = ops.quantize_notebook(dm, ds, dp, sweep32, N=N, want_values=False)
    brute(idx3, None, sweep32, (0, 8, 16, 24, 31))
    for k in (0, 16, 31):
        i1, _ = ops.quantize_notebook(dm, ds, dp, [sweep32[k]], N=N, want_values=False)
        assert torch.equal(idx3[k].view(torch.int16), i1[0].view(torch.int16)), k


def _n_rows_beyond_4gb(L, rows_within):
    """The smallest odd n (an even number plus 1) for which `rows_within` rows of n u16 indices exceed 2^32 bytes."""
    n = -(-(1 << 32) // (2 * rows_within))
    n += n % 2
    return n + 1


@pytest.mark.timeout(900)
@pytest.mark.parametrize("rows_within", [50, 47])
def test_index_rows_beyond_4gb(ops, rows_within):
    """50 betas without values and more than 2^32 bytes of index rows: the instance of the threshold kernel that must not
    use the 4 GB buffer descriptor.  With n just above 2^32 / 100 row 49 crosses the 4 GB mark about a hundred elements
    before its end.  With n just above 2^32 / 94 row 47 -- the last row that the straight block of six full words stores
    (rows 48 and 49 go through plain 64-bit addresses in every instance) -- STARTS beyond the mark: the smallest size at
    which a 32-bit row offset wraps, and so the smallest at which taking the descriptor path by mistake shows.  Windows at
    the start, in the middle and over the last elements (the crossing included), and every row's histogram counts n."""
    N, L = 10, 50
    n = _n_rows_beyond_4gb(L, rows_within)
    assert n % 2 == 1 and 2 * rows_within * n > 0xffffffff and 2 * rows_within * (n - 3) <= 0xffffffff
    cross = (1 << 31) - (rows_within - 1) * n                   # element of the last row within 4 GB whose index starts at byte 2^32
    assert n - W < cross < n
    dvc = torch.device("cuda")
    g = torch.Generator(device=dvc).manual_seed(7)
    rng = np.random.default_rng(7)
    pts, lens, am, asd, scale = NC.case(rng, 500, 10)
    mu = torch.randn(n, device=dvc, generator=g).mul_(1.2 * float(scale))
    sg = torch.randn(n, device=dvc, generator=g).mul_(1.5).sub_(2.0).exp_().mul_(float(scale))
    k = min(am.size, W)
    starts = (0, n // 2, n - W)
    for s in starts:                                                             # the adversarial + non-finite set in every window
        mu[s:s + k] = dev(am[:k])
        sg[s:s + k] = dev(asd[:k])
    idx, _ = ops.quantize_notebook(mu, sg, dev(pts), NC.NB50, N=N, want_values=False)
    torch.cuda.synchronize()
    r2s = O.level_major_to_rank(N)
    for s in starts:
        m, sd = mu[s:s + W].cpu().numpy(), sg[s:s + W].cpu().numpy()
        for kb in (0, 1, 12, 25, 37, 46, 47, 48, 49):
            _, slot = CO.compress_coordinates(m, sd, NC.NB50[kb], pts, lens, threads=THREADS)
            got = idx[kb, s:s + W].cpu().numpy().astype(np.int64)
            assert np.array_equal(got, r2s[slot]), (kb, s, int((got != r2s[slot]).sum()))
    cnt = ops.histogram(idx, 1, N=N)
    assert torch.all(cnt.sum(dim=-1) == n)


def test_tiny_n(ops, case10):
    """n = 1, 2, 3 (one half-filled pair, a grid of one workgroup) for each kernel family, values both ways; n = 0 gives
    empty planes."""
    lists = [[0.7], [0.02, 30.0], NC.log_sweep(5), NC.log_sweep(32), NC.NB50, [-0.5]]
    starts = [0, 1, 500, 1001, 2002, 3003, case10.n - 3]
    for betas in lists:
        for want_values in (True, False):
            for n in (1, 2, 3):
                for s in starts:
                    case10.check(ops, betas, slice(s, s + n), want_values)
            idx, val = ops.quantize_notebook(case10.d_means[:0], case10.d_stds[:0], case10.d_pts, betas, N=10, want_values=want_values)
            assert tuple(idx.shape) == (len(betas), 0) and (val is None or tuple(val.shape) == (len(betas), 0))
