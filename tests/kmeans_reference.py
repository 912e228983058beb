"""NumPy restatements of the exact 1-D k-means DP of include/vbq_kmeans.h, and the launch plan of vbq_amd/kmeans/vbqk_dp.hip.

Everything takes the prefix sums (S1, S2 f64 [n + 1], shift) the C call takes, so that a test hands the SAME sums to the kernel
and to the restatement and compares bit for bit.  Three evaluations of one definition:

    dp_recursive   the recursion of the header, literally: solve(jl, jh, il, ih) with a Python scan in ascending i
    dp_levels      the same nodes taken depth by depth, all nodes of a depth in one vectorised step (what the kernel does; fast
                   enough for n in the hundred thousands).  Identical to dp_recursive bit for bit: a node's il / ih are the
                   back-pointers at jl - 1 / jh + 1, and "first strict minimum in ascending i" is the first occurrence of the minimum
    dp_brute       O(K n^2): every i in [q, j] for every j, first minimum.  No monotonicity assumed.

cost(i, j) = (S2[j] - S2[i-1]) - s * s / (j - i + 1), s = S1[j] - S1[i-1]: NumPy rounds every operation separately in f64 and
never contracts, which is what the kernel does (-ffp-contract=off and explicit round-to-nearest intrinsics).
Importable without a GPU."""
import sys

import numpy as np

EPS = float(np.finfo(np.float64).eps)

# ---- the launch plan of vbqk_dp.hip, restated (tests/test_kmeans_host.py holds it against the library and the source)
THREADS = 512
WAVE_SCAN = 64            # a node with this many candidates or more is scanned by a whole wave
QUEUE = 2048              # such nodes per round; the rest are scanned by their lane
LDS_BYTES = 160 * 1024
LDS_HEAD = 16 + 4 * QUEUE
ROWS_IN_LDS_MAX_N = (LDS_BYTES - LDS_HEAD) // 32 - 1          # 4 (n + 1) doubles beside the queue: n <= 4862
MAX_LEVELS, MAX_K = 64, 1024


def rows_in_lds(n):
    return n <= ROWS_IN_LDS_MAX_N


def slice_bytes(n, Kmax):
    """Workspace of one channel in flight: the back-pointers, and the two value rows when they do not live in LDS."""
    bp = (4 * Kmax * (n + 1) + 15) // 16 * 16
    return bp + (0 if rows_in_lds(n) else 16 * (n + 1))


def root_scan_len(q, n):
    """Candidates of the root node of layer q >= 2: i in [q, (q + n) // 2]."""
    return (q + n) // 2 - q + 1


# ---- the inputs
def sums_of(x_sorted):
    """(shift, S1, S2) of one channel's f32 samples sorted ascending, with np.cumsum."""
    x = np.asarray(x_sorted)
    assert x.dtype == np.float32 and x.ndim == 1 and x.size >= 1
    n = x.size
    shift = np.float64(x[n // 2])                 # x[n // 2 + 1] counting from 1: the upper median
    y = x.astype(np.float64) - shift
    S1 = np.concatenate([[0.0], np.cumsum(y)])
    S2 = np.concatenate([[0.0], np.cumsum(y * y)])
    return shift, S1, S2


def cost(S1, S2, i, j):
    """cost(i, j) for an integer (array) i and an integer (array) j."""
    s = S1[j] - S1[i - 1]
    return (S2[j] - S2[i - 1]) - s * s / np.asarray(j - i + 1, np.float64)


def _first_row(n):
    D = np.full(n + 1, np.inf)
    D[0] = 0.0
    return D


# ---- the recursion, literally
def _layer_recursive(Dprev, S1, S2, q, n):
    Dcur = np.full(n + 1, np.nan)
    Aq = np.zeros(n + 1, np.int64)

    def solve(jl, jh, il, ih):
        if jl > jh:
            return
        j = (jl + jh) // 2
        best, bi = None, None
        for i in range(max(il, q), min(ih, j) + 1):
            v = Dprev[i - 1] + cost(S1, S2, i, j)
            if best is None or v < best:
                best, bi = v, i
        Dcur[j], Aq[j] = best, bi
        solve(jl, j - 1, il, bi)
        solve(j + 1, jh, bi, ih)
    solve(q, n, q, n)
    return Dcur, Aq


# ---- depth by depth
def node(t, d, q, n):
    """Node t of depth d of solve(q, n, ., .) as the kernel finds it: (jl, jh), or None when the recursion never gets there."""
    jl, jh = q, n
    for b in range(d - 1, -1, -1):
        if jl > jh:
            return None
        mid = jl + ((jh - jl) >> 1)
        if (t >> b) & 1:
            jl = mid + 1
        else:
            jh = mid - 1
    return (jl, jh) if jl <= jh else None


def depths(q, n):
    return int(n - q + 1).bit_length()


def _layer_levels(Dprev, S1, S2, q, n, stats=None):
    Dcur = np.full(n + 1, np.nan)
    Aq = np.zeros(n + 1, np.int64)
    jl, jh = np.array([q], np.int64), np.array([n], np.int64)
    d = 0
    while jl.size:
        j = (jl + jh) // 2
        lo = np.where(jl > q, Aq[jl - 1], q)
        ih = np.where(jh < n, Aq[np.minimum(jh + 1, n)], n)
        hi = np.minimum(ih, j)
        lens = hi - lo + 1
        assert (lens >= 1).all()
        if stats is not None:
            stats.append((q, d, int(jl.size), int((lens >= WAVE_SCAN).sum()), int(lens.max())))
        first = np.cumsum(lens) - lens
        seg = np.repeat(np.arange(j.size), lens)
        i = lo[seg] + (np.arange(int(lens.sum())) - first[seg])
        v = Dprev[i - 1] + cost(S1, S2, i, j[seg])
        mn = np.minimum.reduceat(v, first)
        bi = np.minimum.reduceat(np.where(v == mn[seg], i, np.iinfo(np.int64).max), first)      # the first occurrence
        Dcur[j] = v[first + (bi - lo)]
        Aq[j] = bi
        left, right = jl <= j - 1, j + 1 <= jh
        jl, jh = np.concatenate([jl[left], j[right] + 1]), np.concatenate([j[left] - 1, jh[right]])
        d += 1
    assert d == depths(q, n)
    return Dcur, Aq


def _layer_brute(Dprev, S1, S2, q, n):
    Dcur = np.full(n + 1, np.nan)
    Aq = np.zeros(n + 1, np.int64)
    for j in range(q, n + 1):
        i = np.arange(q, j + 1)
        v = Dprev[i - 1] + cost(S1, S2, i, j)
        at = int(np.argmin(v))
        Dcur[j], Aq[j] = v[at], i[at]
    return Dcur, Aq


def _dp(layer, S1, S2, Kmax, **kw):
    S1, S2 = np.asarray(S1, np.float64), np.asarray(S2, np.float64)
    n = S1.size - 1
    assert S2.size == n + 1 and 1 <= Kmax <= n and np.isfinite(S1).all() and np.isfinite(S2).all()
    D = _first_row(n)
    sse = np.empty(Kmax)
    A = np.zeros((Kmax + 1, n + 1), np.int64)
    for q in range(1, Kmax + 1):
        D, A[q] = layer(D, S1, S2, q, n, **kw)
        sse[q - 1] = D[n]
    return sse, A


def dp_recursive(S1, S2, Kmax):
    """-> (sse f64 [Kmax]: sse[q-1] = D[q][n];  A int64 [Kmax + 1, n + 1]: A[q][j] for j >= q, 0 elsewhere)."""
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 10000))
    try:
        return _dp(_layer_recursive, S1, S2, Kmax)
    finally:
        sys.setrecursionlimit(limit)


def dp_levels(S1, S2, Kmax, stats=None):
    """dp_recursive depth by depth; `stats` (a list) gets (q, depth, nodes, nodes with >= WAVE_SCAN candidates, longest scan)."""
    return _dp(_layer_levels, S1, S2, Kmax, stats=stats)


def dp_brute(S1, S2, Kmax):
    return _dp(_layer_brute, S1, S2, Kmax)


# ---- the results
def walk(A, S1, S2, shift, k):
    """-> (starts int32 [k] counting from 1, code points f64 [k] ascending, counts int64 [k]) of the optimum with k levels."""
    n = S1.size - 1
    starts, codes, counts = np.zeros(k, np.int32), np.zeros(k), np.zeros(k, np.int64)
    j = n
    for q in range(k, 0, -1):
        i = int(A[q][j])
        assert q <= i <= j
        starts[q - 1] = i
        codes[q - 1] = shift + (S1[j] - S1[i - 1]) / np.float64(j - i + 1)
        counts[q - 1] = j - i + 1
        j = i - 1
    assert j == 0
    return starts, codes, counts


def fit(S1, S2, shift, levels, dp=dp_levels):
    """What vbqk_kmeans1d_f64 reports for one channel: ({k: (starts, codes, counts)}, sse [max(levels)])."""
    sse, A = dp(S1, S2, max(levels))
    return {k: walk(A, S1, S2, shift, k) for k in levels}, sse


def objective_bound(S2, n):
    """|objective - the real-number objective of the same segmentation| <= 4 n eps S2[n]; see tests/test_kmeans_host.py."""
    return 4.0 * n * EPS * float(S2[n])


# ---- the data families of the tests
def family(name, rng, n):
    """f32 [n], unsorted."""
    if name == "normal":
        x = rng.standard_normal(n)
    elif name == "quarters":
        x = np.round(4 * rng.standard_normal(n)) / 4
    elif name == "student":
        x = rng.standard_t(2, n) * 1.23 - 0.08
    elif name == "equal":
        x = np.full(n, 0.7)
    elif name == "shifted":
        x = rng.standard_normal(n) + 1000
    else:
        raise KeyError(name)
    return x.astype(np.float32)


FAMILIES = ("normal", "quarters", "student", "equal", "shifted")
