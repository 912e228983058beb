"""K2's lane-private counters for the shallow bit levels (hist_add8_hot / hist_fold_hot, vbq_hist.hip), against NumPy.

For N <= 10 `k_hist_flat` counts the ranks of bit levels 0 .. LH (rank q with q + 1 a multiple of 2^(N - LH)) in LDS words of
their own, one per lane, and folds them into the bins before the flush; every other index -- foreign values up to 65535
included -- takes the bin it always took.  Counts are integers and models are table lookups of them: every comparison is
exact equality.  The grids are those of test_gpu_hist_stream.py:
  * L = 2, C = 1024: one workgroup per row; the plain histogram (assign 0) and the fused histogram_models (assign 2), with and
    without the model lookup.
  * L = 2, C = 3: the plain histogram with several workgroups on a row.
Row lengths are the smallest that reach each path of the kernel; the contents put all, none or some of the indices on the hot
words.  The rows of a case come from a pool of 37 different rows (37 and 1024 are coprime: neighbouring rows, channels and
lambdas all differ), so the reference is 37 bincounts per case.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu]
N = 10
T = 2047
LH = 3                              # the cut-off level the library is built with (VBQ_HIST_HOT)
STEP = 1 << (N - LH)                # hot ranks: STEP * k - 1, k = 1 .. 2^(LH+1) - 1
HOT = STEP * np.arange(1, 2 << LH) - 1
POOL = 37

LENGTHS = {
    "no_octet": 7,
    "one_octet": 8,
    "partial_wave": 4096 - 8,
    "odd_no_stage": 3 * 512 * 8 - 3,            # heads on every other row, a tail of 5, no whole register stage
    "pair_plus_one": 2 * 12288 + 8,             # a pipelined pair of stages plus one more load
    "kodak_row": 36864,
}
CONTENTS = ["hot_only", "neighbours", "one_hot", "mix", "any_u16"]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    from vbq_amd import ops as _ops
    return _ops


def mix_rows(rng, rows, n):
    """Bench-like: levels drawn with weights 2^(-level/2), positions uniform within the level."""
    w = 2.0 ** (-np.arange(N + 1) / 2)
    lev = rng.choice(N + 1, size=(rows, n), p=w / w.sum())
    pos = (rng.random((rows, n)) * (1 << lev)).astype(np.int64)
    return (((2 * pos + 1) << (N - lev)) - 1).astype(np.uint16)


def make_pool(content, n, seed):
    rng = np.random.default_rng(seed)
    if content == "hot_only":
        return HOT[rng.integers(0, len(HOT), (POOL, n))].astype(np.uint16)
    if content == "neighbours":                                 # next to every hot rank, never on one; the ends of the table
        pick = np.concatenate([HOT - 1, HOT + 1, [0, 2046]])
        pick = pick[(pick >= 0) & (pick < T)]
        assert not np.isin(pick, HOT).any()
        return pick[rng.integers(0, len(pick), (POOL, n))].astype(np.uint16)
    if content == "one_hot":
        # even rows: one hot rank fills the row (every lane word of one rank); odd rows: one hot index among cold ones
        cold = np.setdiff1d(np.arange(T), HOT)
        pool = cold[rng.integers(0, len(cold), (POOL, n))].astype(np.uint16)
        pool[0::2] = HOT[rng.integers(0, len(HOT), ((POOL + 1) // 2, 1))]
        odd = np.arange(1, POOL, 2)
        pool[odd, rng.integers(0, n, len(odd))] = HOT[rng.integers(0, len(HOT), len(odd))]
        return pool
    pool = mix_rows(rng, POOL, n)
    if content == "any_u16":                                    # 1 % of the entries are not ranks at all
        foreign = rng.random((POOL, n)) < 0.01
        pool[foreign] = rng.integers(2047, 65536, int(foreign.sum()), dtype=np.int64).astype(np.uint16)
        pool[:, 0] = 65535                                      # m = 65536: every low bit clear, and not hot
        pool[:, n - 1] = 4095                                   # m = 4096
        pool[:, n // 2] = 2047                                  # the first value past the table
    else:
        assert content == "mix"
    return pool


def pool_counts(pool):
    """What the bins hold for ANY u16 input: index q lands in the bin i with slot(i) == slot(q) & 2047, slot(x) = x ^ (x >> 6)
    (for q < 2047 that is bin q: np.bincount)."""
    q = pool.astype(np.int64)
    slot = (q ^ (q >> 6)) & 2047
    i = np.arange(T)
    return np.stack([np.bincount(s, minlength=2048)[i ^ (i >> 6)] for s in slot])


def make_case(L, C, key, content):
    n = LENGTHS[key]
    pool = make_pool(content, n, seed=1000 * CONTENTS.index(content) + n % 997 + C)
    cnt = pool_counts(pool)
    if content != "any_u16":
        assert np.array_equal(cnt, np.stack([np.bincount(r, minlength=T) for r in pool]))
    pick = (np.arange(L * C) * 5 + 3) % POOL
    idx_h = np.ascontiguousarray(pool[pick].reshape(L, C, n))
    want = cnt[pick].reshape(L, C, T)
    assert int(want.sum()) <= L * C * n and (content == "any_u16" or int(want.sum()) == L * C * n)
    return idx_h, want


def check_all_modes(ops, L, C, key, content, fused):
    idx_h, want = make_case(L, C, key, content)
    n = idx_h.shape[2]
    idx = torch.from_numpy(idx_h).cuda()
    for dtype in (torch.int64, torch.int32):
        got = ops.histogram(idx, C, N=N, layout="cb", out=torch.zeros((L, C, T), dtype=dtype, device="cuda"))
        assert np.array_equal(got.cpu().numpy(), want), ("histogram", dtype, key, content)
    if not fused:
        return
    lut = torch.rand(n + 1, device="cuda")
    for dtype in (torch.int64, torch.int32):
        want_t = torch.from_numpy(want).to(dtype).cuda()
        want_m = ops.code_lengths_from_counts(want_t, lut, want_len=False, want_model=True)
        cnt = torch.full((L, C, T), -5, dtype=dtype, device="cuda")                  # assigned, not added
        ops.histogram_models(idx, C, cnt, N=N)
        assert torch.equal(cnt, want_t), ("histogram_models", dtype, key, content)
        cnt = torch.full((L, C, T), -5, dtype=dtype, device="cuda")
        mdl = torch.full((L, C, T), -1.0, dtype=torch.float32, device="cuda")
        ops.histogram_models(idx, C, cnt, N=N, lut=lut, models=mdl)
        assert torch.equal(cnt, want_t), ("histogram_models + lut", dtype, key, content)
        assert torch.equal(mdl, want_m), ("models", dtype, key, content)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("key", list(LENGTHS))
def test_one_workgroup_per_row(ops, key, content):
    """L C = 2048: the plain histogram (assign 0) and the fused form (assign 2, with and without models), both counter widths."""
    check_all_modes(ops, 2, 1024, key, content, fused=True)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("key", list(LENGTHS))
def test_several_workgroups_per_row(ops, key, content):
    """L = 2, C = 3: the plain histogram with its workgroups side by side on a row, both counter widths."""
    check_all_modes(ops, 2, 3, key, content, fused=False)


def test_depth_11_unchanged(ops):
    """N = 11 has two copies of its 4095 bins and no hot words: ranks that WOULD be hot at this depth, their neighbours and
    uniform ones, one workgroup per row with heads and a tail, both entry points and counter widths."""
    n11, t11, L, C = 11, 4095, 2, 1024
    n = LENGTHS["odd_no_stage"]
    rng = np.random.default_rng(11)
    hot11 = (1 << (n11 - LH)) * np.arange(1, 2 << LH) - 1
    pool = rng.integers(0, t11, (POOL, n))
    shallow = rng.random((POOL, n)) < 0.6
    pool[shallow] = hot11[rng.integers(0, len(hot11), int(shallow.sum()))]
    pool = pool.astype(np.uint16)
    cnt = np.stack([np.bincount(r, minlength=t11) for r in pool])
    pick = (np.arange(L * C) * 5 + 3) % POOL
    idx = torch.from_numpy(np.ascontiguousarray(pool[pick].reshape(L, C, n))).cuda()
    want = cnt[pick].reshape(L, C, t11)
    for dtype in (torch.int64, torch.int32):
        got = ops.histogram(idx, C, N=n11, layout="cb", out=torch.zeros((L, C, t11), dtype=dtype, device="cuda"))
        assert np.array_equal(got.cpu().numpy(), want), ("histogram", dtype)
        got = torch.full((L, C, t11), -5, dtype=dtype, device="cuda")
        ops.histogram_models(idx, C, got, N=n11)
        assert np.array_equal(got.cpu().numpy(), want), ("histogram_models", dtype)


@pytest.mark.parametrize("depth", [4, 7])
def test_shallower_depths(ops, depth):
    """N < 10 has the hot words too, with a smaller shift (N = 4: every other rank is hot): uniform ranks, 60 % of them moved
    onto hot ones, one workgroup per row with heads and a tail, both entry points and counter widths."""
    t, L, C = (2 << depth) - 1, 2, 1024
    n = LENGTHS["odd_no_stage"]
    rng = np.random.default_rng(depth)
    hot = (1 << (depth - LH)) * np.arange(1, 2 << LH) - 1
    pool = rng.integers(0, t, (POOL, n))
    shallow = rng.random((POOL, n)) < 0.6
    pool[shallow] = hot[rng.integers(0, len(hot), int(shallow.sum()))]
    pool = pool.astype(np.uint16)
    cnt = np.stack([np.bincount(r, minlength=t) for r in pool])
    pick = (np.arange(L * C) * 5 + 3) % POOL
    idx = torch.from_numpy(np.ascontiguousarray(pool[pick].reshape(L, C, n))).cuda()
    want = cnt[pick].reshape(L, C, t)
    for dtype in (torch.int64, torch.int32):
        got = ops.histogram(idx, C, N=depth, layout="cb", out=torch.zeros((L, C, t), dtype=dtype, device="cuda"))
        assert np.array_equal(got.cpu().numpy(), want), ("histogram", dtype)
        got = torch.full((L, C, t), -5, dtype=dtype, device="cuda")
        ops.histogram_models(idx, C, got, N=depth)
        assert np.array_equal(got.cpu().numpy(), want), ("histogram_models", dtype)
