"""The budget sweep (include/vbq_budget.h, vbq_amd/budget/vbqb_sweep.hip) on the device: one forward pass of the budget DP at
the largest budget against one separate solve per budget -- the float64 restatement tests/budget_reference.py (one
budget_dp_rows call per budget) and the single-budget entry points that exist (ops.budget_dp, quantize_rows_to_budget,
compress_to_records).  Every comparison is np.array_equal on values or bit patterns; the one exception,
records_distortion_curve, says so where it stands."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import budget_reference as BR  # noqa: E402
import footprint as FP  # noqa: E402
import stream_order as SO  # noqa: E402

gpu = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


@pytest.fixture(scope="module")
def spin():
    _need_gpu()
    sp, notes = SO.calibrate()
    print(f"\n[test_gpu_budget_sweep] {sp}: {notes}")
    return sp


def _cuda(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()      # the shared tables are read-only


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _scores(rng, N, R, K):
    """The recipe of tests/test_gpu_budget_dp.py: 0 at some depth, falling off steeply above it."""
    err = np.abs(rng.standard_normal((1, R, K))) * 2.0 ** (-np.arange(N + 1))[:, None, None] * rng.uniform(0.5, 2, (N + 1, R, K))
    return -0.5 * (err / np.exp(-3 + rng.standard_normal((1, R, K)))) ** 2


@functools.lru_cache(maxsize=None)
def _reference(key, budget):
    """(bits, obj) of budget_dp_rows for the score table registered under `key`; computed once, read-only."""
    bits, obj = BR.budget_dp_rows(_TABLES[key], budget)
    bits.setflags(write=False)
    obj.setflags(write=False)
    return bits, obj


_TABLES = {}


def _table(key, make):
    if key not in _TABLES:
        t = make()
        t.setflags(write=False)
        _TABLES[key] = t
    return _TABLES[key]


def _sweep(fhat, budgets, curve_len=0, **kw):
    from vbq_amd import ops
    K = fhat.shape[2]
    bits, obj, curve = ops.budget_dp_sweep(_cuda(fhat), K, budgets, curve_len=curve_len, **kw)
    S, R = len(budgets), fhat.shape[1]
    assert bits.dtype == torch.int32 and tuple(bits.shape) == (S, R, K)
    assert obj.dtype == torch.float64 and tuple(obj.shape) == (S, R)
    assert (curve is None) == (curve_len == 0)
    if curve is not None:
        assert curve.dtype == torch.float64 and tuple(curve.shape) == (R, curve_len)
        curve = curve.cpu().numpy()
    return bits.cpu().numpy().astype(np.int64), obj.cpu().numpy(), curve


def _same(key, fhat, budgets, single=True, rows=None, **kw):
    """Slice s of the sweep equals budget_dp_rows at budgets[s] and, with `single`, ops.budget_dp at budgets[s]."""
    from vbq_amd import ops
    bits, obj, curve = _sweep(fhat, budgets, **kw)
    rows = slice(None) if rows is None else rows
    dev = _cuda(fhat) if single else None
    for s, b in enumerate(budgets):
        want_bits, want_obj = _reference(key, b)
        assert np.array_equal(bits[s][rows], want_bits[rows]), (key, b)
        assert np.array_equal(_u64(obj[s][rows]), _u64(want_obj[rows])), (key, b)
        if single:
            one_bits, one_obj = ops.budget_dp(dev, fhat.shape[2], b)
            assert np.array_equal(bits[s], one_bits.cpu().numpy()) and np.array_equal(_u64(obj[s]), _u64(one_obj.cpu().numpy())), (key, b)
    return bits, obj, curve


def _budget_lists(K, N):
    KN = K * N
    mid = KN // 2
    lists = [[0], [KN], [0, KN], sorted({max(0, mid - 1), mid, min(KN, mid + 1)})]
    return [b for i, b in enumerate(lists) if b not in lists[:i]]


# ------------------------------------------------------------------------------------------------------------------ the kernel
@gpu
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("N", [1, 4, 10])
@pytest.mark.parametrize("K", [1, 2, 7, 100])
def test_sweep_equals_one_solve_per_budget(K, N, R):
    _need_gpu()
    key = ("random", K, N, R)
    fhat = _table(key, lambda: _scores(np.random.default_rng(1000 * K + 10 * N + R), N, R, K))
    for budgets in _budget_lists(K, N):
        _same(key, fhat, budgets)


@gpu
@pytest.mark.parametrize("width", [64, 65, 128, 129, 256, 257, 301])
def test_every_thread_plan_and_the_loop_over_n(width):
    """width = largest budget + 1: 64 lanes (<= 64), 128 lanes (<= 128), 256 lanes, and lanes that loop over n (> 256)."""
    _need_gpu()
    K, N, R = 40, 10, 3
    key = ("plans", K, N, R)
    fhat = _table(key, lambda: _scores(np.random.default_rng(41), N, R, K))
    _same(key, fhat, [0, 1, width // 3, width - 2, width - 1])


@gpu
def test_sixty_four_budgets_and_one():
    _need_gpu()
    K, N, R = 20, 10, 5
    key = ("many", K, N, R)
    fhat = _table(key, lambda: _scores(np.random.default_rng(64), N, R, K))
    _same(key, fhat, list(range(0, 192, 3)))                         # S = 64, every lane of the first wave walks
    _same(key, fhat, [137])                                          # S = 1
    from vbq_amd import VBQError
    with pytest.raises(VBQError, match="S=65"):
        _sweep(fhat, list(range(65)))


# ------------------------------------------------------------------------------------------------------------------ the curve
@gpu
@pytest.mark.parametrize("K,N", [(5, 3), (7, 4), (20, 10)])
def test_curve_is_the_objective_of_a_separate_solve_at_every_budget(K, N):
    _need_gpu()
    R, KN = 4, K * N
    key = ("curve", K, N, R)
    fhat = _table(key, lambda: _scores(np.random.default_rng(7 * K + N), N, R, K))
    want = np.stack([_reference(key, n)[1] for n in range(KN + 1)], axis=1)              # [R, KN + 1]
    _, _, only = _sweep(fhat, [], curve_len=KN + 1)                                       # curve-only
    assert np.array_equal(_u64(only), _u64(want))
    budgets = [1, KN // 2, KN]
    _, _, both = _same(key, fhat, budgets, curve_len=KN + 1)                              # a curve together with budgets
    assert np.array_equal(_u64(both), _u64(want))
    short = KN // 3 + 1
    _, _, cut = _same(key, fhat, budgets, curve_len=short)                                # curve_len < budgets[-1] + 1
    assert np.array_equal(_u64(cut), _u64(want[:, :short]))
    _, _, wide = _same(key, fhat, [2], curve_len=KN)                                      # curve_len > budgets[-1] + 1
    assert np.array_equal(_u64(wide), _u64(want[:, :KN]))


# ------------------------------------------------------------------------------------------------------------------ the workspace
@gpu
def test_workspace_path_with_one_slice_and_several_rounds():
    _need_gpu()
    from vbq_amd import VBQError, _lib_budget
    K, N, top, R = 300, 4, 600, 5
    per_row = (K * (top + 1) + 15) // 16 * 16
    assert per_row > 160 * 1024                                                           # the back-pointers do not fit the LDS
    assert _lib_budget.lib().vbqb_budget_sweep_workspace_bytes(R, K, N, top + 1) == R * per_row
    key = ("workspace", K, N, R)
    fhat = _table(key, lambda: _scores(np.random.default_rng(5), N, R, K))
    budgets = [0, 299, 300, 600]
    _same(key, fhat, budgets, single=False, workspace=torch.empty(per_row, dtype=torch.uint8, device="cuda"))   # 5 rounds
    _, _, curve = _same(key, fhat, budgets, single=False, curve_len=3)                    # the call's own workspace
    assert np.array_equal(_u64(curve), _u64(np.stack([_reference(key, n)[1] for n in range(3)], axis=1)))
    with pytest.raises(VBQError, match="workspace"):
        _sweep(fhat, budgets, workspace=torch.empty(per_row - 1, dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------------------------------------------------------ ties, -inf
@gpu
@pytest.mark.parametrize("K,N", [(2, 3), (7, 4), (20, 10), (100, 10)])
def test_ties_take_the_first_maximum(K, N):
    """Scores drawn from {0, -1, -2}: sums are exact and equal sums are the rule."""
    _need_gpu()
    key = ("ties", K, N)

    def make():
        fhat = -np.random.default_rng(77 * K + N).integers(0, 3, (N + 1, 4, K)).astype(np.float64)
        fhat[:, 3, :] = 0.0                                                               # a row where EVERYTHING ties
        return fhat
    fhat = _table(key, make)
    KN = K * N
    _same(key, fhat, sorted({0, 1, N, KN // 3, KN // 2, KN}))


@gpu
@pytest.mark.parametrize("K,N", [(1, 4), (2, 4), (7, 10), (100, 10)])
def test_minus_inf_entries(K, N):
    _need_gpu()
    key = ("ninf", K, N)

    def make():
        rng = np.random.default_rng(31 * K + N)
        fhat = _scores(rng, N, 5, K)
        fhat[rng.uniform(size=fhat.shape) < 0.3] = -np.inf
        fhat[:, 3, :] = -np.inf                                  # no finite allocation at all: objective -inf
        fhat[1:, 4, :] = -np.inf                                 # only "0 bits everywhere" is finite
        return fhat
    fhat = _table(key, make)
    KN = K * N
    budgets = sorted({0, 1, N, KN // 3, KN})
    _, obj, curve = _same(key, fhat, budgets, curve_len=KN + 1)
    assert (obj[:, 3] == -np.inf).all()
    assert np.array_equal(_u64(curve[:, budgets]), _u64(obj.T))


# ------------------------------------------------------------------------------------------------------------------ status
@gpu
def test_nan_row_sets_status_and_leaves_the_other_rows_exact():
    _need_gpu()
    K, N = 40, 10
    key = ("status", K, N)
    clean = _table(key, lambda: _scores(np.random.default_rng(9), N, 6, K))
    fhat = clean.copy()
    fhat[3, 2, 17] = np.nan
    fhat[0, 4, 0] = np.inf
    budgets = [0, 130, 131, 400]
    ok = [0, 1, 3, 5]
    status = torch.zeros(1, dtype=torch.uint32, device="cuda")
    bits, _, curve = _same(key, fhat, budgets, single=False, rows=ok, curve_len=K * N + 1, status=status)
    assert int(status.cpu().item()) == 1
    assert bits.min() >= 0 and bits.max() <= N
    want = np.stack([_reference(key, n)[1] for n in (0, 130, 400)], axis=1)
    assert np.array_equal(_u64(curve[ok][:, [0, 130, 400]]), _u64(want[ok]))
    status.zero_()
    _same(key, clean, budgets, single=False, status=status)
    assert int(status.cpu().item()) == 0
    _sweep(fhat, [], curve_len=5, status=status)                                          # the curve-only pass reports it too
    assert int(status.cpu().item()) == 1
    status.zero_()
    bits, _, _ = _sweep(np.full_like(clean, np.nan), [0, K * N], status=status)           # a remainder far above N
    assert int(status.cpu().item()) == 1 and bits.min() >= 0 and bits.max() <= N


# ------------------------------------------------------------------------------------------------------------------ footprint
@gpu
@pytest.mark.parametrize("offset", [0, 1])
def test_write_footprint(offset):
    """out_bits, out_obj, the curve and an exactly sized workspace between canaries, aligned and one element off."""
    _need_gpu()
    from vbq_amd import _lib_budget, ops
    h = _lib_budget.lib()
    for K, N, R, budgets, curve_len in ((7, 4, 5, [0, 9, 28], 20), (300, 4, 3, [17, 600], 5)):
        key = ("footprint", K, N, R)
        fhat = _table(key, lambda: _scores(np.random.default_rng(K), N, R, K))
        S, width = len(budgets), max(budgets[-1] + 1, curve_len)
        d_fhat = FP.shifted(fhat, offset, "cuda")
        wsb = h.vbqb_budget_sweep_workspace_bytes(R, K, N, width)
        assert (wsb > 0) == (K == 300)
        g_bits = FP.Guarded((S, R, K), torch.int32, "cuda", offset)
        g_obj = FP.Guarded((S, R), torch.float64, "cuda", offset)
        g_curve = FP.Guarded((R, curve_len), torch.float64, "cuda", offset)
        g_ws = FP.guarded_workspace(wsb, "cuda") if wsb else None
        arr = (ops.C.c_int32 * S)(*budgets)
        rc = h.vbqb_budget_sweep_f64(ops._ptr(d_fhat), R, K, N, arr, S, g_bits.ptr, g_obj.ptr, g_curve.ptr, curve_len, None,
                                     g_ws.ptr if g_ws else None, wsb, ops._stream(d_fhat))
        assert rc == 0, h.vbqb_last_error()
        torch.cuda.synchronize()
        for g, what in ((g_bits, "out_bits"), (g_obj, "out_obj"), (g_curve, "curve")) + (((g_ws, "workspace"),) if g_ws else ()):
            g.assert_outside_intact(what)
        for g in (g_bits, g_obj, g_curve):
            assert (g.bits() != FP.canary(g.dtype)).all(), "an output element was not written"
        for s, b in enumerate(budgets):
            want_bits, want_obj = _reference(key, b)
            assert np.array_equal(g_bits.host()[s], want_bits) and np.array_equal(_u64(g_obj.host()[s]), _u64(want_obj))
        # the curve-only pass writes the curve alone; a refused call writes nothing
        g_only = FP.Guarded((R, curve_len), torch.float64, "cuda", offset)
        assert h.vbqb_budget_sweep_f64(ops._ptr(d_fhat), R, K, N, None, 0, None, None, g_only.ptr, curve_len, None, None, 0,
                                       ops._stream(d_fhat)) == 0
        torch.cuda.synchronize()
        g_only.assert_outside_intact("curve-only")
        assert np.array_equal(g_only.bits(), g_curve.bits())
        fresh = [FP.Guarded((S, R, K), torch.int32, "cuda", offset), FP.Guarded((S, R), torch.float64, "cuda", offset),
                 FP.Guarded((R, curve_len), torch.float64, "cuda", offset)]
        bad = (ops.C.c_int32 * S)(*([budgets[-1]] + budgets[1:]))
        rc = h.vbqb_budget_sweep_f64(ops._ptr(d_fhat), R, K, N, bad, S, fresh[0].ptr, fresh[1].ptr, fresh[2].ptr, curve_len, None,
                                     g_ws.ptr if g_ws else None, wsb, ops._stream(d_fhat))
        assert rc == -1 and b"strictly ascending" in h.vbqb_last_error()
        torch.cuda.synchronize()
        for g in fresh:
            g.assert_untouched("refused sweep")


# ------------------------------------------------------------------------------------------------------------------ public calls
def _latents(rng, R, K, per_column, N):
    import vbq_amd
    scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), K)) if per_column else np.array([1.0])
    tab = vbq_amd.gaussian_table(scale, N=N)                                              # [K, T] / [1, T]
    mu = (scale * rng.standard_normal((R, K))).astype(np.float32)
    mu[0, :] = 50.0                                                                       # beyond every table's end
    sg = np.clip(np.exp(-2 + 0.7 * rng.standard_normal((R, K))), 1e-4, 10).astype(np.float32)
    return mu, sg, (tab if per_column else tab[0])


def _mixed_budgets(K, N):
    KN = K * N
    return [KN // 2, 0, KN, KN // 2, min(KN, 3), KN // 3, 0]                              # out of order, with repeats


@gpu
@pytest.mark.parametrize("per_column", [False, True])
@pytest.mark.parametrize("R,K,N", [(9, 1, 4), (40, 7, 10), (12, 100, 10)])
def test_quantize_rows_to_budgets_equals_the_loop(R, K, N, per_column):
    _need_gpu()
    import vbq_amd
    mu, sg, tab = _latents(np.random.default_rng(R * K + N), R, K, per_column, N)
    budgets = _mixed_budgets(K, N)
    idx, num_bits, objective = vbq_amd.quantize_rows_to_budgets(mu, sg, budgets, table=tab, N=N)
    assert idx.is_cuda and idx.dtype == torch.uint16 and tuple(idx.shape) == (len(budgets), R, K)
    assert num_bits.dtype == torch.int32 and objective.dtype == torch.float64
    for s, b in enumerate(budgets):
        i1, n1, o1 = vbq_amd.quantize_rows_to_budget(mu, sg, b, table=tab, N=N)
        assert np.array_equal(idx[s].cpu().numpy(), i1.cpu().numpy()), b
        assert np.array_equal(num_bits[s].cpu().numpy(), n1.cpu().numpy()), b
        assert np.array_equal(_u64(objective[s].cpu().numpy()), _u64(o1.cpu().numpy())), b
    curve = vbq_amd.rows_budget.budget_curve(mu, sg, table=tab, N=N)
    assert tuple(curve.shape) == (R, K * N + 1) and curve.dtype == torch.float64
    assert np.array_equal(_u64(curve.cpu().numpy()[:, budgets]), _u64(objective.cpu().numpy().T))
    short = vbq_amd.rows_budget.budget_curve(mu, sg, table=tab, N=N, max_bits=K * N // 3)
    assert np.array_equal(_u64(short.cpu().numpy()), _u64(curve.cpu().numpy()[:, :K * N // 3 + 1]))
    with pytest.raises(ValueError, match="outside"):
        vbq_amd.quantize_rows_to_budgets(mu, sg, [0, K * N + 1], table=tab, N=N)
    with pytest.raises(vbq_amd.VBQError, match="NaN"):
        vbq_amd.quantize_rows_to_budgets(mu, np.full_like(sg, np.nan), [1], table=tab, N=N)


@gpu
def test_more_than_64_distinct_budgets_take_several_launches():
    _need_gpu()
    import vbq_amd
    R, K, N = 3, 20, 4
    mu, sg, tab = _latents(np.random.default_rng(2), R, K, False, N)
    budgets = list(range(K * N, -1, -1))                                                  # 81 distinct values, descending
    _, num_bits, objective = vbq_amd.quantize_rows_to_budgets(mu, sg, budgets, table=tab, N=N)
    assert np.array_equal(num_bits.cpu().numpy().sum(axis=2), np.repeat(np.array(budgets)[:, None], R, axis=1))
    curve = vbq_amd.rows_budget.budget_curve(mu, sg, table=tab, N=N)
    assert np.array_equal(_u64(curve.cpu().numpy()[:, budgets]), _u64(objective.cpu().numpy().T))


def _embedding_case(seed, R, K, N, per_column=False):
    mu, sg, tab = _latents(np.random.default_rng(seed), R, K, per_column, N)
    mu[0] = mu[-1] * 0.5                                                                  # keep every row inside the tables
    return mu, sg, tab


def _numpy_distortion(mu, sg, tab, N):
    """D(b) from the float64 restatement: the candidates' scores through budget_dp_rows at every b."""
    from vbq_amd import rows_budget
    tab2 = np.asarray(tab).reshape(-1, tab.shape[-1])
    scores, _ = rows_budget.level_candidates(_cuda(mu), _cuda(sg), _cuda(tab2), N)
    scores = scores.cpu().numpy()
    R, K = mu.shape
    return np.array([-2.0 * BR.budget_dp_rows(scores, b)[1].sum() / (R * K) for b in range(K * N + 1)])


@gpu
@pytest.mark.parametrize("per_column", [False, True])
def test_compress_to_records_sweep_equals_the_loop(per_column):
    _need_gpu()
    from vbq_amd import embeddings as E
    R, K, N = 40, 7, 10
    mu, sg, tab = _embedding_case(11, R, K, N, per_column)
    budgets = _mixed_budgets(K, N)
    files = E.compress_to_records_sweep(mu, sg, budgets, tab, N)
    assert len(files) == len(budgets)
    for b, data in zip(budgets, files):
        assert isinstance(data, bytes) and data == E.compress_to_records(mu, sg, b, tab, N), b
        rec = E.RecordEmbeddings(data)
        assert rec.total_bits == b and tuple(rec.shape) == (R, K)
    assert E.compress_to_records_sweep(mu, sg, [], tab, N) == []
    with pytest.raises(ValueError):
        E.compress_to_records_sweep(mu, sg, [3, K * N + 1], tab, N)


@gpu
def test_records_distortion_curve_and_the_quality_target(monkeypatch):
    _need_gpu()
    from vbq_amd import embeddings as E, rows_budget
    R, K, N = 7, 6, 4
    mu, sg, tab = _embedding_case(13, R, K, N)
    want = _numpy_distortion(mu, sg, tab, N)
    got = E.records_distortion_curve(mu, sg, tab, N)
    assert got.dtype == np.float64 and got.shape == (K * N + 1,)
    # The one comparison that is not bit-exact: a float64 sum of R = 7 terms of one sign, in an order the device chooses,
    # is within (R - 1) * 2^-53 < 1e-15 relative of any other order; 1e-12 leaves several orders of magnitude.
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all()
    # chunks of rows: 3 rows to a chunk gives chunks of 3, 3 and 1 rows
    monkeypatch.setattr(rows_budget, "CURVE_SCRATCH_BYTES", 3 * 8 * (K * N + 1))
    chunked = E.records_distortion_curve(mu, sg, tab, N)
    assert (np.abs(chunked - want) <= 1e-12 * np.abs(want)).all()
    monkeypatch.undo()
    # targets midway between neighbouring values of the reference curve
    for b in (0, 5, 11, K * N - 1):
        lo, hi = sorted((want[b], want[b + 1]))
        assert hi - lo > 1e-9 * hi, (b, lo, hi)
        target = 0.5 * (lo + hi)
        b_want = int(np.flatnonzero(want <= target)[0])
        assert E.compress_to_records_quality(mu, sg, tab, target, N) == E.compress_to_records(mu, sg, b_want, tab, N), b
    with pytest.raises(ValueError, match=f"total_bits = {int(np.argmin(want))}"):
        E.compress_to_records_quality(mu, sg, tab, 0.5 * want.min(), N)


@gpu
def test_quality_target_on_a_curve_that_is_not_monotone():
    """K = 1 and mu at the root code point: 0 bits are exact, one bit must move to a level-1 point, deeper levels come back
    towards it.  D(0) = 0 < D(N) < D(1): the smallest qualifying b lies below a non-qualifying one."""
    _need_gpu()
    import vbq_amd
    from vbq_amd import embeddings as E
    N = 4
    tab = vbq_amd.gaussian_table(np.array([1.0]), N=N)[0]
    mu = np.full((3, 1), tab[0], np.float32)
    sg = np.full((3, 1), 0.5, np.float32)
    want = _numpy_distortion(mu, sg, tab, N)
    assert want[0] == 0.0 and want[1] > want[N] > 0.0
    got = E.records_distortion_curve(mu, sg, tab, N)
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all()
    target = 0.5 * (want[1] + want[N])                                                    # b = 0 and b = N qualify, b = 1 does not
    assert E.compress_to_records_quality(mu, sg, tab, target, N) == E.compress_to_records(mu, sg, 0, tab, N)
    rec = E.RecordEmbeddings(E.compress_to_records_quality(mu, sg, tab, target, N))
    assert rec.total_bits == 0


@gpu
def test_total_bits_sweep_equals_the_composition_of_existing_calls():
    _need_gpu()
    from vbq_amd import bitstream as bs, embeddings as E
    R, K, N = 40, 7, 10
    mu, sg, tab = _embedding_case(17, R, K, N)
    rng = np.random.default_rng(3)
    analogies = rng.integers(0, R, (25, 4))
    budgets = [30, 5, 70, 30]
    got = E.test_total_bits(mu, sg, budgets, tab, analogies)
    assert got.dtype == np.float64 and got.shape == (len(budgets), 4)
    for s, b in enumerate(budgets):
        data = E.compress_to_records(mu, sg, b, tab, N)
        emb = E.decompress(data)
        want = E.analogy_metrics(E.prediction_ranks(emb, analogies)) + (8.0 * bs.records_nbytes((R, K), N, b, 1) / (R * K),)
        assert len(data) == bs.records_nbytes((R, K), N, b, 1)
        assert np.array_equal(_u64(got[s]), _u64(np.array(want, np.float64))), b


# ------------------------------------------------------------------------------------------------------------------ stream order
def _late_rows(seed, R=9, K=5):
    rng = np.random.default_rng(seed)
    return [_cuda(rng.normal(0, 1, (R, K)).astype(np.float32)), _cuda(rng.uniform(0.05, 1.0, (R, K)).astype(np.float32))]


@gpu
@pytest.mark.parametrize("name", ["quantize_rows_to_budgets", "budget_curve"])
def test_the_python_calls_are_ordered_on_the_callers_stream(name, spin):
    """Late mu and sigma on a side stream, the exact answer.  Blocking: both calls read one status word after their last
    launch, and every launch is enqueued while the delay runs."""
    _need_gpu()
    import vbq_amd
    N = 4
    book = vbq_amd.gaussian_table(np.array([1.0]), N=N)[0]
    call = {"quantize_rows_to_budgets": lambda b: vbq_amd.quantize_rows_to_budgets(b[0], b[1], [11, 0, 20, 3], table=book, N=N),
            "budget_curve": lambda b: vbq_amd.rows_budget.budget_curve(b[0], b[1], table=book, N=N)}[name]
    SO.run_late(call, _late_rows(7), _late_rows(SO.STALE_SEED), blocking=True, spin=spin, name=name)


@gpu
def test_the_c_call_is_ordered_on_the_callers_stream_and_does_not_synchronize(spin):
    """Armed: the scores arrive late on a side stream, and the call returns while the delay is still running."""
    _need_gpu()
    from vbq_amd import ops
    K, N = 20, 4

    def late(seed):
        return [_cuda(_scores(np.random.default_rng(seed), N, 6, K))]
    got = SO.run_late(lambda b: ops.budget_dp_sweep(b[0], K, [0, 33, 80], curve_len=K * N + 1), late(7), late(SO.STALE_SEED),
                      blocking=False, spin=spin, name="ops.budget_dp_sweep")
    assert got.armed
