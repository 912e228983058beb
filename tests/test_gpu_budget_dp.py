"""The budget DP kernel and the patience scan (vbq_budget.hip) against the float64 restatement of tests/budget_reference.py,
and the surfaces built on them (vbq_amd.utils.encode_mode_dp / encode_mode, vbq_amd.quantize_rows_to_budget).  Every comparison
is exact equality, or the stated inequality: the restatement equals the reference bit for bit (tests/test_budget_dp_host.py)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import budget_reference as BR  # noqa: E402

gpu = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


@pytest.fixture(scope="module")
def g14(golden):
    return golden("g14_budget_dp.npz")


def _dp(fhat, budget, **kw):
    """fhat f64 [N+1, R, K] (NumPy) through the kernel -> (bits int64 [R, K], obj f64 [R]) on the host."""
    from vbq_amd import ops
    K = fhat.shape[2]
    bits, obj = ops.budget_dp(torch.from_numpy(np.ascontiguousarray(fhat)).cuda(), K, budget, **kw)
    assert bits.dtype == torch.int32 and obj.dtype == torch.float64
    return bits.cpu().numpy().astype(np.int64), obj.cpu().numpy()


def _same(fhat, budget, **kw):
    bits, obj = _dp(fhat, budget, **kw)
    want_bits, want_obj = BR.budget_dp_rows(fhat, budget)
    assert np.array_equal(bits, want_bits), (fhat.shape, budget)
    assert obj.tobytes() == want_obj.tobytes(), (fhat.shape, budget)
    assert np.array_equal(bits.sum(axis=1), np.full(fhat.shape[1], budget))


def _scores(rng, N, R, K):
    """Scores shaped like the real ones: 0 at some depth, falling off steeply above it (-0.5 * (error / sigma)**2)."""
    err = np.abs(rng.standard_normal((1, R, K))) * 2.0 ** (-np.arange(N + 1))[:, None, None] * rng.uniform(0.5, 2, (N + 1, R, K))
    return -0.5 * (err / np.exp(-3 + rng.standard_normal((1, R, K)))) ** 2


@gpu
def test_kernel_equals_restatement_and_reference_on_g14(g14):
    _need_gpu()
    from vbq_amd import ops
    for c in BR.g14_cases(g14):
        K, N = c["K"], c["N"]
        bits, obj = _dp(c["scores"][:, None, :], N)
        assert np.array_equal(bits[0], c["dp_num_bits"]) and obj[0].tobytes() == c["dp_obj"].tobytes(), (K, N)
        for budget in sorted({0, 1, N, K * N, K * N // 3}):
            _same(c["scores"][:, None, :], budget)
        for i, lamb in enumerate(g14["em_lambdas"]):
            b, g = ops.budget_patience(torch.from_numpy(c["em_scores"]).cuda(), float(lamb), 3)
            want_b, want_g = BR.patience_scan(c["em_scores"], float(lamb), 3)
            assert np.array_equal(b.cpu().numpy(), want_b) and g.cpu().numpy().tobytes() == want_g.tobytes(), (K, lamb)
            assert np.array_equal(b.cpu().numpy(), c["em_num_bits"][i]), (K, lamb)
            assert np.add.accumulate(g.cpu().numpy())[-1] == c["em_obj"][i], (K, lamb)


@gpu
@pytest.mark.parametrize("N", [1, 4, 10, 16])
@pytest.mark.parametrize("K", [1, 2, 7, 100, 300])
def test_random_rows_equal_restatement(K, N):
    """budget + 1 runs from 1 to 4801: below one wave, beyond 64, beyond 256 (lanes loop over n), back-pointers in LDS below and
    above 64 KiB, and in the workspace."""
    _need_gpu()
    rng = np.random.default_rng(1000 * K + N)
    fhat = _scores(rng, N, 3, K)
    for budget in sorted({0, 1, N, K * N, K * N // 3}):
        _same(fhat, budget)


@gpu
def test_workspace_path_and_several_rounds_of_workgroups():
    _need_gpu()
    from vbq_amd import _lib
    K, N, budget, R = 300, 16, 1600, 7
    per_row = (K * (budget + 1) + 15) // 16 * 16
    assert _lib.lib().vbq_budget_dp_workspace_bytes(R, K, N, budget) == R * per_row          # not in LDS: the workspace path
    fhat = _scores(np.random.default_rng(5), N, R, K)
    _same(fhat, budget)                                                                       # one workgroup per row
    for slices in (1, 2, 3):                                                                  # 7, 4 and 3 rounds over the rows
        _same(fhat, budget, workspace=torch.empty(slices * per_row + 5, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.VBQError, match="workspace"):
        _dp(fhat, budget, workspace=torch.empty(per_row - 1, dtype=torch.uint8, device="cuda"))
    # more rows than the grid of the LDS path has workgroups is not reachable in a test (2**20); many rows on a small shape
    _same(_scores(np.random.default_rng(6), 4, 5000, 5), 9)


@gpu
@pytest.mark.parametrize("K,N", [(2, 3), (7, 4), (20, 10), (100, 10), (300, 4)])
def test_ties_take_the_first_maximum(K, N):
    """Scores rounded to multiples of 0.25: sums are exact and equal sums are the rule, so the allocation is decided by the
    first-maximum order alone."""
    _need_gpu()
    rng = np.random.default_rng(77 * K + N)
    fhat = np.round(-np.abs(rng.standard_normal((N + 1, 4, K))) * 2 * 4) / 4
    fhat[:, 3, :] = 0.0                                                                       # a row where EVERYTHING ties
    for budget in sorted({0, 1, N, K * N, K * N // 3, K * N // 2}):
        _same(fhat, budget)


@gpu
@pytest.mark.parametrize("K,N", [(1, 4), (2, 4), (7, 10), (100, 10)])
def test_minus_inf_entries(K, N):
    _need_gpu()
    rng = np.random.default_rng(31 * K + N)
    fhat = _scores(rng, N, 5, K)
    fhat[rng.uniform(size=fhat.shape) < 0.3] = -np.inf
    fhat[:, 3, :] = -np.inf                                      # no finite allocation at all: objective -inf
    fhat[1:, 4, :] = -np.inf                                     # only "0 bits everywhere" is finite
    for budget in sorted({0, 1, N, K * N, K * N // 3}):
        _same(fhat, budget)
    _, obj = _dp(fhat, K * N // 3)
    assert obj[3] == -np.inf


@gpu
def test_nan_row_sets_status_and_leaves_the_other_rows_exact():
    _need_gpu()
    K, N, budget = 40, 10, 130
    rng = np.random.default_rng(9)
    fhat = _scores(rng, N, 6, K)
    clean = fhat.copy()
    fhat[3, 2, 17] = np.nan
    fhat[0, 4, 0] = np.inf
    status = torch.zeros(1, dtype=torch.uint32, device="cuda")
    bits, obj = _dp(fhat, budget, status=status)
    assert int(status.cpu().item()) & 1
    want_bits, want_obj = BR.budget_dp_rows(clean, budget)
    ok = [0, 1, 3, 5]
    assert np.array_equal(bits[ok], want_bits[ok]) and obj[ok].tobytes() == want_obj[ok].tobytes()
    assert bits.min() >= 0 and bits.max() <= N
    status.zero_()
    _dp(clean, budget, status=status)
    assert int(status.cpu().item()) == 0
    fhat[:, :, :] = np.nan                                        # nothing but NaN, and a remainder far above N
    bits, _ = _dp(fhat, K * N, status=status)
    assert int(status.cpu().item()) & 1 and bits.min() >= 0 and bits.max() <= N


@gpu
def test_public_encode_functions_reproduce_the_reference(g14):
    _need_gpu()
    from vbq_amd import utils as U
    M = int(g14["em_max_bits"])
    for c in BR.g14_cases(g14):
        K, N = c["K"], c["N"]
        f, squash, unsquash = BR.gaussian_callables(c["mu"], c["sigma"], c["prior_scale"])
        mode_hat, obj, num_bits = U.encode_mode_dp(f, c["mu"], N, squash, unsquash, c["zero_bit_mode_hat"])
        assert np.array_equal(num_bits, c["dp_num_bits"]), (K, N)
        assert np.float64(obj).tobytes() == c["dp_obj"].tobytes(), (K, N)
        assert np.asarray(mode_hat, np.float64).tobytes() == c["dp_mode_hat"].tobytes(), (K, N)
        for i, lamb in enumerate(g14["em_lambdas"]):
            mode_hat, obj, num_bits = U.encode_mode(f, c["mu"], float(lamb), squash, unsquash, c["zero_bit_mode_hat"],
                                                    max_bits_per_coord=M)
            assert np.array_equal(num_bits, c["em_num_bits"][i]), (K, lamb)
            assert obj == c["em_obj"][i], (K, lamb)
            assert np.asarray(mode_hat, np.float64).tobytes() == c["em_mode_hat"][i].tobytes(), (K, lamb)


# ------------------------------------------------------------------ quantize_rows_to_budget
def _latents(rng, R, K, per_column, N):
    import vbq_amd
    scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), K)) if per_column else np.array([1.0])
    tab = vbq_amd.gaussian_table(scale, N=N)                                                  # [K, T] / [1, T]
    mu = (scale * rng.standard_normal((R, K))).astype(np.float32)
    mu[0, :] = 50.0                                                                           # beyond every table's end
    sg = np.clip(np.exp(-2 + 0.7 * rng.standard_normal((R, K))), 1e-4, 10).astype(np.float32)
    return mu, sg, (tab if per_column else tab[0])


def _check_rows(mu, sg, tab, N, budgets, idx, num_bits, objective):
    """What quantize_rows_to_budget promises, from its outputs and the candidates it was given."""
    from vbq_amd import rows_budget, tables
    R, K = mu.shape
    tab2 = np.asarray(tab).reshape(-1, tab.shape[-1])
    scores, values = rows_budget.level_candidates(torch.from_numpy(mu).cuda(), torch.from_numpy(sg).cuda(),
                                                  torch.from_numpy(tab2).cuda(), N)
    scores, values = scores.cpu().numpy(), values.cpu().numpy()
    # the candidates are code points of their level, scored in float64 on the upcast float32 values; level 0 is the root
    want = -0.5 * (((values.astype(np.float64) - mu.astype(np.float64)) / sg.astype(np.float64)) ** 2)
    assert scores.tobytes() == want.tobytes()
    for n in range(N + 1):
        for k in range(K):
            level = tab2[k if tab2.shape[0] > 1 else 0, 2 ** n - 1: 2 ** (n + 1) - 1]
            assert np.isin(values[n, :, k], level).all(), (n, k)
    idx, num_bits, objective = idx.cpu().numpy(), num_bits.cpu().numpy(), objective.cpu().numpy()
    assert idx.dtype == np.uint16 and num_bits.dtype == np.int32 and objective.dtype == np.float64
    budgets = np.broadcast_to(np.asarray(budgets), (R,))
    assert np.array_equal(num_bits.sum(axis=1), budgets)
    assert num_bits.min() >= 0 and num_bits.max() <= N
    for b in np.unique(budgets):
        rows = np.nonzero(budgets == b)[0]
        want_bits, want_obj = BR.budget_dp_rows(scores[:, rows], int(b))
        assert np.array_equal(num_bits[rows], want_bits) and objective[rows].tobytes() == want_obj.tobytes(), b
    chosen = np.take_along_axis(values, num_bits[None].astype(np.int64), axis=0)[0]           # [R, K]
    srt = tables.level_major_to_sorted(tab2)
    for k in range(K):
        s = srt[k if tab2.shape[0] > 1 else 0]
        assert np.array_equal(s[idx[:, k]], chosen[:, k]), k
        assert np.array_equal(idx[:, k], np.searchsorted(s, chosen[:, k], side="left")), k    # the lower bound
    return scores


@gpu
@pytest.mark.parametrize("per_column", [False, True])
@pytest.mark.parametrize("R,K,N,total", [(9, 1, 4, 3), (40, 7, 10, 23), (12, 100, 10, 300), (5, 20, 6, 0), (5, 20, 6, 120)])
def test_quantize_rows_to_budget(per_column, R, K, N, total):
    _need_gpu()
    import vbq_amd
    mu, sg, tab = _latents(np.random.default_rng(R * K + N), R, K, per_column, N)
    idx, num_bits, objective = vbq_amd.quantize_rows_to_budget(mu, sg, total, table=tab, N=N)
    assert idx.is_cuda and num_bits.is_cuda and objective.is_cuda and tuple(idx.shape) == (R, K)
    _check_rows(mu, sg, tab, N, total, idx, num_bits, objective)


@gpu
def test_budget_array_gives_the_rows_of_separate_calls():
    _need_gpu()
    import vbq_amd
    R, K, N = 30, 12, 10
    rng = np.random.default_rng(3)
    mu, sg, tab = _latents(rng, R, K, True, N)
    budgets = rng.choice([0, 5, 40, 41, K * N], size=R)
    idx, num_bits, objective = vbq_amd.quantize_rows_to_budget(mu, sg, budgets, table=tab, N=N)
    _check_rows(mu, sg, tab, N, budgets, idx, num_bits, objective)
    for b in np.unique(budgets):
        rows = np.nonzero(budgets == b)[0]
        i1, n1, o1 = vbq_amd.quantize_rows_to_budget(mu[rows], sg[rows], int(b), table=tab, N=N)
        assert np.array_equal(i1.cpu().numpy(), idx.cpu().numpy()[rows]), b
        assert np.array_equal(n1.cpu().numpy(), num_bits.cpu().numpy()[rows]), b
        assert o1.cpu().numpy().tobytes() == objective.cpu().numpy()[rows].tobytes(), b
    with pytest.raises(vbq_amd.VBQError, match="budget"):
        vbq_amd.quantize_rows_to_budget(mu, sg, K * N + 1, table=tab, N=N)
    with pytest.raises(vbq_amd.VBQError, match="NaN"):
        vbq_amd.quantize_rows_to_budget(mu, np.full_like(sg, np.nan), 10, table=tab, N=N)


@gpu
def test_dp_at_the_rate_of_a_lambda_solution_is_at_least_as_good():
    """The raw-length quantize() solution at lambda spends B* bits in a row; it is ONE allocation of B* bits (its point on every
    level scores no better than that level's best neighbour), so the DP at B* is at least as good -- in float64, with both sums
    folded over ascending k, exactly (rounding is monotone)."""
    _need_gpu()
    import vbq_amd
    from vbq_amd import tables
    R, K, N = 60, 16, 10
    mu, sg, tab = _latents(np.random.default_rng(8), R, K, True, N)
    mu[0] = mu[1]                                                                             # (keep every row inside the tables)
    srt, lev = tables.level_major_to_sorted(tab), tables.level_of_rank(N)
    for lam in (0.05, 0.5, 3.0):
        q = vbq_amd.quantize(mu, sg, lam, table=tab, N=N)                                     # [R, K] rank indices
        bits = lev[q.astype(np.int64)]
        z = np.take_along_axis(srt.T, q.astype(np.int64), axis=0)                             # srt[k, q[r, k]]
        s = -0.5 * (((z.astype(np.float64) - mu.astype(np.float64)) / sg.astype(np.float64)) ** 2)
        score = np.add.accumulate(s, axis=1)[:, -1]
        b_star = bits.sum(axis=1)
        _, num_bits, objective = vbq_amd.quantize_rows_to_budget(mu, sg, b_star, table=tab, N=N)
        assert np.array_equal(num_bits.cpu().numpy().sum(axis=1), b_star)
        obj = objective.cpu().numpy()
        assert (obj >= score).all(), lam
