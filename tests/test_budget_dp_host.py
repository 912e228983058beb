"""The budget DP's float64 restatement (tests/budget_reference.py) against the reference's recorded results (g14), against brute
force, and the host-side pieces of the feature: the scalar helpers of vbq_amd.utils and the argument checks of the two entry
points, which run before any device work.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import budget_reference as BR


@pytest.fixture(scope="module")
def g14(golden):
    return golden("g14_budget_dp.npz")


def test_g14_covers_the_case_grid(g14):
    cases = list(BR.g14_cases(g14))
    assert sorted({(int(c["K"]), int(c["N"])) for c in cases}) == [(K, N) for K in (1, 2, 5, 8, 20) for N in (1, 3, 8, 12)]
    assert len(cases) == 20


def test_restatement_equals_the_reference_dp_bit_for_bit(g14):
    for c in BR.g14_cases(g14):
        K, N = int(c["K"]), int(c["N"])
        bits, obj = BR.budget_dp(c["scores"], N)
        assert np.array_equal(bits, c["dp_num_bits"]), (K, N)
        assert np.float64(obj).tobytes() == c["dp_obj"].tobytes(), (K, N)
        mode_hat = c["values"][bits, np.arange(K)]
        assert mode_hat.tobytes() == c["dp_mode_hat"].tobytes(), (K, N)
        assert bits.sum() == N and bits.min() >= 0


def test_patience_restatement_equals_the_reference_encode_mode(g14):
    lambs = g14["em_lambdas"]
    for c in BR.g14_cases(g14):
        K = int(c["K"])
        for i, lamb in enumerate(lambs):
            bits, g = BR.patience_scan(c["em_scores"], float(lamb), 3)
            assert np.array_equal(bits, c["em_num_bits"][i]), (K, lamb)
            assert np.add.accumulate(g)[-1] == c["em_obj"][i], (K, lamb)
            assert c["em_values"][bits, np.arange(K)].tobytes() == c["em_mode_hat"][i].tobytes(), (K, lamb)


@pytest.mark.parametrize("K,N", [(1, 1), (1, 3), (2, 2), (3, 3), (4, 2), (4, 3)])
def test_objective_equals_brute_force_for_every_budget(K, N):
    rng = np.random.default_rng(100 * K + N)
    for trial in range(3):
        fhat = -np.abs(rng.standard_normal((N + 1, K))) * 3
        if trial == 1:
            fhat = np.round(fhat * 4) / 4                       # exact ties
        if trial == 2:
            fhat[rng.integers(0, N + 1), rng.integers(0, K)] = -np.inf
        for budget in range(K * N + 1):
            bits, obj = BR.budget_dp(fhat, budget)
            assert bits.sum() == budget
            assert obj == BR.brute_force(fhat, budget), (K, N, trial, budget)
            if np.isfinite(obj):
                assert bits.min() >= 0 and bits.max() <= N
                s = fhat[bits[0], 0]
                for k in range(1, K):
                    s = s + fhat[bits[k], k]
                assert s == obj                                  # the allocation returned is one that attains the objective


def test_scalar_helpers_reproduce_the_reference(g14):
    from vbq_amd import utils as U
    for x, n, lr in zip(g14["iv_x"], g14["iv_n"], g14["iv_lr"]):
        got = U.get_n_bit_interval(float(x), int(n))
        assert len(got) == 2 and float(got[0]) == lr[0] and float(got[1]) == lr[1], (x, n)
    for x, n, x_hat, bits in zip(g14["iv_x"], g14["iv_n"], g14["tr_x_hat"], g14["tr_bits"]):
        got = U.truncate_float_to_n_bits(float(x), int(n))
        assert got[0] == x_hat and got[1] == str(bits), (x, n)
    assert U.get_n_bit_interval(0.4375, 2) == (0.375, 0.625)        # the reference's docstring example
    f, squash, unsquash = BR.gaussian_callables([0.3], [0.05], [1.5])
    for n in range(14):
        mode_hat, f_hat = U.encode_mode_1d(f[0], 0.3, n, squash[0], unsquash[0])
        assert mode_hat == g14["e1_mode_hat"][n] and f_hat == g14["e1_f_hat"][n], n


def test_argument_validation_runs_without_a_device():
    from vbq_amd import _lib
    h = _lib.lib()
    dp, pa, err = h.vbq_budget_dp_f64, h.vbq_budget_patience_f64, h.vbq_last_error
    one = C.c_void_p(8)                                              # never dereferenced: every call below fails (or has no rows)
    assert dp(one, 4, 3, 10, -1, one, one, None, None, 0, None) == -1 and b"budget" in err()
    assert dp(one, 4, 3, 10, 31, one, one, None, None, 0, None) == -1 and b"budget" in err()
    assert dp(one, 4, 3, 53, 5, one, one, None, None, 0, None) == -1 and b"N=53" in err()
    assert dp(one, 4, 0, 10, 0, one, one, None, None, 0, None) == -1 and b"K=0" in err()
    assert dp(one, -1, 3, 10, 5, one, one, None, None, 0, None) == -1
    assert dp(None, 4, 3, 10, 5, one, one, None, None, 0, None) == -1 and b"null pointer" in err()
    assert dp(one, 4, 3, 10, 5, None, one, None, None, 0, None) == -1 and b"null pointer" in err()
    assert dp(one, 4, 3, 10, 5, one, None, None, None, 0, None) == -1 and b"null pointer" in err()
    assert dp(None, 0, 3, 10, 5, None, None, None, None, 0, None) == 0          # no rows: nothing to do
    # back-pointers that do not fit the LDS need a workspace of at least one row's slice
    assert dp(one, 4, 300, 16, 1600, one, one, None, None, 0, None) == -4 and b"workspace" in err()
    ws = h.vbq_budget_dp_workspace_bytes
    assert ws(100000, 100, 10, 100) == 0 and ws(100000, 100, 10, 600) == 0     # in LDS
    per_row = (300 * 1601 + 15) // 16 * 16
    assert ws(3, 300, 16, 1600) == 3 * per_row
    assert per_row <= ws(10 ** 5, 300, 16, 1600) < 10 ** 5 * per_row            # never the whole table
    assert ws(0, 300, 16, 1600) == 0 and ws(4, 300, 16, 9999) == 0
    assert pa(one, 5, 10, C.c_double(0.1), 0, one, one, None) == -1 and b"patience" in err()
    assert pa(one, -1, 10, C.c_double(0.1), 3, one, one, None) == -1
    assert pa(None, 5, 10, C.c_double(0.1), 3, one, one, None) == -1 and b"null pointer" in err()
    assert pa(None, 0, 10, C.c_double(0.1), 3, None, None, None) == 0
