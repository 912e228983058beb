"""Float64 NumPy restatement of the budget DP (img-compression/utils.py:106-160, generalised to any budget) and of the patience
scan (utils.py:186-203): what vbq_budget_dp_f64 / vbq_budget_patience_f64 are tested against, bit for bit.  Test infrastructure
only; g14 ties it to the reference (tests/test_budget_dp_host.py).

    T[0][n] = fhat(0, n) for n <= N, -inf for n > N
    T[k][n] = max over m = 0..min(n, N) of fhat(k, m) + T[k-1][n-m]      (one rounded add; the first maximum in ascending m)
"""
import itertools

import numpy as np


def budget_dp_rows(fhat, budget):
    """fhat: f64 [N+1, R, K] -> (bits int64 [R, K], obj f64 [R]).  Every row's bits sum to `budget`; coordinate 0 takes the
    remainder.  Entries must be finite or -inf."""
    fhat = np.asarray(fhat, dtype=np.float64)
    N, R, K = fhat.shape[0] - 1, fhat.shape[1], fhat.shape[2]
    W = budget + 1
    assert 0 <= budget <= K * N
    T = np.full((R, W), -np.inf)
    top = min(W, N + 1)
    T[:, :top] = fhat[:top, :, 0].T
    back = np.zeros((K, R, W), dtype=np.int64)
    rr = np.arange(R)[:, None]
    for k in range(1, K):
        # m > n is no candidate: -inf there can tie with a candidate but never beat one, and every candidate comes first
        cand = np.full((N + 1, R, W), -np.inf)
        for m in range(min(N, budget) + 1):
            cand[m, :, m:] = fhat[m, :, k][:, None] + T[:, :W - m]
        best = np.argmax(cand, axis=0)                                  # the first maximum in ascending m
        back[k] = best
        T = cand[best, rr, np.arange(W)[None, :]]
    obj = T[:, budget].copy()
    bits = np.zeros((R, K), dtype=np.int64)
    left = np.full(R, budget, dtype=np.int64)
    for k in range(K - 1, 0, -1):
        bits[:, k] = back[k, np.arange(R), left]
        left -= bits[:, k]
    bits[:, 0] = left
    return bits, obj


def budget_dp(fhat, budget):
    """One row: fhat f64 [N+1, K] -> (bits int64 [K], obj)."""
    bits, obj = budget_dp_rows(np.asarray(fhat, dtype=np.float64)[:, None, :], budget)
    return bits[0], obj[0]


def brute_force(fhat, budget):
    """The largest left-to-right float64 sum over ALL allocations of exactly `budget` bits, at most N each (tiny cases only)."""
    fhat = np.asarray(fhat, dtype=np.float64)
    N, K = fhat.shape[0] - 1, fhat.shape[1]
    best = -np.inf
    for alloc in itertools.product(range(N + 1), repeat=K):
        if sum(alloc) != budget:
            continue
        s = fhat[alloc[0], 0]
        for k in range(1, K):
            s = s + fhat[alloc[k], k]
        best = max(best, s)
    return best


def patience_scan(fhat, lamb, patience=3):
    """fhat f64 [N+1, E] -> (bits int64 [E], g f64 [E]): g_0 = fhat_0, g_b = fhat_b - lamb * b; a strictly greater g is the new
    best and resets the counter; `patience` non-improvements in a row end the scan."""
    fhat = np.asarray(fhat, dtype=np.float64)
    N, E = fhat.shape[0] - 1, fhat.shape[1]
    bits, g = np.zeros(E, dtype=np.int64), np.full(E, -np.inf)
    for e in range(E):
        bad = 0
        for b in range(N + 1):
            v = fhat[0, e] if b == 0 else fhat[b, e] - np.float64(lamb) * np.float64(b)
            if v > g[e]:
                g[e], bits[e], bad = v, b, 0
            else:
                bad += 1
                if bad == patience:
                    break
    return bits, g


def gaussian_callables(mu, sigma, prior_scale):
    """The per-coordinate scalar functions g14 was recorded with (tests/golden/make_golden_budget.py)."""
    from scipy.stats import norm
    f = [lambda z, m=m, s=s: -0.5 * ((z - m) / s) ** 2 for m, s in zip(mu, sigma)]
    squash = [lambda z, p=p: norm.cdf(z, loc=0.0, scale=p) for p in prior_scale]
    unsquash = [lambda xi, p=p: norm.ppf(xi, loc=0.0, scale=p) for p in prior_scale]
    return f, squash, unsquash


def g14_cases(g):
    """The cases of g14 cut out of its flat per-field arrays: dicts with K, N and the fields in their shapes."""
    L, M = len(g["em_lambdas"]), int(g["em_max_bits"])
    pos = {}
    for K, N in zip(g["case_K"].tolist(), g["case_N"].tolist()):
        shapes = {"mu": (K,), "sigma": (K,), "prior_scale": (K,), "zero_bit_mode_hat": (K,), "scores": (N + 1, K),
                  "values": (N + 1, K), "dp_mode_hat": (K,), "dp_obj": (), "dp_num_bits": (K,), "em_scores": (M + 1, K),
                  "em_values": (M + 1, K), "em_mode_hat": (L, K), "em_obj": (L,), "em_num_bits": (L, K)}
        c = {"K": K, "N": N}
        for key, shape in shapes.items():
            n = int(np.prod(shape, dtype=np.int64))
            at = pos.get(key, 0)
            c[key] = g[key][at:at + n].reshape(shape)
            pos[key] = at + n
        yield c
