"""oracle/rd_f64.py, the exhaustive reference the literal-solve GPU tests (test_gpu_literal_solve.py) check
against, pinned on the CPU: against the golden vectors of the reference (G5 in both score modes, G6's exhaustive
search) and against the C oracle's 21-candidate solve."""
import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import rd_f64 as R
from oracle import vbq_oracle as O

N = 10


def _g5_tables(g):
    C = g["mu"].shape[1]
    orc = O.ChannelwiseOracle(C, N)
    orc.build_code_points(O.factored_gaussian_icdf(g["ch_mean"], g["ch_std"]))
    assert np.array_equal(orc.all_code_points, g["all_code_points"])
    return orc


@pytest.mark.parametrize("mode", ["f32", "f64"])
def test_g5_winners_reach_the_exhaustive_maximum(golden, mode):
    g = golden("g5_batch_quantize.npz")
    lam = list(g["lambdas"])
    best = R.exhaustive_max(g["mu"], g["sigma"], g["all_code_points"], lam, N, mode=mode)
    got = np.stack([R.score(g["zhat_" + mode][i], g["bits_" + mode][i], g["mu"], g["sigma"], l, mode)
                    for i, l in enumerate(lam)])
    assert got.dtype == best.dtype == (np.float64 if mode == "f64" else np.float32)
    assert np.array_equal(got, best)
    # the other mode's winners are scored by this mode's arithmetic: never above the maximum
    other = "f32" if mode == "f64" else "f64"
    for i, l in enumerate(lam):
        assert np.all(R.score(g["zhat_" + other][i], g["bits_" + other][i], g["mu"], g["sigma"], l, mode) <= best[i])


def test_g6_brute_force_is_the_exhaustive_maximum(golden):
    g5, g6 = golden("g5_batch_quantize.npz"), golden("g6_brute_force.npz")
    rows = g6["rows"]
    best = R.exhaustive_max(g5["mu"][rows], g5["sigma"][rows], g5["all_code_points"], list(g5["lambdas"][g6["lam_idx"]]), N)
    for a, li in enumerate(g6["lam_idx"]):
        s = R.score(g6["zhat"][a], g6["bits"][a], g5["mu"][rows], g5["sigma"][rows], g5["lambdas"][li], "f32")
        assert np.array_equal(s, best[a])


def test_chosen_scores_of_the_rank_indices(golden):
    """chosen_scores reads the kernels' output (ranks into the sorted table) back to points and levels."""
    g = golden("g5_batch_quantize.npz")
    orc = _g5_tables(g)
    lam = list(g["lambdas"])
    idx = O.qidx_lookup(orc.by_channel, g["zhat_f64"].reshape(-1, orc.C)).T.reshape(g["zhat_f64"].shape)
    s = R.chosen_scores(g["mu"], g["sigma"], g["all_code_points"], lam, N, idx, mode="f64")
    assert np.array_equal(s, R.exhaustive_max(g["mu"], g["sigma"], g["all_code_points"], lam, N, mode="f64"))
    assert np.array_equal(O.levels_of_sorted_ranks(N)[idx], g["bits_f64"])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("Nb,C", [(4, 3), (7, 2), (10, 5), (12, 1)])
def test_c_oracle_reaches_the_exhaustive_maximum(mode, Nb, C):
    rng = np.random.default_rng(40 + Nb * 2 + mode)
    orc = O.ChannelwiseOracle(C, Nb)
    orc.build_code_points(O.factored_gaussian_icdf(rng.normal(0, 0.3, C), np.exp(rng.uniform(-1, 1, C))))
    rows = 400
    mu = rng.normal(0, 1.5, (rows, C)).astype(np.float32)
    sg = np.exp(rng.normal(-2, 1.0, (rows, C))).astype(np.float32)
    srt = np.sort(orc.all_code_points, axis=1)
    mu[:20] = srt[:, rng.integers(0, srt.shape[1], 20)].T                       # exact hits
    mu[20:25] = srt[:, -1] + np.float32(1.0)                                    # above the last point: no deepest-level padding
    mu[25:30] = srt[:, 0] - np.float32(1.0)
    lam = [0.0, 2.0 ** -8 * np.sqrt(2.0), 0.1, 1.0, 37.0, 1e25]
    ll = (np.arange(Nb + 1, dtype=np.float32)[None, None] + rng.uniform(0, 3, (len(lam), C, Nb + 1))).astype(np.float32)
    for level_len in ((None, ll) if mode == 0 else (None,)):
        idx = CO.quantize(mu, sg, orc.all_code_points, lam, N=Nb, level_len=level_len, mode=mode, threads=8)
        m = "f64" if mode else "f32"
        best = R.exhaustive_max(mu, sg, orc.all_code_points, lam, Nb, level_len=level_len, mode=m)
        assert np.array_equal(R.chosen_scores(mu, sg, orc.all_code_points, lam, Nb, idx, level_len=level_len, mode=m), best)


def test_the_check_fails_on_a_worse_choice():
    """A one-rank shift of the winners must show: the check is not vacuous."""
    rng = np.random.default_rng(3)
    orc = O.ChannelwiseOracle(2, N)
    orc.build_code_points(O.factored_gaussian_icdf(np.zeros(2), np.ones(2)))
    mu = rng.normal(0, 1, (300, 2)).astype(np.float32)
    sg = np.exp(rng.normal(-3, 0.5, (300, 2))).astype(np.float32)
    lam = [0.0, 0.01]
    idx = CO.quantize(mu, sg, orc.all_code_points, lam, N=N, mode=1)
    best = R.exhaustive_max(mu, sg, orc.all_code_points, lam, N, mode="f64")
    bad = np.clip(idx.astype(np.int64) + 1, 0, 2 ** (N + 1) - 2)
    s = R.chosen_scores(mu, sg, orc.all_code_points, lam, N, bad, mode="f64")
    assert np.all(s <= best) and np.sum(s < best) > 500
