"""Elements that split the two score modes of the R-D solve (TEST INFRASTRUCTURE ONLY).

Found by searching seeded candidates with the oracles, for the GPU tests of the literal solves and of K1c: a test run on
this set fails if the f64 mode scored in f32, rounded lambda to f32 first, or took the last maximum instead of the first.
"""
import numpy as np

from . import c_oracle as CO
from . import rd_f64 as R
from . import vbq_oracle as O

F32 = np.float32
SPLIT_LAMS = [0.0, 2.0 ** -8 * np.sqrt(2.0), 0.1, 0.3]


def _candidate_scores(z, s, grids, lam, how):
    """Scores of the 21 candidates [L_0..L_N, R_1..R_N] (NumPy oracle intervals) under the f64 rule and its mutants."""
    Nb = grids.shape[1] - 1
    left, right = O.get_all_N_bit_intervals(grids, z[:, None])
    P = O.assemble_candidates(left, right)[:, :, 0]
    lv = np.concatenate([np.arange(Nb + 1), np.arange(1, Nb + 1)])[:, None]
    if how == "f32_scores":                                          # f64 penalty, then score in f32
        pen = (np.float64(lam) * lv).astype(F32)
        return P, lv, R.distortion(P, z[None], s[None]) - pen
    return P, lv, R.score(P, lv, z[None], s[None], lam, "f64")



def _winner(P, lv, S, last=False):
    j = S.shape[0] - 1 - np.argmax(S[::-1], axis=0) if last else np.argmax(S, axis=0)
    cols = np.arange(S.shape[1])
    return P[j, cols], lv[j, 0]



def mode_splitting_set(seed=2024, n=20000, centre=48):
    """Elements searched from seeded candidates with the oracle: exact-score pairs of adjacent code points near the
    middle of an N = 10 table (where an f32 step of z is small against the tie window), 2 ulps either side; lambda = 0
    midpoints for exact ties.  Kept: the elements where the f32 and f64 winners differ, or where a mutant f64 rule
    (lambda rounded to f32 first, '>=' instead of '>', f64 penalties but f32 scores) moves the winner.  Returns
    (table, mu, sigma, counts of disagreeing elements per rule)."""
    rng = np.random.default_rng(seed)
    orc = O.ChannelwiseOracle(1, 10)
    orc.build_code_points(O.factored_gaussian_icdf(np.zeros(1), np.ones(1)))
    srt = np.sort(orc.all_code_points[0]).astype(np.float64)
    lev = O.levels_of_sorted_ranks(10)
    mid = len(srt) // 2
    zs, ss = [], []
    for lam in SPLIT_LAMS:
        k = rng.integers(mid - centre, mid + centre, n) if lam else rng.integers(0, len(srt) - 1, n // 8)
        a, b = srt[k], srt[k + 1]
        di = (lev[k] - lev[k + 1]).astype(np.float64)
        gap = b - a
        if lam:
            s = np.sqrt(rng.uniform(0.02, 0.98, len(k)) * gap ** 2 / (2 * lam * np.abs(di))).astype(F32)
        else:
            s = np.exp(rng.uniform(np.log(1e-3), 0, len(k))).astype(F32)
        sd = s.astype(np.float64)
        z = (0.5 * (a + b) - sd * sd * lam * di / gap).astype(F32)
        for u in range(-2, 3):
            zu = z
            for _ in range(abs(u)):
                zu = np.nextafter(zu, F32(np.inf) if u > 0 else F32(-np.inf))
            zs.append(zu)
            ss.append(s)
    z, s = np.concatenate(zs), np.concatenate(ss)
    tab = orc.all_code_points
    i32 = CO.quantize(z, s, tab, SPLIT_LAMS, N=10, mode=0, threads=8)[:, :, 0]
    i64 = CO.quantize(z, s, tab, SPLIT_LAMS, N=10, mode=1, threads=8)[:, :, 0]
    il = CO.quantize(z, s, tab, [float(F32(l)) for l in SPLIT_LAMS], N=10, mode=1, threads=8)[:, :, 0]
    ge = np.zeros(i64.shape, bool)
    fs = np.zeros(i64.shape, bool)
    for i, lam in enumerate(SPLIT_LAMS):
        P, lv, S = _candidate_scores(z, s, orc.grids, lam, "f64")
        (p0, l0), (p1, l1) = _winner(P, lv, S), _winner(P, lv, S, last=True)
        ge[i] = (p0 != p1) | (l0 != l1)
        P, lv, S = _candidate_scores(z, s, orc.grids, lam, "f32_scores")
        p2, l2 = _winner(P, lv, S)
        fs[i] = (p0 != p2) | (l0 != l2)
    dis = {"f32_vs_f64": i32 != i64, "lambda_rounded_to_f32": il != i64, "ge_instead_of_gt": ge, "f64_pen_f32_score": fs}
    keep = np.zeros(len(z), bool)
    for d in dis.values():
        keep |= d.any(axis=0)
    keep |= rng.random(len(z)) < 2000 / len(z)
    counts = {k: int(d[:, keep].any(axis=0).sum()) for k, d in dis.items()}
    return tab, z[keep], s[keep], counts
