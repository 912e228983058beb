"""Seeded inputs that reach the two events the fast f32 solve (k_quant_fast, vbq_quantize_fast.hip) cannot decide by itself,
at every bit depth, and a NumPy restatement of the f32 cost chain that counts them.  No GPU and no package import: the
oracle's interval search (oracle.vbq_oracle.get_all_N_bit_intervals) and NumPy's float32 arithmetic only.

The reference scans the candidates [L_0..L_N, R_1..R_N] of an element and keeps the first minimum of
cost = fl(fl(0.5 * fl(t * t)) + fl(fl32(lambda) * len_n)), t = fl(fl(P - mu) / sigma).  The fast kernel keeps one cost per
level, c_n = fl(min(dL_n, dR_n) + pen_n), and answers "the better side of the shallowest level that attains min_n c_n"
unless it raises a flag and re-solves with the literal scan:
    (a)         more than one level attains the minimum (the reference's L-before-R order decides);
    (b)         R is the better side of that level and dL - dR is so small against the cost that fl(dL + pen) may round onto
                fl(dR + pen) -- restated here as: the top 11 bits of fl(dL - dR) are at most the bits of fl(2^-19 S), the
                kernel's test without the rank bits it keeps below the gap;
    (b-merged)  R is strictly nearer and the two rounded costs ARE equal: the reference takes L.
`events` counts them, and the solves at which the unflagged answer differs from the reference's.

Four data families, each as [rows, C] arrays with C = 1 or 2 (`families`):
    dyadic_case          code points on multiples of 1/32, mu on multiples of 1/64, sigma a power of two, dyadic lambdas: every
                         product and sum of the cost chain is exact or nearly so, and cross-level ties (a) are common;
    near_midpoint_case   mu one ulp above the mid-point of two neighbours of level n, a caller length table that makes
                         level n win: (b) in most solves, (b-merged) in many;
    certificate_edge_case  the same mid-points with sigmas that walk (dL - dR) / cost through the octaves around the
                         certificate: merged solves that a tighter certificate would leave unflagged;
    edge_case            `latents`: exact hits, nextafter neighbours, both rims, extreme sigmas.
The second channel of the first three families is the first one scaled by two (table, mu and sigma: every t, hence every
cost and every event, is the same) with a different length table."""
from collections import namedtuple

import numpy as np

from oracle import vbq_oracle as O

F32 = np.float32
DEPTHS = (4, 5, 6, 7, 8, 9, 10, 11, 12)
DYADIC_LAMS = [2.0 ** -12, 2.0 ** -9, 2.0 ** -6, 2.0 ** -3, 1.0, 8.0, 37.0, 0.3]
MIDPOINT_LAMS = [1.0, 8.0]
EDGE_LAMS = [2.0 ** -8 * np.sqrt(2.0), 0.01, 0.1, 1.0, 4.0, 37.0, 300.0, 2.0 ** -5]

Case = namedtuple("Case", "name N tab mu sg lam level_len")
"""tab f32 [C, T] level-major; mu, sg f32 [rows, C]; lam list of L floats; level_len None (raw lengths) or f32 [L, C, N + 1]."""


# ------------------------------------------------------------------------------------------------------------ code books
def gaussian_table(N, step=None):
    """The level-major code book of a standard Gaussian prior, one channel [1, T]; step: rounded to multiples of it (the
    order is kept, neighbours within and across levels coincide)."""
    icdf = O.factored_gaussian_icdf(np.zeros(1), np.ones(1))
    if step is None:
        return O.build_code_points(icdf, 1, N)[0]
    return O.build_code_points(lambda xi: np.round(icdf(xi) / step) * step, 1, N)[0]


def search_grids(tab, N):
    """quantizer.py:54-57 from a level-major table [C, T]: every level padded to 2^N slots with its end points."""
    C = tab.shape[0]
    grids = np.empty((C, N + 1, 2 ** N), F32)
    for c in range(C):
        for n, (a, b) in enumerate(O.level_slices(N)):
            lvl = tab[c, a:b]
            if n == 0:
                grids[c, n] = np.pad(np.array([lvl[0], lvl[0]]), (2 ** (N - 1) - 1,), "edge")
            else:
                grids[c, n] = np.pad(lvl, (2 ** (N - 1) - 2 ** (n - 1),), "edge")
    return grids


def edge_tables(rng, C, N):
    orc = O.ChannelwiseOracle(C, N)
    orc.build_code_points(O.factored_gaussian_icdf(rng.normal(0, 0.2, C), np.exp(rng.uniform(-1, 1, C))))
    return orc.all_code_points


# ------------------------------------------------------------------------------------------------------------ the data
def latents(rng, rows, C, tab):
    """mu, sigma [rows, C] with exact code-point hits, nextafter neighbours, midpoints of adjacent points (L/R ties at
    lambda = 0), points beyond both ends (the deepest level has no edge padding), sigma at 1e-4 and 10 and the
    all-ones mantissa mixed in."""
    srt = np.sort(tab, axis=1)
    T = srt.shape[1]
    scale = np.abs(srt[:, -1] - srt[:, 0]) / 6
    mu = (scale * rng.normal(0, 1.0, (rows, C))).astype(F32)
    sg = np.clip(np.exp(rng.normal(-2.5, 1.0, (rows, C))), 1e-4, 10).astype(F32)
    k = rng.integers(0, T - 1, (rows, C))
    pick = np.take_along_axis(srt.T, k, axis=0)
    nxt = np.take_along_axis(srt.T, k + 1, axis=0)
    kind = rng.integers(0, 12, (rows, C))
    mu = np.where(kind == 0, pick, mu)
    mu = np.where(kind == 1, np.nextafter(pick, F32(np.inf)), mu)
    mu = np.where(kind == 2, np.nextafter(pick, F32(-np.inf)), mu)
    mu = np.where(kind == 3, F32(0.5) * (pick + nxt), mu)
    mu = np.where(kind == 4, srt[:, -1] + np.abs(mu), mu)
    mu = np.where(kind == 5, srt[:, 0] - np.abs(mu), mu)
    mu = np.where(kind == 6, np.nextafter(srt[:, -1], F32(np.inf))[None], mu)
    sg = np.where(kind == 7, F32(1e-4), sg)
    sg = np.where(kind == 8, F32(10.0), sg)
    sg = np.where(kind == 9, F32(2.0) - F32(2.0 ** -23), sg)
    mu = np.where(kind == 10, F32(1.0) - F32(2.0 ** -24), mu)        # all-ones mantissa
    return mu.astype(F32), sg.astype(F32)


def _second_channel(tab, mu, sg):
    """[.., 1] -> [.., 2]: the same solves on a table twice as wide (exact scaling: every quotient t is unchanged)."""
    two = F32(2.0)
    return np.concatenate([tab, two * tab], 0), np.concatenate([mu, two * mu], 1), np.concatenate([sg, two * sg], 1)


def dyadic_case(N, rows=2000, seed=None, C=1):
    """Raw lengths; dyadic_level_len is the caller table that goes with it."""
    rng = np.random.default_rng(N if seed is None else seed)
    tab = gaussian_table(N, step=1.0 / 32)
    mu = (rng.integers(-96, 97, (rows, 1)) / 64.0).astype(F32)       # within 1.5 prior deviations: where the levels compete
    sg = (2.0 ** rng.integers(-3, 3, (rows, 1))).astype(F32)
    if C == 2:
        tab, mu, sg = _second_channel(tab, mu, sg)
    return Case("dyadic", N, tab, mu, sg, list(DYADIC_LAMS), None)


def dyadic_level_len(N, L, C):
    """A caller table in the dyadic spirit: n plus an overhead on multiples of 1/4 that depends on lambda, channel and level."""
    l, c, n = np.meshgrid(np.arange(L), np.arange(C), np.arange(N + 1), indexing="ij")
    return (n + ((5 * n + l + 2 * c) % 4) / 4.0).astype(F32)


def near_midpoint_case(N, n, rows=1000, seed=None, C=1, spread=False):
    """Level n's neighbours pair up at random; mu is the f32 next above their mid-point (R is nearer, by about an ulp of mu),
    sigma = 1, and level n alone is cheap (length 1 against 60, 59 on the second channel).
    spread (certificate_edge_case): sigma = s0 * 2^u instead, u uniform in [0, 8) and s0 the sigma at which level n's
    distortion is 16.  dL - dR grows with 1 / sigma^2 and the cost with 1 + d / sigma^2, so their ratio walks through sixteen
    octaves below about 8 ulp(mu) / (R - L) -- across 2^-23, where the two rounded costs stop merging, and across the
    certificate's 2^-19 .. 2^-20: a certificate that is a few octaves too tight leaves merged solves unflagged here."""
    assert 1 <= n <= N
    rng = np.random.default_rng((2000 if spread else 1000) * N + n if seed is None else seed)
    tab = gaussian_table(N)
    lvl = tab[0, 2 ** n - 1:2 ** (n + 1) - 1]
    j = rng.integers(0, 2 ** n - 1, rows)
    mid = F32(0.5) * (lvl[j] + lvl[j + 1])
    mu = np.nextafter(mid, F32(np.inf)).astype(F32)[:, None]
    sg = np.ones((rows, 1), F32)
    if spread:
        s0 = (lvl[j + 1] - lvl[j]).astype(np.float64) / (2.0 * np.sqrt(32.0))       # 0.5 * ((R - L) / 2 / s0)^2 = 16
        sg = (s0 * 2.0 ** rng.uniform(0, 8, rows)).astype(F32)[:, None]
    if C == 2:
        tab, mu, sg = _second_channel(tab, mu, sg)
    ll = np.full((len(MIDPOINT_LAMS), C, N + 1), 60.0, F32)
    ll[:, 1:] = 59.0
    ll[:, :, n] = 1.0
    return Case(f"{'certificate_edge' if spread else 'near_midpoint'}[{n}]", N, tab, mu, sg, list(MIDPOINT_LAMS), ll)


def certificate_edge_case(N, n, rows=1000, seed=None, C=1):
    return near_midpoint_case(N, n, rows, seed, C, spread=True)


def edge_case(N, rows=301, seed=None, C=1):
    rng = np.random.default_rng(100 + N if seed is None else seed)
    tab = edge_tables(rng, C, N)
    mu, sg = latents(rng, rows, C, tab)
    return Case("edge", N, tab, mu, sg, [float(v) for v in EDGE_LAMS], None)


def edge_level_len(N, L, C, seed=7):
    rng = np.random.default_rng(seed + N)
    return (np.arange(N + 1, dtype=F32)[None, None] + rng.uniform(0, 3, (L, C, N + 1))).astype(F32)


def with_lambdas(case, L, level_len="keep"):
    """The case with its sweep cycled to L lambdas (its own length table cycled with it, or `level_len` instead)."""
    base = len(case.lam)
    pick = [i % base for i in range(L)]
    ll = case.level_len if isinstance(level_len, str) else level_len
    if ll is not None and ll.shape[0] != L:
        ll = np.ascontiguousarray(ll[[i % ll.shape[0] for i in range(L)]])
    return case._replace(lam=[case.lam[i] for i in pick], level_len=ll)


def families(N, C=1, rows=None):
    """The families at depth N (the mid-point ones at both of their levels), in the sizes the GPU tests use."""
    r = {} if rows is None else {"rows": rows}
    return [dyadic_case(N, C=C, **r), near_midpoint_case(N, N // 2, C=C, **r), near_midpoint_case(N, N, C=C, **r),
            edge_case(N, C=C, **r), certificate_edge_case(N, N // 2, C=C, **r), certificate_edge_case(N, N, C=C, **r)]


# ------------------------------------------------------------------------------------------------------------ the restatement
Solved = namedtuple("Solved", "level side zhat bits unflagged_level unflagged_side multi b_flag b_merged")
"""Arrays [L, rows, C].  level, side (True: R), zhat, bits: the reference's winner.  unflagged_*: the fast kernel's answer with
its flags off.  multi, b_flag, b_merged: events (a), (b), (b-merged)."""

Events = namedtuple("Events", "solves a b b_merged differs level_differs")


def restate(case, certificate=2.0 ** -19):
    """The f32 cost chain of utils.py:387-401 on the candidates of quantizer.py:65-80, in NumPy float32 arithmetic.
    certificate: the factor of event (b)'s test (the kernel's is 2^-19); b_merged does not depend on it."""
    N, mu, sg = case.N, case.mu, case.sg
    rows, C = mu.shape
    L = len(case.lam)
    left, right = O.get_all_N_bit_intervals(search_grids(case.tab, N), mu)           # [C, N + 1, rows]
    PL, PR = left.transpose(1, 2, 0), right.transpose(1, 2, 0)                       # [N + 1, rows, C]
    with np.errstate(over="ignore"):
        def dist(P):
            t = (P - mu) / sg
            return F32(0.5) * (t * t)
        dL, dR = dist(PL), dist(PR)
        assert dL.dtype == F32
        if case.level_len is None:
            ln = np.broadcast_to(np.arange(N + 1, dtype=F32)[None, None], (L, C, N + 1))
        else:
            ln = case.level_len
        lam32 = np.asarray(case.lam, np.float64).astype(F32)
        pen = (lam32[:, None, None] * ln).transpose(0, 2, 1)[:, :, None, :]          # [L, N + 1, 1, C]
        assert pen.dtype == F32
        cL, cR = dL[None] + pen, dR[None] + pen                                      # [L, N + 1, rows, C]
        # the reference: first minimum over [L_0 .. L_N, R_1 .. R_N]
        j = np.argmin(np.concatenate([cL, cR[:, 1:]], axis=1), axis=1)               # [L, rows, C]
        level = np.where(j > N, j - N, j)
        side = j > N
        at = lambda a, lv: np.take_along_axis(a, lv[:, None], axis=1)[:, 0]
        zhat = np.where(side, at(np.broadcast_to(PR[None], cL.shape), level), at(np.broadcast_to(PL[None], cL.shape), level))
        bits = np.take_along_axis(np.broadcast_to(ln.transpose(0, 2, 1)[:, :, None, :], cL.shape), level[:, None], axis=1)[:, 0]
        # the fast kernel without its flags: one cost per level, the shallowest level that attains the minimum, its better side
        cmin = np.minimum(dL, dR)[None] + pen
        assert np.array_equal(cmin, np.minimum(cL, cR))                              # rounding is monotone
        S = cmin.min(axis=1)
        attain = cmin == S[:, None]
        multi = attain.sum(axis=1) > 1
        n1 = np.argmax(attain, axis=1)
        r_better = at(np.broadcast_to((dR < dL)[None], cL.shape), n1)
        gap = at(np.broadcast_to((dL - dR)[None], cL.shape), n1)                     # > 0 where R is the better side
        word = np.ascontiguousarray(gap).view(np.uint32) & np.uint32(0xffe00000)
        thr = np.ascontiguousarray(S * F32(certificate)).view(np.uint32)
        b_flag = r_better & (word <= thr)
        b_merged = r_better & (at(cL, n1) == at(cR, n1))
    return Solved(level, side, zhat.astype(F32), bits.astype(F32), n1, r_better, multi, b_flag, b_merged)


def events(case, solved=None):
    s = restate(case) if solved is None else solved
    differs = (s.unflagged_level != s.level) | (s.unflagged_side != s.side)
    return Events(int(s.level.size), int(s.multi.sum()), int(s.b_flag.sum()), int(s.b_merged.sum()), int(differs.sum()),
                  int((s.unflagged_level != s.level).sum()))
