"""The position phase of the threshold kernels -- bucket, sweep position, guard band, counter update -- bit for bit against the
C oracle: K1t (k_level_counts_hull) through ops.level_counts with raw lengths, K1e (k_quant_hull_idx) through ops.quantize on
the same sweeps (K1nt has the notebook tests).  N = 10, the one depth the two kernels are built for.

Two channels of 513 rows; every launch takes the first `rows` rows of one channel or of both (planes).  Every fourth row, and
every second one of the second channel, is one of:
    hit       mu on the level-0 point, sigma 1: deeper levels only lose, thresholds at or below zero;
    overflow  sigma 1e-4 and mu 1e17: every distortion is infinite, the element takes the flagged route -- more than the 192
              entries of a workgroup's queue among the first 512 rows of the second channel;
    clamp     mu on a level-1 point and sigma near 1e-19: a finite level-0 distortion above 1e38, its threshold at the 1e38 clamp;
the others are random latents.  Sweeps: 32 values ON thresholds of the random elements (inside their guard bands), 31 values
inside one octave (most thresholds below the first bucket or above the last), two and one of the first."""
import functools

import numpy as np
import pytest

import launch_plans as LP
from fast_solve_runs import dev
from oracle import c_oracle as CO
from oracle import vbq_oracle as O

N = 10
F32 = np.float32
ROWS = (1, 2, 127, 128, 129, 513)
MAX_ROWS = max(ROWS)
QUEUE = 192                                                   # kFixQueue

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    from vbq_amd import ops as _ops
    return _ops


def _du(tab_c, mu, sg):
    """Per-level distortion of the nearer neighbour, [rows, N + 1], in the reference's f32 operations."""
    with np.errstate(over="ignore", invalid="ignore"):
        t = (tab_c[None, :] - mu[:, None]) / sg[:, None]
        d = F32(0.5) * (t * t)
    return np.stack([d[:, a:b].min(axis=1) for a, b in O.level_slices(N)], axis=1)


def _thresholds(du):
    """T_n = max_{j > n} min_{i <= n} (du_i - du_j) / (j - i), [rows, N], in f64 from the f32 distortions."""
    du = du.astype(np.float64)
    T = np.empty((du.shape[0], N))
    with np.errstate(over="ignore", invalid="ignore"):
        for n in range(N):
            T[:, n] = np.max([np.min([(du[:, i] - du[:, j]) / (j - i) for i in range(n + 1)], axis=0) for j in range(n + 1, N + 1)], axis=0)
    return T


@functools.lru_cache(maxsize=None)
def data():
    rng = np.random.default_rng(1010)
    C = 2
    scale = np.array([0.7, 1.9])
    orc = O.ChannelwiseOracle(C, N)
    orc.build_code_points(O.factored_gaussian_icdf(np.zeros(C), scale))
    tab = orc.all_code_points.astype(F32)
    mu = (scale * rng.normal(0, 1.0, (MAX_ROWS, C))).astype(F32)
    sg = np.clip(np.exp(rng.normal(-2, 0.7, (MAX_ROWS, C))), 1e-4, 10).astype(F32)
    kind = np.full((MAX_ROWS, C), -1)
    kind[1::4, 0] = np.arange(len(kind[1::4, 0])) % 3          # rows 1, 5, 9, ..: hit, overflow, clamp in turn
    kind[0::2, 1] = 1                                          # the second channel: every second row overflows ..
    kind[1::8, 1] = np.arange(len(kind[1::8, 1])) % 3          # .. and the two other kinds now and then
    for c in range(C):
        mu[kind[:, c] == 0, c], sg[kind[:, c] == 0, c] = tab[c, 0], 1.0
        mu[kind[:, c] == 1, c], sg[kind[:, c] == 1, c] = 1e17, 1e-4
        # on a level-1 point, level 0 at t = 1.7e19: du_0 = 1.4e38 (t * t still finite), du_1 = 0, T_0 = du_0 - du_1 above the clamp
        mu[kind[:, c] == 2, c], sg[kind[:, c] == 2, c] = tab[c, 2], F32(abs(float(tab[c, 2]) - float(tab[c, 0])) / 1.7e19)
    du = [_du(tab[c], mu[:, c], sg[:, c]) for c in range(C)]
    T = [_thresholds(d) for d in du]
    assert (kind[:512, 1] == 1).sum() > QUEUE and np.isinf(du[1][kind[:, 1] == 1]).all()
    assert all((T[c][kind[:, c] == 0] <= 0).any() for c in range(C))
    assert all((T[c][kind[:, c] == 2] >= 1e38).any() and np.isfinite(du[c][kind[:, c] == 2]).all() for c in range(C))
    # 32 sweep points on thresholds of random elements, each as the f32 the kernel forms, a bucket (7 mantissa bits) apart
    cand = np.sort(np.concatenate([T[c][kind[:, c] == -1].ravel() for c in range(C)]))
    cand = cand[(cand > 1e-3) & (cand < 50.0)]
    on = []
    for target in np.geomspace(4e-3, 30.0, 32):               # the threshold nearest to each point of a sweep like the headline's
        v = float(F32(cand[np.argmin(np.abs(np.log(cand / target)))]))
        if not on or v > on[-1] * 1.03:
            on.append(v)
    assert len(on) == 32, len(on)
    octave = [float(v) for v in np.linspace(0.75, 1.45, 31)]    # 31 points inside one octave: 0.023 apart, buckets are 0.004 to 0.008 wide
    order = rng.permutation(32)
    sweeps = {"on-thresholds-32": [on[i] for i in order], "one-octave-31": octave, "two": [on[20], on[5]], "one": [on[10]]}
    allT = np.concatenate([t.ravel() for t in T])
    assert ((allT > 0) & (allT < 0.7)).any() and (allT > 1.5).any()              # below the first bucket of `octave`, above its last
    for lam in sweeps.values():
        assert LP.sweep_eligible(lam) and LP.solve_kernel(N, lam, "cb", C, counting=True) == "K1t"
    lev = O.levels_of_sorted_ranks(N)
    want = {}
    for name, lam in sweeps.items():
        idx = CO.quantize(mu, sg, tab, lam, N=N, threads=8)                       # [L, rows, C], raw lengths
        idx.setflags(write=False)
        want[name] = idx
    for a in (tab, mu, sg):
        a.setflags(write=False)
    return tab, mu, sg, sweeps, want, lev


def _counts(idx, lev, rows, chans):
    return np.stack([[np.bincount(lev[idx[l, :rows, c]], minlength=N + 1) for c in chans] for l in range(idx.shape[0])]).astype(np.int64)


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("sweep", ["on-thresholds-32", "one-octave-31", "two", "one"])
def test_level_counts_on_every_position_path(ops, sweep, C):
    tab, mu, sg, sweeps, want, lev = data()
    lam = sweeps[sweep]
    for rows in ROWS:
        for chans in ([(0, 1)] if C == 2 else [(0,), (1,)]):
            ch = list(chans)
            if C == 2:
                got = ops.level_counts(dev(mu[:rows].T), dev(sg[:rows].T), dev(tab), lam, N=N, layout="cb")
            else:
                got = ops.level_counts(dev(mu[:rows, ch[0]]), dev(sg[:rows, ch[0]]), dev(tab[ch]), lam, N=N)
            w = _counts(want[sweep], lev, rows, ch)
            assert np.array_equal(got.cpu().numpy(), w), (sweep, rows, chans, np.argwhere(got.cpu().numpy() != w)[:5].tolist())


def test_rank_indices_on_the_same_sweeps(ops):
    """K1e takes the bucket routine too: the 32 on-threshold points and 16 of them, planes and one code book, odd row counts."""
    tab, mu, sg, sweeps, want, _ = data()
    lam32 = sweeps["on-thresholds-32"]
    for lam, pick in ((lam32, slice(0, 32)), (lam32[::2], slice(0, 32, 2))):
        assert LP.solve_kernel(N, lam, "cb", 2, elements=2 * MAX_ROWS) == "K1e"
        w = want["on-thresholds-32"][pick]
        got = ops.quantize(dev(mu.T), dev(sg.T), dev(tab), lam, N=N, layout="cb").cpu().numpy().transpose(0, 2, 1)
        assert np.array_equal(got, w), len(lam)
        got = ops.quantize(dev(mu[:129, 1]), dev(sg[:129, 1]), dev(tab[1:]), lam, N=N).cpu().numpy()
        assert np.array_equal(got, w[:, :129, 1]), len(lam)
