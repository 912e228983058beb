"""Exhaustive rate-distortion reference (TEST INFRASTRUCTURE ONLY).

Scores EVERY code point of an element's channel -- no descent, no candidate assembly -- in the
arithmetic of a score mode, so that it shares nothing with the 21-candidate solve it checks:

* ``"f32"`` (VBQ_MODE_F32, the TF-eager path): d = -0.5 * ((p - mu) / sigma)**2 in four
  separately rounded f32 ops, then ``fl32(lambda) * len`` and ``d - pen`` in f32.
* ``"f64"`` (VBQ_MODE_F64_SCORE, the reference's NumPy backend, utils.py:388-401): the same f32
  distortion, then ``float64(lambda) * len`` and ``float64(d) - pen`` in f64.

The tests compare VALUES: the score of the code point a kernel chose must equal the maximum over
all T points.  That holds whatever the kernel's tie order, and fails when it picks a worse point.
"""
import numpy as np

F32 = np.float32


def distortion(p, mu, sigma):
    """utils.py:319-320 (ignore_const=True), f32 op by op; broadcasts."""
    p, mu, sigma = (np.asarray(a, F32) for a in (p, mu, sigma))
    with np.errstate(all="ignore"):
        t = (p - mu) / sigma
        return F32(-0.5) * (t * t)


def score(p, ln, mu, sigma, lamb, mode):
    """Mode-aware score of code point(s) p with code length(s) ln for element(s) (mu, sigma); broadcasts.
    Returns f32 (mode "f32") or f64 (mode "f64")."""
    d = distortion(p, mu, sigma)
    with np.errstate(all="ignore"):
        if mode == "f32":
            return d - F32(lamb) * np.asarray(ln, F32)
        if mode == "f64":
            return d.astype(np.float64) - np.float64(lamb) * np.asarray(ln, np.float64)
    raise ValueError(mode)


def slot_levels(N):
    """Bit level of every slot of a level-major table: slot (n, i) at 2**n - 1 + i."""
    return np.concatenate([np.full(2 ** n, n, np.int64) for n in range(N + 1)])


def exhaustive_max(mu, sigma, table_lm, lambdas, N, level_len=None, mode="f32", chunk=1 << 22):
    """max over the T code points of each element's channel of score(point, len(level)).
    mu, sigma: [rows, C] (or [rows] for one channel); table_lm: [C, T] level-major; level_len: optional [L, C, N+1]
    (raw lengths = the level otherwise).  Returns [L, rows, C] (f32 or f64 by mode)."""
    mu = np.asarray(mu, F32)
    sigma = np.asarray(sigma, F32)
    if mu.ndim == 1:
        mu, sigma = mu[:, None], sigma[:, None]
    rows, C = mu.shape
    tab = np.asarray(table_lm, F32).reshape(C, -1)
    T = tab.shape[1]
    assert T == 2 ** (N + 1) - 1
    lev = slot_levels(N)
    L = len(lambdas)
    out = np.empty((L, rows, C), np.float64 if mode == "f64" else F32)
    step = max(1, chunk // T)
    for c in range(C):
        for r0 in range(0, rows, step):
            r1 = min(rows, r0 + step)
            d = distortion(tab[c][None, :], mu[r0:r1, c, None], sigma[r0:r1, c, None])    # [rows, T]
            if mode == "f64":
                d = d.astype(np.float64)
            for i, lamb in enumerate(lambdas):
                ln = lev if level_len is None else np.asarray(level_len, F32)[i, c][lev]
                with np.errstate(all="ignore"):
                    if mode == "f32":
                        s = d - F32(lamb) * ln.astype(F32)
                    else:
                        s = d - np.float64(lamb) * ln.astype(np.float64)
                out[i, r0:r1, c] = s.max(axis=1)
    return out


def chosen_scores(mu, sigma, table_lm, lambdas, N, idx, level_len=None, mode="f32"):
    """Score of the code point each element was given: idx u16 [L, rows, C] ranks into the channel's sorted table
    (the kernels' output).  Returns [L, rows, C] like exhaustive_max."""
    mu = np.asarray(mu, F32)
    sigma = np.asarray(sigma, F32)
    if mu.ndim == 1:
        mu, sigma = mu[:, None], sigma[:, None]
    idx = np.asarray(idx).astype(np.int64).reshape((len(lambdas),) + mu.shape)
    C = mu.shape[1]
    tab = np.asarray(table_lm, F32).reshape(C, -1)
    srt = np.sort(tab, axis=1)
    k = idx + 1                                             # rank k = 1..T has level N - ctz(k)
    ctz = np.zeros_like(k)
    for _ in range(N + 1):
        even = (k & 1) == 0
        ctz += even
        k = np.where(even, k >> 1, k)
    lvl = N - ctz
    out = np.empty(idx.shape, np.float64 if mode == "f64" else F32)
    for i, lamb in enumerate(lambdas):
        p = np.take_along_axis(srt, idx[i].T, axis=1).T
        ln = lvl[i] if level_len is None else np.take_along_axis(np.asarray(level_len, F32)[i].T, lvl[i], axis=0)
        out[i] = score(p, ln, mu, sigma, lamb, mode)
    return out
