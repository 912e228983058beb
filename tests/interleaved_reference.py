"""NumPy coder for the wave-interleaved rANS layout (the payload of a VBQc file), vectorised over the 64 lanes.

Written from the format's text (include/vbq.h, vbq_rans_il_encode_u16), not from the kernels; the GPU tests compare the
kernels' sizes, payload bytes and decoded indices with it.  Restated:

  * 32-bit state, start state 2^16, 16-bit words, 15 probability bits; c = exclusive cumulative frequency.
  * The S * n indices in stream-major order are cut every `part` symbols into parts; a run is a maximal stretch of a part
    inside one stream and uses that stream's table; a run of `len` symbols takes ceil(len / 64) steps; in step t lane l owns
    the run's symbol 64 t + l when that is < len.  The 64 lane states carry on from run to run.
  * A part's words as the decoder reads them: 128 state words (lane 0 low, lane 0 high, lane 1 low, ...); then for every run
    and step in order: each active lane decodes (slot = x & 32767; x = f (x >> 15) + slot - c) and each active lane whose
    state is now below 2^16 takes one word, in ascending lane order (x = x << 16 | w).  At the end every word is taken and
    every state is 2^16.
  * The encoder is the inverse: runs last to first, steps last to first; a lane with x >= f << 17 emits x & 0xffff and shifts
    x >>= 16, then x = (x / f << 15) + x % f + c.  A step's words stay in ascending lane order.
"""
import functools

import numpy as np

LANES = 64
PB = 15
L = 1 << 16
STATE_WORDS = 2 * LANES

# (S, n, part) of the kernel tests, each at N = 10 and N = 3
CASES = [(1, 1, 64), (3, 100, 1000), (5, 777, 64), (2, 4096, 4096), (1, 70000, 16384), (64, 1536, 1 << 17)]
SPREADS = [0.2, 2.0, 25.0, 300.0]


def _runs(a, b, n):
    """The runs of the part [a, b): (stream, start, end) with global positions."""
    out = []
    for s in range(a // n, (b - 1) // n + 1):
        out.append((s, max(a, s * n), min(b, (s + 1) * n)))
    return out


def _parts(total, part):
    return [(a, min(a + part, total)) for a in range(0, total, part)]


def encode(idx, freq, part):
    """idx [S, n], freq [S, T] (rows summing to 2^15, entries >= 1) -> (sizes u32 [P], payload u16 [sum(sizes)])."""
    idx = np.asarray(idx)
    S, n = idx.shape
    flat = idx.reshape(-1).astype(np.int64)
    f_all = np.asarray(freq).astype(np.uint64)
    c_all = np.cumsum(f_all, axis=1, dtype=np.uint64) - f_all
    sizes, out = [], []
    for a, b in _parts(S * n, part):
        x = np.full(LANES, L, dtype=np.uint64)
        steps = []                                               # the words of every step, in encoding order
        for s, rs, re in reversed(_runs(a, b, n)):
            for t in reversed(range((re - rs + LANES - 1) // LANES)):
                sym = flat[rs + LANES * t: min(rs + LANES * t + LANES, re)]
                k = sym.size                                     # lanes 0 .. k-1 are active
                f, c = f_all[s, sym], c_all[s, sym]
                xs = x[:k]
                emit = xs >= (f << np.uint64(17))
                steps.append((xs[emit] & np.uint64(0xffff)).astype(np.uint16))
                xs = np.where(emit, xs >> np.uint64(16), xs)
                x[:k] = ((xs // f) << np.uint64(PB)) + xs % f + c
        states = np.empty(STATE_WORDS, dtype=np.uint16)
        states[0::2] = (x & np.uint64(0xffff)).astype(np.uint16)
        states[1::2] = (x >> np.uint64(16)).astype(np.uint16)
        words = np.concatenate([states] + steps[::-1])
        sizes.append(words.size)
        out.append(words)
    payload = np.concatenate(out) if out else np.zeros(0, np.uint16)
    return np.asarray(sizes, dtype=np.uint32), payload.astype(np.uint16)


def decode(sizes, payload, freq, n, part):
    """-> idx u16 [S, n]; ValueError when a part runs out of words, leaves words over or ends in a state other than 2^16."""
    f_all = np.asarray(freq).astype(np.uint64)
    S, T = f_all.shape
    cum = np.concatenate([np.zeros((S, 1), np.uint64), np.cumsum(f_all, axis=1, dtype=np.uint64)], axis=1)   # [S, T + 1]
    payload = np.asarray(payload, dtype=np.uint16)
    flat = np.zeros(S * n, dtype=np.uint16)
    parts = _parts(S * n, part)
    if len(sizes) != len(parts) or int(np.sum(sizes, dtype=np.int64)) != payload.size:
        raise ValueError("sizes do not match the parts or the payload")
    off = 0
    for (a, b), k in zip(parts, (int(v) for v in sizes)):
        if not STATE_WORDS <= k <= (b - a) + STATE_WORDS:
            raise ValueError("part size out of range")
        w = payload[off: off + k].astype(np.uint64)
        off += k
        x = w[0:STATE_WORDS:2] | (w[1:STATE_WORDS:2] << np.uint64(16))
        rp = STATE_WORDS
        for s, rs, re in _runs(a, b, n):
            for t in range((re - rs + LANES - 1) // LANES):
                lo = rs + LANES * t
                k_act = min(LANES, re - lo)
                xs = x[:k_act]
                slot = xs & np.uint64((1 << PB) - 1)
                sym = np.searchsorted(cum[s], slot, side="right") - 1
                xs = f_all[s, sym] * (xs >> np.uint64(PB)) + slot - cum[s, sym]
                need = xs < L
                cnt = int(need.sum())
                if rp + cnt > k:
                    raise ValueError("part ran out of words")
                xs[need] = (xs[need] << np.uint64(16)) | w[rp: rp + cnt]
                rp += cnt
                x[:k_act] = xs
                flat[lo: lo + k_act] = sym
        if rp != k or np.any(x != L):
            raise ValueError("left-over words or wrong final state")
    return flat.reshape(S, n)


def make_case(S, n, N, seed=0):
    """(idx u16 [S, n], freq u16 [S, T]): stream s is a rounded normal of spread SPREADS[s % 4] about a random centre, clipped
    to the table; stream 1 (when there is one) is constant, so that its quantised table gives one symbol nearly all the
    mass; every other stream of three symbols or more holds symbol 0 and symbol T - 1."""
    from vbq_amd.coder import quantize_frequencies
    T = 2 ** (N + 1) - 1
    rng = np.random.default_rng(1000 * S + n + 7 * N + seed)
    idx = np.empty((S, n), np.uint16)
    for s in range(S):
        if s == 1:
            idx[s] = rng.integers(0, T)
            continue
        centre = rng.integers(T // 8, T - T // 8)
        v = np.rint(rng.normal(centre, SPREADS[s % len(SPREADS)], n)).astype(np.int64)
        idx[s] = np.clip(v, 0, T - 1)
        if n >= 3:
            idx[s, n // 3] = 0
            idx[s, (2 * n) // 3] = T - 1
    freq = quantize_frequencies(np.stack([np.bincount(r, minlength=T) for r in idx]))
    return idx, freq


@functools.lru_cache(maxsize=None)
def reference_case(S, n, part, N):
    """(idx, freq, sizes, payload) of one case, computed once per process and shared (read-only arrays)."""
    idx, freq = make_case(S, n, N)
    sizes, payload = encode(idx, freq, part)
    for arr in (idx, freq, sizes, payload):
        arr.setflags(write=False)
    return idx, freq, sizes, payload
