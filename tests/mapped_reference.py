"""Plain NumPy / Python coder for the class-mapped segment layout (the payload of a VBQm file) and the file's 2-bit class block.

Written from the format's text (include/vbq.h, "Class-mapped rANS" and the VBQm layout under it), not from the kernels; the
GPU tests compare the kernels' sizes, words and decoded indices with it.  Restated:

  * 32-bit state, start state 2^16, 16-bit words, 15 probability bits; c = exclusive cumulative frequency.
  * Every stream of n symbols is cut into segments of `seg` symbols, each coded on its own, last symbol to first.  Symbol i of
    stream s has class cls[i] and uses the table freq[cls[i]][s].
  * Encoder, per symbol: when x >= f << 17, emit x & 0xffff and x >>= 16; then x = (x // f << 15) + x % f + c.  After the
    first symbol of the segment the state goes out low half, then high half.  A segment of m symbols takes 2 .. m + 2 words.
  * Decoder: the state from the last two words, then words backwards.  Per symbol: slot = x & 32767, the symbol is the one with
    c <= slot < c + f, x = f (x >> 15) + slot - c; while x < 2^16 and a word is left: x = x << 16 | word.  At the end no word
    is left and x == 2^16.
  * Status bits of the decoder: 1 a size outside [2, seg + 2]; 2 a segment ran out of words (zeros from there on); 4 words left
    over or a wrong final state; 8 a table of the stream that does not sum to 2^15; 64 a class >= P in the segment.  Segments
    with 1, 8 or 64 decode to zeros.
  * Class block of the file: 2 bits per position, position b in byte b // 4 at bits 2 (b % 4), zero-padded to 8 bytes.
"""
import functools

import numpy as np

PB = 15
L = 1 << 16
MASK = (1 << PB) - 1


def _cum(freq):
    f = np.asarray(freq).astype(np.int64)
    return f, np.cumsum(f, axis=-1) - f


def select(planes, cls):
    """planes [P, S, n], cls [n] -> [S, n]: symbol i of stream s is planes[cls[i], s, i]."""
    planes = np.asarray(planes)
    return planes[np.asarray(cls).astype(np.int64), :, np.arange(planes.shape[2])].T.copy()


def encode(idx, cls, freq, seg):
    """idx [S, n] (already selected), cls [n], freq [P, S, T] -> (words u16 [S, nseg, seg + 2], zero beyond each size,
    sizes u32 [S, nseg])."""
    idx = np.asarray(idx)
    S, n = idx.shape
    f_all, c_all = _cum(freq)
    cls = [int(c) for c in np.asarray(cls)]
    nseg = (n + seg - 1) // seg
    words = np.zeros((S, nseg, seg + 2), dtype=np.uint16)
    sizes = np.zeros((S, nseg), dtype=np.uint32)
    for s in range(S):
        row = [int(v) for v in idx[s]]
        for g in range(nseg):
            x, out = L, []
            for i in range(min(n, (g + 1) * seg) - 1, g * seg - 1, -1):
                f, c = int(f_all[cls[i], s, row[i]]), int(c_all[cls[i], s, row[i]])
                if x >= f << 17:
                    out.append(x & 0xffff)
                    x >>= 16
                x = (x // f << PB) + x % f + c
            out += [x & 0xffff, x >> 16]
            words[s, g, : len(out)] = out
            sizes[s, g] = len(out)
    return words, sizes


def sizes(idx, cls, freq, seg):
    return encode(idx, cls, freq, seg)[1]


def decode(words, sizes, cls, freq, n, seg):
    """-> (idx u16 [S, n], status): the OR of the status bits over all segments."""
    f_all = np.asarray(freq).astype(np.int64)
    P, S, T = f_all.shape
    cum = np.concatenate([np.zeros((P, S, 1), np.int64), np.cumsum(f_all, axis=2)], axis=2)      # [P, S, T + 1]
    cls = [int(c) for c in np.asarray(cls)]
    nseg = (n + seg - 1) // seg
    idx = np.zeros((S, n), dtype=np.uint16)
    status = 0
    for s in range(S):
        tables_ok = all(int(cum[p, s, T]) == 1 << PB for p in range(P))
        for g in range(nseg):
            a, b = g * seg, min(n, (g + 1) * seg)
            k = int(sizes[s, g])
            bad = 0 if tables_ok else 8
            if not 2 <= k <= seg + 2:
                bad |= 1
            if any(c >= P for c in cls[a:b]):
                bad |= 64
            if bad:
                status |= bad
                continue
            w = [int(v) for v in words[s, g, :k]]
            x = w[k - 1] << 16 | w[k - 2]
            k -= 2
            for i in range(a, b):
                p = cls[i]
                slot = x & MASK
                sym = int(np.searchsorted(cum[p, s], slot, side="right")) - 1
                x = int(f_all[p, s, sym]) * (x >> PB) + slot - int(cum[p, s, sym])
                idx[s, i] = sym
                if x < L:
                    if k == 0:
                        bad |= 2
                        break
                    k -= 1
                    x = x << 16 | w[k]
            if not bad and (k != 0 or x != L):
                bad |= 4
            status |= bad
    return idx, status


def pack_classes(cls):
    """cls [B] in [0, 4) -> the class block (bytes), zero-padded to a multiple of 8 bytes."""
    out = bytearray(8 * ((len(cls) + 31) // 32))
    for b, c in enumerate(cls):
        out[b // 4] |= int(c) << 2 * (b % 4)
    return bytes(out)


def unpack_classes(block, B):
    return np.array([(block[b // 4] >> 2 * (b % 4)) & 3 for b in range(B)], dtype=np.uint8)


# ---- the cases of the kernel tests: S = 3 streams in segments of 64 symbols
S, SEG = 3, 64


def maps(P, n):
    """name -> class map u8 [n] for a palette of P classes."""
    out = {f"uniform{p}": np.full(n, p, np.uint8) for p in range(P)}
    mid = np.zeros(n, np.uint8)
    mid[SEG + SEG // 2 + 3:] = P - 1                             # a change in the middle of segment 1
    out["mid"] = mid
    out["checker"] = (np.arange(n) % P).astype(np.uint8)         # a change at every symbol
    if P == 3:
        out["skip1"] = np.where(np.arange(n) // 5 % 2 == 0, 0, 2).astype(np.uint8)    # class 1 never used
    return out


def make_planes(P, n, N, seed=0):
    """(planes u16 [P, S, n], freq u16 [P, S, T]): rounded normals of different spreads about random centres, clipped to the
    table, with symbol 0 and symbol T - 1 present; the tables are the quantised histograms of the planes."""
    from vbq_amd.coder import quantize_frequencies
    T = 2 ** (N + 1) - 1
    rng = np.random.default_rng(100 * P + n + 7 * N + seed)
    spreads = [0.3, 2.0, 25.0, 300.0]
    planes = np.empty((P, S, n), np.uint16)
    for p in range(P):
        for s in range(S):
            centre = rng.integers(T // 8, T - T // 8)
            v = np.rint(rng.normal(centre, spreads[(p + s) % 4] * T / 2047, n)).astype(np.int64)
            planes[p, s] = np.clip(v, 0, T - 1)
            planes[p, s, n // 3] = 0
            planes[p, s, (2 * n) // 3] = T - 1
    freq = quantize_frequencies(np.stack([[np.bincount(r, minlength=T) for r in pl] for pl in planes]))
    return planes, freq


@functools.lru_cache(maxsize=None)
def reference_case(P, n, N, name):
    """(planes, freq, cls, selected idx, words, sizes) of one case, computed once per process and shared (read-only)."""
    planes, freq = make_planes(P, n, N)
    cls = maps(P, n)[name]
    idx = select(planes, cls)
    words, szs = encode(idx, cls, freq, SEG)
    for arr in (planes, freq, cls, idx, words, szs):
        arr.setflags(write=False)
    return planes, freq, cls, idx, words, szs
