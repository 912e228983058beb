"""The record format of vbq_amd/bitstream.py (magic b"VBQr") stated a second time, in NumPy, from its specification alone: one
explicit array of bits per record, no word arithmetic shared with the kernels.

A code point of bit length n has rank index q; with k = q + 1: n = N - ctz(k), code j = k >> (N - n + 1), and back
q = ((2 j + 1) << (N - n)) - 1.  W = N.bit_length().  Bit i of a record is bit i % 32 of little-endian u32 word i / 32:
lengths at [k W, (k+1) W), then the codes back to back from bit K W, each least significant bit first, then zero padding up to
ceil((K W + total_bits) / 32) words.
"""
import numpy as np


def record_words(K, N, total_bits):
    return (K * N.bit_length() + total_bits + 31) // 32


def length_and_code(q, N):
    """(n, j) of the rank indices q (any integer array)."""
    k = np.asarray(q, dtype=np.int64) + 1
    ctz = np.zeros_like(k)
    for b in range(N + 1):                                   # the number of trailing zero bits of k
        ctz += ((k & ((1 << (b + 1)) - 1)) == 0)
    n = N - ctz
    return n, k >> (N - n + 1)


def rank_of(n, j, N):
    return ((2 * np.asarray(j, dtype=np.int64) + 1) << (N - np.asarray(n, dtype=np.int64))) - 1


def _bits(value, width):
    return [(int(value) >> b) & 1 for b in range(width)]


def pack(idx, N, total_bits):
    """Rank indices [R, K] -> u32 [R, record_words].  Every row's lengths must add up to total_bits."""
    idx = np.asarray(idx)
    R, K = idx.shape
    W, RW = N.bit_length(), record_words(K, N, total_bits)
    out = np.zeros((R, RW), dtype="<u4")
    for r in range(R):
        n, j = length_and_code(idx[r], N)
        assert int(n.sum()) == total_bits, (r, int(n.sum()), total_bits)
        bits = []
        for k in range(K):
            bits += _bits(n[k], W)
        for k in range(K):
            bits += _bits(j[k], int(n[k]))
        bits += [0] * (32 * RW - len(bits))
        out[r] = np.packbits(np.array(bits, dtype=np.uint8), bitorder="little").view("<u4")
    return out


def unpack(words, K, N, total_bits):
    """u32 [R, record_words] -> rank indices int64 [R, K].  ValueError for a record the format does not allow."""
    words = np.ascontiguousarray(words, dtype="<u4")
    R, RW = words.shape
    W = N.bit_length()
    assert RW == record_words(K, N, total_bits)
    out = np.zeros((R, K), dtype=np.int64)
    for r in range(R):
        bits = np.unpackbits(words[r].view(np.uint8), bitorder="little").astype(np.int64)

        def take(pos, width):
            return int(sum(int(bits[pos + b]) << b for b in range(width)))
        n = [take(k * W, W) for k in range(K)]
        if max(n) > N:
            raise ValueError(f"record {r}: a length above N")
        if sum(n) != total_bits:
            raise ValueError(f"record {r}: lengths add up to {sum(n)}, not {total_bits}")
        if bits[K * W + total_bits:].any():
            raise ValueError(f"record {r}: non-zero padding")
        pos = K * W
        for k in range(K):
            out[r, k] = rank_of(n[k], take(pos, n[k]), N)
            pos += n[k]
    return out


def random_indices(rng, R, K, N, total_bits):
    """Rank indices [R, K] (uint16) with random lengths per row that add up to total_bits (each <= N) and random codes."""
    assert 0 <= total_bits <= K * N
    idx = np.zeros((R, K), dtype=np.uint16)
    for r in range(R):
        slots = np.repeat(np.arange(K), N)                   # N one-bit slots per coordinate: a random total_bits of them
        n = np.bincount(rng.permutation(slots)[:total_bits], minlength=K).astype(np.int64)
        j =rng.integers(0, 1 << 62, size=K) & ((1 << n) - 1)
        idx[r] = rank_of(n, j, N)
    return idx
