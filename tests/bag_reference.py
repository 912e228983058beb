"""The pooled lookup of include/vbq.h ("Pooled rows") stated a second time, in NumPy float32: a plain loop over bags, entries
and coordinates.  Every operation is one np.float32 operation, which is correctly rounded, so a kernel that follows the
definition agrees with this bit for bit.

    rows      emb f32 [V, K]
    ids       int64 [n]; bag b is the entries offsets[b] .. offsets[b + 1] - 1, in that order
    entries   a negative id is padding (skipped, not counted); an id >= V is skipped, not counted, and sets status bit 3
    sum       acc = +0, then acc = acc + v_k, or acc = acc + (w_i * v_k): two roundings
    mean      the unweighted sum divided by float32(count); count == 0 gives +0
    max       the first counted entry's v_k, replaced only where v_k > acc
    offsets   each bag's range is clamped into [0, n] and begin > end is an empty bag; either sets status bit 4
"""
import numpy as np

BAD_ROW, BAD_OFFSETS = 8, 16
MODES = ("sum", "mean", "max")


def bag(emb, ids, offsets, weights=None, mode="sum"):
    """-> (out f32 [B, K], status)."""
    assert mode in MODES and (weights is None or mode == "sum")
    emb = np.asarray(emb, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    V, K = emb.shape
    n, B = ids.size, offsets.size - 1
    out = np.zeros((B, K), dtype=np.float32)
    status = 0
    for b in range(B):
        begin, end = int(offsets[b]), int(offsets[b + 1])
        if not (0 <= begin <= n and 0 <= end <= n and begin <= end):
            status |= BAD_OFFSETS
            begin, end = min(max(begin, 0), n), min(max(end, 0), n)
            end = max(end, begin)
        acc = [np.float32(0.0)] * K
        count = 0
        for i in range(begin, end):
            r = int(ids[i])
            if r < 0:
                continue
            if r >= V:
                status |= BAD_ROW
                continue
            v = emb[r]
            for k in range(K):
                if mode == "max":
                    if count == 0 or v[k] > acc[k]:
                        acc[k] = v[k]
                elif weights is None:
                    acc[k] = np.float32(acc[k] + v[k])
                else:
                    acc[k] = np.float32(acc[k] + np.float32(np.float32(weights[i]) * v[k]))
            count += 1
        if mode == "mean" and count:
            acc = [np.float32(a / np.float32(count)) for a in acc]
        out[b] = acc
    return out, status


def padded(ids, offsets, pad=-1):
    """The bags of (ids, offsets) as one row each of an int64 [B, L] matrix, filled up with `pad` at the end."""
    ids = np.asarray(ids, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    B = offsets.size - 1
    L = max(1, int(np.diff(offsets).max()) if B else 1)
    out = np.full((B, L), pad, dtype=np.int64)
    for b in range(B):
        out[b, :offsets[b + 1] - offsets[b]] = ids[offsets[b]:offsets[b + 1]]
    return out


def contraction_case():
    """(emb, ids, offsets, weights, want): a weighted sum on which a fused multiply-add and the definition's two roundings
    differ.  With x = 1 + 2^-12 the product x * x = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11 (a tie, to even); added to the
    accumulator -1 that leaves 2^-11, where fma(x, x, -1) keeps the 2^-24."""
    x = np.float32(1.0 + 2.0 ** -12)
    emb = np.array([[1.0], [x]], dtype=np.float32)
    weights = np.array([-1.0, x], dtype=np.float32)
    return emb, np.array([0, 1], np.int64), np.array([0, 2], np.int64), weights, np.float32(2.0 ** -11)
