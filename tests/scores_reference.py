"""The scores of listed rows (include/vbq_ext.h, "Listed rows"; the score of include/vbq.h, "Nearest rows") stated a second time,
exactly: every float32 operation of the definition rounded once, so that a kernel's result is compared bit for bit.

    fma32_exact(a, b, c)         a * b + c as a rational number (fractions.Fraction), rounded once to float32, ties to even
    fma32(a, b, c)               the same for arrays, in float64: the product of two float32 numbers is exact there, TwoSum
                                 gives the error of the sum, the sum is rounded to odd and then to float32 (53 >= 24 + 2 bits:
                                 the second rounding sees what a single one would); tests/test_scores_host.py pins it to
                                 fma32_exact on random and on midpoint cases
    raw_scores(q, v)             acc = fma32(q_k, v_k, acc) over ascending k from +0.0, for pairs of rows q [P, K], v [P, K]
    denominators(v)              1e-8 + sqrt(sum), sum = sum + v_k * v_k over ascending k from 0, every operation in float32
    scores(queries, rows, ids, metric)   f32 [Q, M] and the status word: -inf for a negative id (padding), -inf and bit 3 for
                                 an id >= V
    decode(words, K, N, total_bits, table)   the rows of a record file through tests/records_reference.py; a record the
                                 format does not allow is a row of zeros
Importable without a GPU."""
from fractions import Fraction

import numpy as np

import records_reference as RR

BAD_ROW = 8


def round_to_f32(x, negative_zero=False):
    """The rational x rounded to the nearest float32, ties to even (subnormals kept, overflow to infinity)."""
    x = Fraction(x)
    if x == 0:
        return np.float32(-0.0 if negative_zero else 0.0)
    mag = abs(x)
    e = mag.numerator.bit_length() - mag.denominator.bit_length()
    if Fraction(2) ** e > mag:
        e -= 1
    assert Fraction(2) ** e <= mag < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n = mag / quantum
    r = n.numerator // n.denominator
    rest = n - r
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and r % 2 == 1):
        r += 1
    out = r * quantum
    if out >= Fraction(2) ** 128:
        return np.float32(-np.inf if x < 0 else np.inf)
    return np.float32(float(-out if x < 0 else out))           # exact: 24 bits


def fma32_exact(a, b, c):
    a, b, c = (np.float32(t) for t in (a, b, c))
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    # an exact zero: -0 only when both the product and the addend are -0 (IEEE 754, round to nearest)
    product_negative = bool(np.signbit(a)) != bool(np.signbit(b))
    both_zero = (a == 0 or b == 0) and c == 0
    return round_to_f32(exact, negative_zero=both_zero and product_negative and bool(np.signbit(c)))


def fma32(a, b, c):
    """Arrays of finite float32 -> float32, one rounding."""
    a, b, c = (np.atleast_1d(np.asarray(t, np.float32)).astype(np.float64) for t in (a, b, c))
    p = a * b                                                    # exact: 48 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                              # TwoSum: p + c = s + err exactly
    bits = s.view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0)                         # round to odd: the inexact sum takes its odd neighbour
    step = np.where((err > 0) == (s > 0), 1, -1)
    return np.where(fix, bits + step, bits).view(np.float64).astype(np.float32)


def raw_scores(q, v):
    q, v = np.asarray(q, np.float32), np.asarray(v, np.float32)
    acc = np.zeros(q.shape[0], np.float32)
    for k in range(q.shape[1]):
        acc = fma32(q[:, k], v[:, k], acc)
    return acc


def denominators(v):
    v = np.asarray(v, np.float32)
    total = np.zeros(v.shape[0], np.float32)
    for k in range(v.shape[1]):
        total = total + v[:, k] * v[:, k]                        # float32 arithmetic: each operation rounded once
    assert total.dtype == np.float32
    return np.float32(1e-8) + np.sqrt(total)


def scores(queries, rows, ids, metric):
    """(f32 [Q, M], status) for queries f32 [Q, K] taken as given, rows f32 [V, K], ids int [Q, M]."""
    queries, rows, ids = np.asarray(queries, np.float32), np.asarray(rows, np.float32), np.asarray(ids, np.int64)
    Q, M = ids.shape
    V = rows.shape[0]
    flat = ids.reshape(-1)
    listed = (flat >= 0) & (flat < V)
    out = np.full(Q * M, -np.inf, np.float32)
    if listed.any():
        q = queries[np.repeat(np.arange(Q), M)[listed]]
        v = rows[flat[listed]]
        s = raw_scores(q, v)
        if metric == "cosine":
            with np.errstate(invalid="ignore", divide="ignore"):
                s = s / denominators(v)
        else:
            assert metric == "dot", metric
        assert s.dtype == np.float32
        out[listed] = s
    return out.reshape(Q, M), (BAD_ROW if (flat >= V).any() else 0)


def decode(words, K, N, total_bits, table):
    """f32 [V, K] of the records u32 [V, record_words] and the code points f32 [C, T] in rank order, C = 1 or K."""
    table = np.asarray(table, np.float32)
    out = np.zeros((words.shape[0], K), np.float32)
    for r in range(words.shape[0]):
        try:
            q = RR.unpack(words[r:r + 1], K, N, total_bits)[0]
        except ValueError:
            continue                                             # a damaged record takes part as a row of zeros
        out[r] = table[np.arange(K) if table.shape[0] > 1 else 0, q]
    return out
