"""Frequency tables that do NOT fit the data they code, and data drawn without looking at them -- for the rANS coder tests.

Everywhere else in the suite a table is the quantised histogram of the very stream it codes.  The library is not used that way:
build_entropy_models fits the tables on validation images and compress* codes other images with them, so a latent outside the
fitted distribution is coded almost entirely with symbols of frequency 1 (15 bits each).  The tables here are made by hand, for
T = 2^(N+1) - 1 symbols, as uint16 rows summing to 2^15:

  spike(N, at)    f[at] = 2^15 - (T - 1), every other entry 1 (N = 1 gives f = 32766, the largest divisor a table without zeros has)
  half_ones(N)    the first T // 2 symbols have frequency 1, the rest share the remainder as evenly as integers allow: buckets
                  of 16 one-slot symbols next to wide ranges
  ramp()          N = 7 only: f[i] = i + 1 (sum 32640) plus 128 on the last entry: every divisor 1 .. 254, and 383
  zero_tables(N)  two entries hold all the mass, every other entry is 0 -- only for the entry points whose text in include/vbq.h
                  admits zeros: (1, 0.., 32767), (32767, 1, 0..), (16384, 0.., 16384)

and the data, per table and over its symbols with f > 0 (DATA_KINDS): uniform, only the rarest symbols, only the most frequent
symbol, alternating most frequent / rare, and -- the control -- drawn from the table itself.  Seeds are fixed.

encoder_trace is a plain restatement of the segment encoder's loop (include/vbq.h, vbq_rans_encode_u16) that reports what the
state reaches before a push; the host test uses it to prove that the cases come close to the limit x < f 2^17 the kernels'
division is written for.  No GPU and nothing of the package is needed here.
"""
import functools

import numpy as np

PB = 15
M = 1 << PB
L = 1 << 16
DATA_KINDS = ("uniform", "rare", "frequent", "alternating", "table")
BIT_DEPTHS = (1, 4, 7, 10)                                       # 7 is where the ramp lives


def table_size(N):
    return 2 ** (N + 1) - 1


def spike(N, at):
    T = table_size(N)
    f = np.ones(T, np.int64)
    f[at] = M - (T - 1)
    return _row(f)


def half_ones(N):
    T = table_size(N)
    f = np.ones(T, np.int64)
    rest = T - T // 2
    left = M - T // 2
    f[T // 2:] = left // rest
    f[T // 2: T // 2 + left % rest] += 1
    return _row(f)


def ramp():
    f = np.arange(1, table_size(7) + 1, dtype=np.int64)
    f[-1] += 128
    return _row(f)


def zero_tables(N):
    """name -> row with zeros: two symbols hold all the mass."""
    T = table_size(N)
    out = {}
    for name, (a, fa, b, fb) in (("zero-1-32767", (0, 1, T - 1, M - 1)), ("zero-32767-1", (0, M - 1, 1, 1)),
                                 ("zero-halves", (0, M // 2, T - 1, M // 2))):
        f = np.zeros(T, np.int64)
        f[a], f[b] = fa, fb
        out[name] = _row(f)
    return out


def _row(f):
    assert int(f.sum()) == M and f.min() >= 0 and f.max() < M
    return f.astype(np.uint16)


def tables(N, zero=False):
    """name -> row: the families of bit depth N, every entry >= 1; with zero=True the zero-entry tables as well."""
    T = table_size(N)
    out = {"spike-first": spike(N, 0), "spike-mid": spike(N, T // 2), "spike-last": spike(N, T - 1), "half-ones": half_ones(N)}
    if N == 7:
        out["ramp"] = ramp()
    if zero:
        out.update(zero_tables(N))
    return out


def draw(freq, kind, n, rng):
    """n symbols u16 over the symbols of the row with f > 0, of one DATA_KINDS kind."""
    f = np.asarray(freq).astype(np.int64)
    used = np.flatnonzero(f)
    rare = used[f[used] == f[used].min()]
    top = int(np.argmax(f))
    if kind == "uniform":
        out = rng.choice(used, n)
    elif kind == "rare":
        out = rng.choice(rare, n)
    elif kind == "frequent":
        out = np.full(n, top)
    elif kind == "alternating":
        out = np.where(np.arange(n) % 2 == 0, top, rng.choice(rare, n))
    elif kind == "table":
        out = np.searchsorted(np.cumsum(f), rng.integers(0, M, n), side="right")
    else:
        raise ValueError(kind)
    assert np.all(f[out] > 0)
    return out.astype(np.uint16)


@functools.lru_cache(maxsize=None)
def streams(N, n, zero=False, seed=0):
    """(names, idx u16 [S, n], freq u16 [S, T]): one stream per (table, data kind) of bit depth N, computed once per process
    and shared read-only.  names[s] = (table name, data kind)."""
    rng = np.random.default_rng(10007 * N + 31 * n + seed)
    names, idx, freq = [], [], []
    for tname, row in tables(N, zero).items():
        for kind in DATA_KINDS:
            names.append((tname, kind))
            idx.append(draw(row, kind, n, rng))
            freq.append(row)
    idx, freq = np.stack(idx), np.stack(freq)
    idx.setflags(write=False)
    freq.setflags(write=False)
    return tuple(names), idx, freq


def pick(names, table=None, kind=None):
    """The stream numbers whose table name starts with `table` and whose data kind is `kind` (None: any)."""
    return [s for s, (t, k) in enumerate(names) if (table is None or t.startswith(table)) and (kind is None or k == kind)]


def rare_stream(N, n, seed=0):
    """(idx u16 [1, n], freq u16 [1, T]): one stream of only frequency-1 symbols under spike(N, T // 2)."""
    row = spike(N, table_size(N) // 2)
    return draw(row, "rare", n, np.random.default_rng(977 * N + n + seed))[None], row[None]


def mixed_model(n_tables, C_, N, seed=0):
    """Tables and draws for the batch and window kernels' case classes, in place of their fitted ones: -> (freq u16
    [n_tables, C_, T], draw(t, n) -> u16 [C_, n]).  The rows cycle through a spike, the ramp (N = 7; another spike otherwise),
    half_ones and a spike in the middle across (table, channel), so that with three tables every file's first channel has
    another family.  Every file of table 0 is all-rare data: each of its streams is coded at 15 bits per symbol; the data kinds
    of the other tables cycle with a period of their own."""
    T = table_size(N)
    rows = [spike(N, 0), ramp() if N == 7 else spike(N, T - 1), half_ones(N), spike(N, T // 2)]
    rng = np.random.default_rng(4241 + 17 * n_tables + C_ + 7 * N + seed)
    freq = np.stack([[rows[(t + c) % len(rows)] for c in range(C_)] for t in range(n_tables)])
    kinds = [["rare" if t == 0 else DATA_KINDS[(2 * t + c) % len(DATA_KINDS)] for c in range(C_)] for t in range(n_tables)]

    def draw_file(t, n):
        return np.stack([draw(freq[t, c], kinds[t][c], n, rng) for c in range(C_)])
    return freq, draw_file


def mapped_rows(P, S, N):
    """freq u16 [P, S, T]: every class's row of every stream from another family."""
    rows = list(tables(N).values())
    return np.stack([[rows[(p + s) % len(rows)] for s in range(S)] for p in range(P)])


def mapped_planes(freq, n, seed=0):
    """planes u16 [P, S, n] for freq [P, S, T]: the data kinds cycle over (class, stream)."""
    P, S, T = freq.shape
    rng = np.random.default_rng(7919 * P + 13 * S + n + T + seed)
    return np.stack([[draw(freq[p, s], DATA_KINDS[(p + 2 * s) % len(DATA_KINDS)], n, rng) for s in range(S)] for p in range(P)])


def encoder_trace(idx_row, freq_row, seg):
    """The segment encoder's loop, restated: -> (sizes [nseg], the largest state before a push, the largest x / (f << 17)
    before a push).  The state before a push is the renormalised one: what the kernels divide by f."""
    f_all = [int(v) for v in np.asarray(freq_row)]
    c_all = [0]
    for v in f_all:
        c_all.append(c_all[-1] + v)
    row = [int(v) for v in np.asarray(idx_row)]
    n = len(row)
    sizes, x_max, ratio = [], 0, 0.0
    for a in range(0, n, seg):
        x, k = L, 0
        for i in range(min(n, a + seg) - 1, a - 1, -1):
            f, c = f_all[row[i]], c_all[row[i]]
            if x >= f << 17:
                k += 1
                x >>= 16
            assert 2 * f <= x < f << 17
            x_max = max(x_max, x)
            ratio = max(ratio, x / (f << 17))
            x = (x // f << PB) + x % f + c
        sizes.append(k + 2)
    return sizes, x_max, ratio


# ---- the cases of the kernel tests; tests/test_adversarial_tables_host.py proves on the references what they reach
SEGMENT_SHAPES = [(1003, 64), (1024, 64), (520, 8)]              # (n, seg): the 2-byte paths, the 16-byte paths, a second workgroup
LARGEST_SEGMENT = (65538, 65533)                                 # one all-rare stream: the largest segment, then one of 5 symbols
IL_SHAPES = [(130, 64), (1000, 1000), (4096, 1024)]              # (n, part) over the streams of `streams`
IL_CROSSING = (130, 200)                                         # parts that end inside streams: runs of other rows in one part
MAPPED_S, MAPPED_SEG = 3, 64
MAPPED_MAPS = ("per-symbol", "blocks-of-8")


def class_map(name, P, n):
    """per-symbol: a change at every symbol (the kernels' scalar path); blocks-of-8: constant over every aligned group of eight
    (their vector path)."""
    i = np.arange(n)
    return ((i if name == "per-symbol" else i // 8) % P).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def mapped_case(P, n, N, name):
    """(planes [P, S, n], freq [P, S, T], cls [n], selected idx [S, n], words, sizes) by tests/mapped_reference.py, once per
    process, read-only."""
    import mapped_reference as MR
    freq = mapped_rows(P, MAPPED_S, N)
    planes = mapped_planes(freq, n)
    cls = class_map(name, P, n)
    idx = MR.select(planes, cls)
    words, sizes = MR.encode(idx, cls, freq, MAPPED_SEG)
    for a in (planes, freq, cls, idx, words, sizes):
        a.setflags(write=False)
    return planes, freq, cls, idx, words, sizes
