"""The mismatched-table cases of tests/adversarial_tables.py on the host: proof, from the references alone (the C checker,
tests/interleaved_reference.py, tests/mapped_reference.py and a plain restatement of the encoder's loop), that the cases
reach what tests/test_gpu_adversarial_tables.py relies on -- segments of the smallest and (nearly) the largest size, parts in
which about 60 of 64 lanes take a word at every step, and encoder states close to the limit f 2^17 of the kernels' division, at
the divisors 32766 and 32767.  Each test prints the figures it asserts (pytest -s)."""
import numpy as np
import pytest

import adversarial_tables as AT
import interleaved_reference as IR
import mapped_reference as MR
from oracle import c_oracle as CO


def test_tables_are_what_they_claim():
    for N in AT.BIT_DEPTHS:
        T = AT.table_size(N)
        for name, row in AT.tables(N, zero=True).items():
            assert row.dtype == np.uint16 and row.shape == (T,) and int(row.astype(np.int64).sum()) == 1 << 15, (N, name)
            assert (int(row.min()) == 0) == name.startswith("zero"), (N, name)
        for at in (0, T // 2, T - 1):
            f = AT.spike(N, at)
            assert f[at] == (1 << 15) - (T - 1) and np.all(np.delete(f, at) == 1)
        h = AT.half_ones(N).astype(np.int64)
        assert np.all(h[: T // 2] == 1) and h[T // 2:].max() - h[T // 2:].min() <= 1 and h[T // 2:].min() >= 16
        z = AT.zero_tables(N)
        assert (z["zero-1-32767"][0], z["zero-1-32767"][T - 1]) == (1, 32767) and np.count_nonzero(z["zero-1-32767"]) == 2
        assert (z["zero-32767-1"][0], z["zero-32767-1"][1]) == (32767, 1) and np.count_nonzero(z["zero-32767-1"]) == 2
        assert (z["zero-halves"][0], z["zero-halves"][T - 1]) == (16384, 16384) and np.count_nonzero(z["zero-halves"]) == 2
    assert AT.spike(1, 0)[0] == 32766
    r = AT.ramp().astype(np.int64)
    assert np.array_equal(r[:254], np.arange(1, 255)) and r[254] == 383
    # the data is drawn without a look at the table's shape: all five kinds per table, over its symbols with f > 0
    names, idx, freq = AT.streams(7, 1003, zero=True)
    assert len(names) == 5 * 8 and idx.shape == (40, 1003)
    for s, (tname, kind) in enumerate(names):
        f = freq[s].astype(np.int64)
        assert np.all(f[idx[s]] > 0)
        if kind == "rare":
            assert np.all(f[idx[s]] == f[f > 0].min())
        if kind == "frequent":
            assert np.all(f[idx[s]] == f.max())
        if kind == "alternating":
            assert np.all(f[idx[s, 0::2]] == f.max()) and np.all(f[idx[s, 1::2]] == f[f > 0].min())


@pytest.mark.parametrize("N", AT.BIT_DEPTHS)
def test_checker_round_trip_and_segment_sizes(N):
    smallest, largest = None, 0
    for n, seg in AT.SEGMENT_SHAPES:
        names, idx, freq = AT.streams(N, n, zero=True)
        words, sizes = CO.rans_encode(idx, freq, seg)
        assert np.array_equal(CO.rans_decode(words, sizes, freq, n, seg), idx)
        lens = np.minimum(seg, n - seg * np.arange(sizes.shape[1]))
        assert np.all(sizes >= 2) and np.all(sizes <= lens + 2)
        spikes = AT.pick(names, "spike", "frequent")
        assert len(spikes) == 3 and np.all(sizes[spikes] == 2)   # the all-spike data: two words at every length <= 64
        rare = AT.pick(names, "spike", "rare") + AT.pick(names, "half-ones", "rare")
        assert np.all(sizes[rare] >= 2 + (15 * lens) // 16)
        smallest = int(sizes.min()) if smallest is None else min(smallest, int(sizes.min()))
        largest = max(largest, int((sizes.astype(np.int64) - lens).max()))
    assert smallest == 2
    print(f"N={N}: smallest segment 2 words; largest size - len = {largest} (bound 2)")


@pytest.mark.parametrize("N", [1, 3, 10])
def test_all_rare_segments_come_close_to_their_capacity(N):
    got = []
    for m in (7, 64, 1024):
        idx, freq = AT.rare_stream(N, m)
        assert np.all(freq[0][idx[0]] == 1)
        words, sizes = CO.rans_encode(idx, freq, m)
        assert np.array_equal(CO.rans_decode(words, sizes, freq, m, m), idx)
        assert 2 + (15 * m) // 16 <= int(sizes[0, 0]) <= m + 2
        got.append(int(sizes[0, 0]))
    print(f"N={N}: all-rare segments of 7, 64, 1024 symbols take {got} words (capacity 9, 66, 1026)")
    assert got == [8, 62, 962]                                   # 15 bits a symbol on top of the 16 of the start state


def test_the_largest_segment():
    n, seg = AT.LARGEST_SEGMENT
    idx, freq = AT.rare_stream(10, n)
    words, sizes = CO.rans_encode(idx, freq, seg)
    assert np.array_equal(CO.rans_decode(words, sizes, freq, n, seg), idx)
    assert sizes.shape == (1, 2) and 2 + (15 * seg) // 16 <= int(sizes[0, 0]) <= seg + 2 and int(sizes[0, 0]) < 1 << 16
    print(f"the segment of {seg} symbols takes {int(sizes[0, 0])} words (capacity {seg + 2}, u16 size field 65535)")


@pytest.mark.parametrize("N", AT.BIT_DEPTHS)
def test_interleaved_round_trip_and_part_sizes(N):
    for n, part in AT.IL_SHAPES + [AT.IL_CROSSING]:
        names, idx, freq = AT.streams(N, n)
        S = len(names)
        sizes, payload = IR.encode(idx, freq, part)
        assert np.array_equal(IR.decode(sizes, payload, freq, n, part), idx)
        m = np.minimum(part, S * n - part * np.arange(sizes.size))
        assert np.all(sizes >= 128) and np.all(sizes <= m + 128)
        first = np.arange(sizes.size) * part                     # parts that lie inside one stream
        inside = first // n == (first + m - 1) // n
        stream = first // n
        spike = np.isin(stream, AT.pick(names, "spike", "frequent")) & inside
        rare = np.isin(stream, AT.pick(names, None, "rare")) & inside
        if (n, part) != AT.IL_CROSSING:
            assert spike.any() and np.all(sizes[spike] == 128)
            assert rare.any()
        if part >= 1000:
            assert np.all(sizes[rare] >= 128 + 0.9 * m[rare])    # about 60 of 64 lanes take a word at every step
            print(f"N={N} n={n} part={part}: all-rare parts of {sorted(set(int(v) for v in m[rare]))} symbols take "
                  f"{sorted(set(int(v) for v in sizes[rare]))} words (capacity m + 128)")
    # the crossing case: some part holds the end of an all-rare stream and the start of the all-spike stream after it
    n, part = AT.IL_CROSSING
    names, _, _ = AT.streams(N, n)
    r = AT.pick(names, "spike-first", "rare")[0]
    assert names[r + 1] == ("spike-first", "frequent")
    boundary = (r + 1) * n
    assert (boundary - 1) // part == boundary // part            # both sides of the boundary lie in one part
    start = max(r * n, boundary // part * part)
    assert (boundary - start) % 64 != 0                          # the all-rare run ends in mid-step


def test_the_encoder_state_comes_close_to_its_limit():
    """The largest state before a push over the cases, and the largest x / (f << 17): the division of the kernels is written
    for x < f 2^17 and estimates the quotient in float."""
    best, at = 0, None
    for N in AT.BIT_DEPTHS:
        n, seg = AT.SEGMENT_SHAPES[0]
        names, idx, freq = AT.streams(N, n)
        ref = CO.rans_encode(idx, freq, seg)[1]
        for s, name in enumerate(names):
            sizes, x_max, _ = AT.encoder_trace(idx[s], freq[s], seg)
            assert sizes == ref[s].tolist()                      # the restatement is the checker's encoder
            if x_max > best:
                best, at = x_max, (N,) + name
    print(f"largest state before a push: {best:#x} at N, table, data = {at}")
    assert best >= 0xC0000000
    ratio, x_top = 0.0, 0
    for N in AT.BIT_DEPTHS:
        for n, seg in AT.SEGMENT_SHAPES[:2]:
            names, idx, freq = AT.streams(N, n, zero=True)
            for s in AT.pick(names, "zero-32767-1"):
                _, x_max, r = AT.encoder_trace(idx[s], freq[s], seg)
                ratio, x_top = max(ratio, r), max(x_top, x_max)
    print(f"table (32767, 1, 0 ..): largest x / (f << 17) = {ratio:.6f}, largest state {x_top:#x}")
    assert ratio > 0.999


@pytest.mark.parametrize("N", AT.BIT_DEPTHS)
@pytest.mark.parametrize("P", [2, 4])
def test_mapped_reference_round_trip(P, N):
    for n in (1003, 1024):
        for name in AT.MAPPED_MAPS:
            planes, freq, cls, idx, words, sizes = AT.mapped_case(P, n, N, name)
            assert len({freq[p, 0].tobytes() for p in range(P)}) == P         # every class's row from another family
            assert set(cls.tolist()) == set(range(P))
            if name == "blocks-of-8":
                assert np.all(cls[: n // 8 * 8].reshape(-1, 8) == cls[: n // 8 * 8: 8, None])
            back, status = MR.decode(words, sizes, cls, freq, n, AT.MAPPED_SEG)
            assert status == 0 and np.array_equal(back, idx)
            lens = np.minimum(AT.MAPPED_SEG, n - AT.MAPPED_SEG * np.arange(sizes.shape[1]))
            assert np.all(sizes >= 2) and np.all(sizes <= lens + 2)
    # a uniform map is the plain coder with that class's rows
    planes, freq, _, _, _, _ = AT.mapped_case(P, 1003, N, "per-symbol")
    for p in range(P):
        w, s = MR.encode(planes[p], np.full(1003, p, np.uint8), freq, AT.MAPPED_SEG)
        w_ref, s_ref = CO.rans_encode(planes[p], freq[p], AT.MAPPED_SEG)
        assert np.array_equal(s, s_ref) and np.array_equal(w, w_ref)
