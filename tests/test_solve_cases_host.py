"""tests/solve_cases.py without a GPU: at every bit depth the seeded recipes reach the events the fast f32 solve has to flag
(conditions on the data, met by the reference arithmetic alone), and the NumPy restatement that counts them names the same
winners as the C oracle -- level, code point and length of every solve on all the families, raw and caller lengths."""
import numpy as np
import pytest

import solve_cases as SC
from oracle import c_oracle as CO
from oracle import vbq_oracle as O


@pytest.mark.parametrize("N", SC.DEPTHS)
def test_dyadic_case_reaches_cross_level_ties(N):
    case = SC.dyadic_case(N)
    assert np.all(case.mu * 64 == np.round(case.mu * 64)) and np.all(case.tab * 32 == np.round(case.tab * 32))
    assert N < 6 or len(np.unique(case.tab[0])) < case.tab.shape[1]          # duplicates once the grid is finer than 1/32
    ev = SC.events(case)
    print(f"\nN={N} dyadic, raw lengths: {ev}")
    assert ev.solves == 16000
    assert ev.level_differs >= 10, ev
    ev4 = SC.events(case._replace(level_len=SC.dyadic_level_len(N, len(case.lam), 1)))
    print(f"N={N} dyadic, caller lengths: {ev4}")
    assert ev4.level_differs >= 10, ev4


@pytest.mark.parametrize("N", SC.DEPTHS)
def test_near_midpoint_case_merges_the_two_sides(N):
    for n in (N // 2, N):
        case = SC.near_midpoint_case(N, n)
        s = SC.restate(case)
        ev = SC.events(case, s)
        print(f"\nN={N} near mid-points of level {n}: {ev}")
        assert ev.solves == 2000
        assert np.all(s.level == n)                                  # the length table makes level n win
        assert ev.b_merged >= 100, ev
        assert ev.b >= ev.b_merged                                   # the kernel's certificate covers every merged solve
        assert np.all(s.b_flag[s.b_merged])
        assert ev.differs >= 100, ev                                 # ... and without it the answer is R, the reference's L


@pytest.mark.parametrize("N", SC.DEPTHS)
def test_certificate_edge_case_needs_the_certificate_as_wide_as_it_is(N):
    """Rounded costs can merge while dL - dR <= ulp(S) <= 2^-22 S; the kernel flags below 2^-20 S (tested as 2^-19 S on the
    unmasked word).  With the sigmas spread, merged solves sit right up to that bound: a certificate five octaves tighter
    (2^-24) leaves at least ten of them unflagged at every depth, the kernel's own none."""
    missed = merged = 0
    for n in (N // 2, N):
        case = SC.certificate_edge_case(N, n)
        s, tight = SC.restate(case), SC.restate(case, certificate=2.0 ** -24)
        assert np.array_equal(s.level, tight.level) and np.array_equal(s.b_merged, tight.b_merged)
        assert np.all(s.b_flag[s.b_merged])
        merged += int(s.b_merged.sum())
        missed += int((tight.b_merged & ~tight.b_flag).sum())
        print(f"\nN={N} certificate edge at level {n}: {SC.events(case, s)}, unflagged by a 2^-24 certificate "
              f"{int((tight.b_merged & ~tight.b_flag).sum())}")
    assert merged >= 100 and missed >= 10, (merged, missed)


@pytest.mark.parametrize("N", SC.DEPTHS)
@pytest.mark.parametrize("C", [1, 2])
def test_restatement_names_the_c_oracles_winners(N, C):
    lev = O.levels_of_sorted_ranks(N)
    cases = SC.families(N, C=C, rows=301)
    assert [c.name.split("[")[0] for c in cases] == ["dyadic", "near_midpoint", "near_midpoint", "edge", "certificate_edge",
                                                     "certificate_edge"]
    cases += [cases[0]._replace(level_len=SC.dyadic_level_len(N, len(cases[0].lam), C)),
              cases[3]._replace(level_len=SC.edge_level_len(N, len(cases[3].lam), C))]
    for case in cases:
        s = SC.restate(case)
        idx, zh, bt = CO.quantize(case.mu, case.sg, case.tab, case.lam, N=N, level_len=case.level_len, mode=0, want_zhat=True,
                                  want_bits=True, threads=4)
        ctx = f"{case.name} N={N} C={C} lengths={'raw' if case.level_len is None else 'caller'}"
        assert np.array_equal(lev[idx], s.level), ctx
        assert np.array_equal(zh, s.zhat), ctx
        assert np.array_equal(bt, s.bits), ctx
        # the index is the rank of the winner in the channel's sorted table: it addresses the winner's value
        srt = np.sort(case.tab, axis=1)
        for c in range(C):
            assert np.array_equal(srt[c][idx[:, :, c]], zh[:, :, c]), ctx


def test_second_channel_repeats_the_first_ones_events():
    for case in (SC.dyadic_case(7, rows=500, C=2), SC.near_midpoint_case(9, 4, rows=500, C=2)._replace(level_len=None)):
        s = SC.restate(case)
        for f in ("level", "side", "multi", "b_flag", "b_merged", "unflagged_level"):
            a = getattr(s, f)
            assert np.array_equal(a[:, :, 0], a[:, :, 1]), f
        assert np.array_equal(s.zhat[:, :, 1], np.float32(2) * s.zhat[:, :, 0])
