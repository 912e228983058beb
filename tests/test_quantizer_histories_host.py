"""tests/quantizer_histories.py against the class it probes, without a GPU.

Coverage: every public callable of ChannelwisePriorCDFQuantizer is in exactly one of PROBED and EXEMPT, every name in either
exists, every probe PROBED names exists and really calls the method, and EXEMPT holds only the reasons the closed set allows.
Recipes: they are deterministic, E and E2 are non-strict tables and the others strict (through the rank_of_slot ordering
build_code_points uses), Lsub's lambdas relate to A's as described, every class map uses every class of its palette, and a
budget taken between two rungs selects the rung it was meant to."""
import inspect

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import quantizer_histories as QH  # noqa: E402


def _cls():
    from vbq_amd import ChannelwisePriorCDFQuantizer
    return ChannelwisePriorCDFQuantizer


def test_every_public_method_is_probed_or_exempt():
    methods = QH.public_methods(_cls())
    both = sorted(set(QH.PROBED) & set(QH.EXEMPT))
    assert not both, f"in PROBED and in EXEMPT of tests/quantizer_histories.py: {both}"
    missing = [m for m in methods if m not in QH.PROBED and m not in QH.EXEMPT]
    assert not missing, (f"public methods of ChannelwisePriorCDFQuantizer without an entry: {missing}.  Add each to PROBED of "
                         "tests/quantizer_histories.py with a probe that calls it (a method that reads cached state), or to "
                         "EXEMPT with one of EXEMPT_REASONS")
    gone = [m for m in list(QH.PROBED) + list(QH.EXEMPT) if m not in methods]
    assert not gone, f"PROBED / EXEMPT of tests/quantizer_histories.py name methods the class does not have: {gone}"


def test_probed_names_probes_that_call_the_method():
    used = set()
    for method, probes in QH.PROBED.items():
        assert probes, f"PROBED[{method!r}] names no probe"
        for name in probes:
            assert name in QH.PROBES, f"PROBED[{method!r}] names the probe {name!r}, which PROBES does not have"
            src = inspect.getsource(QH.PROBES[name])
            assert f"q.{method}(" in src, f"the probe {name!r} does not call q.{method}"
            used.add(name)
    unused = sorted(set(QH.PROBES) - used)
    assert not unused, f"probes no entry of PROBED names: {unused}"


def test_exempt_holds_only_the_allowed_reasons():
    methods = set(QH.public_methods(_cls()))
    for method, reason in QH.EXEMPT.items():
        assert reason.startswith(QH.EXEMPT_REASONS), f"EXEMPT[{method!r}] = {reason!r}: not one of EXEMPT_REASONS"
        if reason.startswith(QH.WRAPPER):
            target = reason[len(QH.WRAPPER):]
            assert target in methods and (target in QH.PROBED or QH.EXEMPT.get(target) == QH.TRANSITION), \
                f"EXEMPT[{method!r}] names {target!r}, which is neither probed nor a transition"
            src = inspect.getsource(getattr(_cls(), method))
            assert f"self.{target}(" in src and ("vae.encode(" in src or "self._encode(X, vae)" in src), f"{method} is no wrapper of {target}"


def test_every_transition_has_a_failed_attempt_and_every_attempt_a_method():
    methods = set(QH.public_methods(_cls()))
    attempted = {}
    for name, (fn, exc) in QH.FAILED_ATTEMPTS.items():
        method, sep, what = name.partition(":")
        assert sep and what and method in methods, f"FAILED_ATTEMPTS[{name!r}] names no public method of the class"
        assert callable(fn) and (isinstance(exc, str) or (isinstance(exc, type) and issubclass(exc, Exception))), name
        assert not isinstance(exc, str) or isinstance(QH.expected_type(exc), type), name
        attempted.setdefault(method, []).append(what)
    transitions = sorted(m for m, reason in QH.EXEMPT.items() if reason == QH.TRANSITION)
    assert transitions == ["build_code_points", "build_entropy_models_from_latents", "load", "save"]
    missing = [m for m in transitions if m not in attempted]
    assert not missing, f"transitions without a failed attempt in FAILED_ATTEMPTS of tests/quantizer_histories.py: {missing}"
    # the families the harness is held to: every budget call, every reader twice, every batch writer
    budget = sorted(m for m in QH.PROBED if "_budget" in m)
    assert len(budget) == 8 and all(any(w.startswith("no_rung_fits") for w in attempted.get(m, [])) for m in budget), budget
    for reader in QH.READERS:
        (method,) = [m for m, ps in QH.PROBED.items() if reader in ps]
        assert {f"damaged_file_{reader}", f"file_of_another_state_{reader}"} <= set(attempted[method]), reader
    for writer in QH.BATCHES:
        (method,) = [m for m, ps in QH.PROBED.items() if writer in ps]
        assert "bad_file_in_the_middle" in attempted[method], writer
    assert set(QH.BAD_FILE_OF) == set(QH.READERS) and set(QH.OTHER_STATE) == {"A", "E"}
    assert QH.NEW_IMAGE_SHAPE not in QH.IMAGE_SHAPES and QH.UNBUILT not in QH.LAMBS_A + QH.LAMBS_SUB


def test_the_bad_priors_are_bad_in_the_way_they_say():
    from vbq_amd.tables import n_bit_binary_floats, rank_of_slot
    xi = np.repeat(np.hstack([n_bit_binary_floats(n) for n in range(QH.N + 1)])[:, None], QH.C, axis=1)
    good = QH.Grid(1.25).inverse_cdf(xi)
    for st in QH.STATES.values():                      # the table of no state: a half-applied build would show
        assert good.astype(np.float32).T.tobytes() != QH.code_points(st).tobytes()
    order = QH.BadPrior("order").inverse_cdf(xi)
    assert order.shape == good.shape == (QH.T, QH.C) and (order != good).sum() == 2
    for pts, monotone in ((good, True), (order, False)):
        ranked = np.empty((QH.C, QH.T), np.float32)
        ranked[:, rank_of_slot(QH.N)] = pts.astype(np.float32).T
        assert bool(np.all(np.diff(ranked, axis=1) >= 0)) == monotone
    assert QH.BadPrior("shape").inverse_cdf(xi).shape == (QH.T - 1, QH.C)
    with pytest.raises(ArithmeticError):
        QH.BadPrior("raises").inverse_cdf(xi)


def test_recipes_are_deterministic():
    for kind in ("A", "B"):
        a, b = QH.fit_latents(kind), QH.fit_latents(kind)
        assert all(np.array_equal(x, y) and x.dtype == np.float32 and x.shape == (QH.FIT_ROWS, QH.C) for x, y in zip(a, b))
    assert not np.array_equal(QH.fit_latents("A")[0], QH.fit_latents("B")[0])
    # B as described: means near 0 with wide posteriors where A has means of the prior's spread and narrow posteriors
    (ma, la), (mb, lb) = QH.fit_latents("A"), QH.fit_latents("B")
    assert mb.std() < 0.25 * ma.std() and lb.mean() > la.mean() + 3
    for st in QH.STATES.values():
        assert np.array_equal(QH.code_points(st), QH.code_points(st))
    for a, b in zip(QH.latents(QH.FILE_SHAPES), QH.latents(QH.FILE_SHAPES)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].shape == a[1].shape
    assert [a[0].shape for a in QH.latents(QH.FILE_SHAPES)] == list(QH.FILE_SHAPES)
    assert np.array_equal(QH.image(QH.IMAGE_SHAPES[0]), QH.image(QH.IMAGE_SHAPES[0]))


def test_states_keep_the_shapes_and_differ_as_described():
    A = QH.STATES["A"]
    assert set(QH.STATES) >= {"A", "B", "S2", "Lsub", "E", "E2", "R"}
    assert QH.STATES["B"]._replace(name="A", fit="A") == A and QH.STATES["S2"]._replace(name="A", smoothing=1) == A
    assert QH.STATES["S2"].smoothing == 2 and QH.STATES["R"]._replace(name="A", replaced=None) == A
    assert QH.STATES["R"].replaced in A.lambs
    assert len(A.lambs) == 6 and min(A.lambs) <= 0.01 and max(A.lambs) >= 30
    sub, full = QH.STATES["Lsub"].lambs, A.lambs
    kept = [l for l in sub if l in full]
    assert set(sub) - set(full) == {QH.NEW} and set(full) - set(sub) == set(QH.DROPPED) and 0 < len(kept) < len(full)
    assert kept != sorted(kept) and kept != [l for l in full if l in kept]               # reordered
    # the inputs name the lambda at index 2 of the sorted list in every probe: NEW in Lsub, a dropped one in A
    assert sorted(sub)[2] == QH.NEW and sorted(full)[2] in QH.DROPPED and sorted(full)[2] == QH.REPLACED


def test_tables_are_strict_except_the_clamped_ones():
    """Through the ordering build_code_points uses: the level-major table put into rank order is non-decreasing for every state,
    strictly increasing for all but E and E2, whose outer code points coincide in every channel -- and differently in the two."""
    from vbq_amd.tables import rank_of_slot
    canon = {}
    for name, st in QH.STATES.items():
        lm = QH.code_points(st)
        assert lm.shape == (QH.C, QH.T) and lm.dtype == np.float32
        ranked = np.empty_like(lm)
        ranked[:, rank_of_slot(QH.N)] = lm
        d = np.diff(ranked, axis=1)
        assert np.all(d >= 0), name
        if st.clamp is None:
            assert np.all(d > 0), name
        else:
            assert np.all(ranked[:, 0] == ranked[:, 1]) and np.all(ranked[:, -1] == ranked[:, -2]), name
            assert np.all((d > 0).sum(axis=1) > QH.T // 2), name                    # most of the grid is still there
            canon[name] = np.stack([np.searchsorted(r, r, side="left") for r in ranked])
    assert set(canon) == {"E", "E2"} and not np.array_equal(canon["E"], canon["E2"])


def test_class_maps_use_every_class():
    for P in (2, 3):
        maps = QH.class_maps(QH.FILE_SHAPES, P)
        assert len(maps) == len(QH.FILE_SHAPES)
        for m, sh in zip(maps, QH.FILE_SHAPES):
            assert m.shape == sh[:-1] and m.dtype.kind == "i" and set(np.unique(m)) == set(range(P))
        again = QH.class_maps(QH.FILE_SHAPES, P)
        assert all(np.array_equal(a, b) for a, b in zip(maps, again))


def test_inputs_name_the_third_lambda_everywhere():
    inp = QH.Inputs(sorted(QH.LAMBS_SUB), QH.latents(QH.FILE_SHAPES), QH.class_maps(QH.FILE_SHAPES, 2),
                    QH.class_maps(QH.FILE_SHAPES, 3), {}, "t")
    l = QH.NEW
    assert inp.lamb == l and l in inp.lambs and l in inp.ls and l in inp.palette2 and l in inp.palette3
    assert inp.file_lambs[0] == l and all(l in p for p in inp.file_palettes) and any(l in p for p in inp.ladder)
    assert len(inp.ladder) >= 3 and all(len(p) == 2 for p in inp.ladder)
    assert len(set(inp.file_lambs)) >= 3 and len(set(inp.file_palettes)) == 3


@pytest.mark.parametrize("lengths,want,rung", [([90, 80, 70, 60, 50], 2, 2), ([90, 90, 70, 60], 1, 2), ([50, 60, 40, 45, 30], 4, 4), ([50, 60, 40, 45, 30], 3, 2),
                                               ([50, 60, 40, 45, 30], 1, 2), ([10, 8], 3, 1)])
def test_interior_budget_selects_its_rung(lengths, want, rung):
    from vbq_amd import bitstream
    b = QH.interior_budget(lengths, want)
    assert lengths[rung] <= b < min(lengths[:rung])
    assert int(bitstream.smallest_rates_within(np.array([lengths]), b)[0]) == rung
    assert bitstream.smallest_rate_within({float(k): v for k, v in enumerate(lengths)}, b) == float(rung)


def test_interior_budget_without_room():
    with pytest.raises(AssertionError):
        QH.interior_budget([40, 40, 41], 1)
    assert QH.interior_budget([40, 40, 41], 1, strict=False) == 40


def test_outcomes_compare_exactly():
    a = ("ok", (b"ab", 3, np.array([1.0, np.nan], np.float32), ((0.5, 7),)))
    assert QH.same(a, ("ok", (b"ab", 3, np.array([1.0, np.nan], np.float32), ((0.5, 7),))))
    assert not QH.same(a, ("ok", (b"ab", 3, np.array([1.0, np.nan], np.float64), ((0.5, 7),))))
    assert not QH.same(a, ("ok", (b"ab", 3, np.array([1.0, -np.nan], np.float32), ((0.5, 7),))))
    assert not QH.same(a, ("ok", (b"ac", 3, np.array([1.0, np.nan], np.float32), ((0.5, 7),))))
    assert not QH.same(a, ("ok", (b"ab", 3, np.array([[1.0, np.nan]], np.float32), ((0.5, 7),))))
    assert not QH.same(a, ("raised", "KeyError", "0.3")) and not QH.same(("ok", (1,)), ("ok", (1, 1)))
    assert QH.same(QH._plain({0.5: [np.float32(1), torch.arange(3)]}), ((0.5, (np.float32(1), np.arange(3))),))
    assert QH.outcome(lambda q, i: {}[i], None, 0.3) == ("raised", "KeyError", "0.3")
    with pytest.raises(ZeroDivisionError):                        # nothing but the documented errors is recorded
        QH.outcome(lambda q, i: 1 // 0, None, None)
