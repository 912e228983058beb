"""A quantizer with a history answers as a fresh one does (tests/quantizer_histories.py states the property and holds the
states, the probes and the registry of probed methods).

a. transitions: a quantizer warmed by every probe in one state and moved to another through the public API answers every probe
   as fresh(new) does -- and fresh(old) and fresh(new) disagree on every probe outside UNCHANGED, so the transition is not
   vacuous; pickling and save / load of a warmed quantizer answer as fresh(A);
b. files written before a transition that changes the tables are refused by every reader with its digest error (the batch
   readers name the file), files of fresh(new) are read bit for bit;
c. one quantizer through a schedule of shapes -- the batch, one file of one row, a batch whose plan outgrows the pinned staging
   block, the first batch again, no file -- for every batch and budget family in both input forms; image shapes for
   compress_latents and compress_replay; boxes for the window readers;
d. more (palette, segment) and (lambdas, segment) tags than the codec caches hold;
e. the control: a stale entry planted in each cache slot, re-keyed so the lookup accepts it, changes at least one probe.

Every comparison is exact (quantizer_histories.same).  The answers of the fresh quantizers are computed once per (state,
probe, inputs), each by a quantizer built for that one question, and shared by the tests."""
import pickle
import re
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import quantizer_histories as QH  # noqa: E402

pytestmark = pytest.mark.gpu
C = QH.C


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    t0 = time.perf_counter()
    yield
    print(f"\n[test_gpu_quantizer_histories] {time.perf_counter() - t0:.1f} s")


# ------------------------------------------------------------------------------------------------------------------ the oracle
_INPUTS, _ORACLE, _FILES = {}, {}, {}
ONE_ROW = ((1, C),)
BIG = tuple((1 + f % 3, C) for f in range(1200))        # its plan alone (descriptors, items, totals) is more than 64 KiB
SHAPES = {"main": QH.FILE_SHAPES, "one_row": ONE_ROW, "big": BIG, "none": ()}


def inputs(state, which="main"):
    """The inputs of a state: its lambdas, the files of SHAPES[which], budgets from a fresh quantizer of the state."""
    key = (state, which)
    if key not in _INPUTS:
        _INPUTS[key] = QH.make_inputs(QH.fresh(QH.STATES[state]), QH.STATES[state].lambs, SHAPES[which], f"{state}/{which}",
                                      strict=which == "main")
    return _INPUTS[key]


def oracle(state, name, probe, inp):
    """What a quantizer built once, in `state`, and asked only this answers."""
    key = (state, name, inp.tag)
    if key not in _ORACLE:
        _ORACLE[key] = QH.outcome(probe, QH.fresh(QH.STATES[state]), inp)
    return _ORACLE[key]


def files_of(state):
    """Every file of the state's main inputs in every format, written by a fresh quantizer."""
    if state not in _FILES:
        _FILES[state] = QH.written_all(QH.fresh(QH.STATES[state]), inputs(state))
    return _FILES[state]


def _brief(o):
    if o[0] == "raised":
        return f"{o[1]}({o[2][:120]!r})"
    return "ok(" + ", ".join(f"{type(x).__name__}" + (f"[{len(x)}]" if hasattr(x, "__len__") else "") for x in o[1]) + ")"


def disagreements(q, state, inp, only=None):
    """The probes on which q's answer is not the fresh quantizer's, each with a short account."""
    bad = []
    for name, probe, i in QH.runs(inp):
        if only is not None and name not in only:
            continue
        got, want = QH.outcome(probe, q, i), oracle(state, name, probe, i)
        if not QH.same(got, want):
            bad.append(f"{name}: got {_brief(got)}, fresh {_brief(want)}")
    return bad


def warm(q, state):
    """Every probe once (every cache and buffer is warm afterwards) -- and each answer the fresh one's, whatever came before."""
    bad = disagreements(q, state, inputs(state))
    assert not bad, f"in state {state}, after the probes before it: " + "; ".join(bad)


# ------------------------------------------------------------------------------------------------------------------ a. transitions
TRANSITIONS = [("A", "B"), ("A", "S2"), ("A", "Lsub"), ("A", "E"), ("E", "A"), ("A", "R"),
               ("R", "A"), ("Lsub", "A"), ("E", "E2")]       # and back: a rebuild over replaced arrays, lambdas that return, two non-strict tables
NO_LAMBDA = "names no lambda and reads the code-point table alone"
SAME_TABLE = "the code points did not change"
UNCHANGED = {
    ("A", "B"): {"intervals": NO_LAMBDA + ": " + SAME_TABLE},
    ("A", "S2"): {"intervals": NO_LAMBDA + ": " + SAME_TABLE},
    ("A", "Lsub"): {"intervals": NO_LAMBDA + ": " + SAME_TABLE},
    ("A", "E"): {},
    ("E", "A"): {},
    ("A", "R"): {"intervals": NO_LAMBDA + ": " + SAME_TABLE},
    ("R", "A"): {"intervals": NO_LAMBDA + ": " + SAME_TABLE},
    ("Lsub", "A"): {"intervals": NO_LAMBDA + ": " + SAME_TABLE},
    ("E", "E2"): {},
}
"""transition -> {probe: why fresh(old) and fresh(new) give the same answer}.  Everything else must differ."""


@pytest.mark.parametrize("old,new", TRANSITIONS, ids=[f"{a}-{b}" for a, b in TRANSITIONS])
def test_transition(old, new):
    q = QH.fresh(QH.STATES[old])
    warm(q, old)
    QH.move(q, QH.STATES[new], QH.STATES[old])
    inp = inputs(new)
    bad = disagreements(q, new, inp)
    assert not bad, f"after {old} -> {new}: " + "; ".join(bad)
    # not vacuous: asked the same, fresh(old) and fresh(new) disagree wherever UNCHANGED does not say why they agree
    unchanged = UNCHANGED[(old, new)]
    assert all(unchanged.values())
    agree = [name for name, probe, i in QH.runs(inp) if QH.same(oracle(old, name, probe, i), oracle(new, name, probe, i))]
    listed = [n for n in agree if n.split("[")[0] in unchanged]
    assert sorted(agree) == sorted(listed), f"{old} and {new} agree on probes UNCHANGED does not list: {sorted(set(agree) - set(listed))}"
    silent = [n for n in unchanged if n not in agree]
    assert not silent, f"UNCHANGED[{old} -> {new}] lists probes that do change: {silent}"


def test_chain_of_transitions():
    """One long-lived quantizer that keeps returning to a state it has been in: every cache has then held entries for the very
    state it is asked about again, built from objects that are gone (and whose addresses may have been given out anew)."""
    chain = ["A", "B", "A", "E", "A", "R", "A"]
    q = QH.fresh(QH.STATES[chain[0]])
    warm(q, chain[0])
    for step, (old, new) in enumerate(zip(chain, chain[1:])):
        QH.move(q, QH.STATES[new], QH.STATES[old])
        bad = disagreements(q, new, inputs(new))
        assert not bad, f"step {step}, {old} -> {new}: " + "; ".join(bad)


def test_dropped_lambda_raises_key_error():
    """After A -> Lsub every probe that names a lambda the rebuild dropped raises KeyError, as on fresh(Lsub): asked to write,
    and asked to read the files a fresh A wrote at that lambda."""
    q = QH.fresh(QH.STATES["A"])
    warm(q, "A")
    QH.move(q, QH.STATES["Lsub"], QH.STATES["A"])
    ls = sorted(QH.DROPPED[0] if l == QH.NEW else l for l in QH.LAMBS_SUB)
    drop = QH.make_inputs(QH.fresh(QH.STATES["A"]), ls, QH.FILE_SHAPES, "Lsub/dropped")
    assert drop.lamb == QH.DROPPED[0] == inputs("A").lamb
    asked = [r for r in QH.runs(drop) if r[0] != "intervals"]
    asked += [(name + "[given]", p, drop.reading(files_of("A"), "A")) for name, p in QH.READERS.items()]
    for name, probe, i in asked:
        got, want = QH.outcome(probe, q, i), oracle("Lsub", name, probe, i)
        assert got[:2] == ("raised", "KeyError") and QH.same(got, want), f"{name}: got {_brief(got)}, fresh {_brief(want)}"


def test_pickled_quantizer_answers_as_fresh():
    q = QH.fresh(QH.STATES["A"])
    warm(q, "A")
    q2 = pickle.loads(pickle.dumps(q))
    assert q2._dev_cache == {}
    bad = disagreements(q2, "A", inputs("A"))
    assert not bad, "after pickling: " + "; ".join(bad)
    bad = disagreements(q, "A", inputs("A"), only=("latents", "to_bytes", "b_mapped", "r_batch"))
    assert not bad, "the pickled quantizer itself: " + "; ".join(bad)


def test_saved_and_loaded_quantizer_answers_as_fresh(tmp_path):
    from vbq_amd import ChannelwisePriorCDFQuantizer
    q = QH.fresh(QH.STATES["A"])
    warm(q, "A")
    path = str(tmp_path / "quantizer.npz")
    q.save(path)
    bad = disagreements(ChannelwisePriorCDFQuantizer.load(path), "A", inputs("A"))
    assert not bad, "after save and load: " + "; ".join(bad)


@pytest.mark.parametrize("state", ["A", "B", "E"])
def test_budgets_choose_interior_rungs_that_differ_between_files(state):
    """The budgets are conditions computed from the oracle, and they do what they are for: every budget call of the main inputs
    keeps an interior rung -- not the first, which fits any larger budget, nor the last -- and the files of a batch keep
    different ones; the one-file and total calls keep the rung of ls[2]."""
    from vbq_amd import bitstream
    inp = inputs(state)
    ls, ladder = inp.ls, [tuple(p) for p in inp.ladder]
    fresh = lambda name: oracle(state, name, QH.PROBES[name], inp)[1]
    for name, parse in (("b_to_budget", bitstream.parse), ("b_compact_budget", bitstream.parse_compact)):
        rungs = [ls.index(parse(d)[0].lamb) for d in fresh(name)[0]]
        assert all(0 < r < len(ls) - 1 for r in rungs) and len(set(rungs)) > 1, (name, rungs)
    rungs = [ladder.index(bitstream.parse_mapped(d)[0].lambs) for d in fresh("b_mapped_budget")[0]]
    assert all(0 < r < len(ladder) - 1 for r in rungs) and len(set(rungs)) > 1, rungs
    for name, parse in (("to_budget", bitstream.parse), ("to_budget_c", bitstream.parse_compact)):
        assert parse(fresh(name)[0])[0].lamb == ls[2], name
    for name in ("b_total_budget", "b_compact_total_budget"):
        assert fresh(name)[0] == ls[2], name
    assert ladder[1] == (ls[1], ls[2]) and fresh("b_mapped_total_budget")[0] == 1
    assert bitstream.parse_mapped(fresh("to_budget_mapped")[0])[0].lambs == ladder[1]


# ------------------------------------------------------------------------------------------------------------------ b. old files
MIXED_1D = (1, 4, 4)                                     # the files the one-axis call of the batch readers takes (QH.BOXES_1D)


@pytest.mark.parametrize("new", ["B", "S2", "E"])
def test_old_files_are_refused_and_new_files_read(new):
    old_files, new_files = files_of("A"), files_of(new)
    q = QH.fresh(QH.STATES["A"])
    for name, probe in QH.READERS.items():                 # warm: the readers on the files they are about to refuse
        i = inputs("A").reading(old_files, "A")
        assert QH.same(QH.outcome(probe, q, i), oracle("A", name, probe, i)), name
    QH.move(q, QH.STATES[new], QH.STATES["A"])
    for name, probe in QH.READERS.items():
        i = inputs(new).reading(old_files, "A")
        got = QH.outcome(probe, q, i)
        assert got[:2] == ("raised", "ValueError") and "digest mismatch" in got[2], f"{name}: {_brief(got)}"
        if name in QH.BATCH_READERS:
            assert re.match(r"file 0 ", got[2]), f"{name}: {got[2]}"
        assert QH.same(got, oracle(new, name, probe, i)), name
        i = inputs(new).reading(new_files, new)
        got = QH.outcome(probe, q, i)
        assert got[0] == "ok" and QH.same(got, oracle(new, name, probe, i)), f"{name}: {_brief(got)}"
    # one old file among new ones: refused, and the error names it
    b = [new_files["b"][f] for f in MIXED_1D]
    b[1] = old_files["b"][MIXED_1D[1]]
    with pytest.raises(ValueError, match=r"^file 1 .*digest mismatch"):
        q.decompress_latents_batch(b, regions=QH.BOXES_1D)
    m = [new_files["m"][f] for f in MIXED_1D]
    m[2] = old_files["m"][MIXED_1D[2]]
    with pytest.raises(ValueError, match=r"^file 2 .*digest mismatch"):
        q.decompress_latents_mapped_batch(m, regions=QH.BOXES_1D)
    c = list(new_files["c"])
    c[3] = old_files["c"][3]
    with pytest.raises(ValueError, match=r"^file 3 .*digest mismatch"):
        q.decompress_latents_compact_batch(c, stack=False)
    # and the refusals left nothing behind: the new files still read as before
    for name in QH.BATCH_READERS:
        i = inputs(new).reading(new_files, new)
        assert QH.same(QH.outcome(QH.READERS[name], q, i), oracle(new, name, QH.READERS[name], i)), name


# ------------------------------------------------------------------------------------------------------------------ c. schedules
SCHEDULE = ("main", "one_row", "big", "main", "none")


@pytest.mark.parametrize("form", ["numpy", "device"])
@pytest.mark.parametrize("family", list(QH.BATCHES))
def test_schedule_of_batches(family, form):
    """After every step the answer is fresh(A)'s for that step alone: a region of the reused staging block a smaller plan no
    longer rewrites, or totals that were not zeroed, would show in the step after the large one."""
    probe = QH.BATCHES[family]
    q = QH.fresh(QH.STATES["A"])
    for step, which in enumerate(SCHEDULE):
        i = inputs("A", which) if form == "numpy" else inputs("A", which).on_device()
        if which == "big":
            assert q._dev_cache["_encode_stage"].numel() == 1 << 16            # the premise: the block is at its minimum ...
        got, want = QH.outcome(probe, q, i), oracle("A", family, probe, i)
        assert QH.same(got, want), f"step {step} ({which}): got {_brief(got)}, fresh {_brief(want)}"
        if which == "big":
            assert q._dev_cache["_encode_stage"].numel() > 1 << 16             # ... and this plan made it grow
        assert (want[0] == "ok") == (which != "none" or "total" not in family), _brief(want)


def _latents_at(shape):
    def probe(q, i):
        m, lv = QH.latents([shape], seed=13)[0]
        out = q.compress_latents(m, lv, i.lambs)
        return tuple(np.asarray(out[k][l]) for k in ("Z_hat", "raw_num_bits", "num_bits_cl", "num_bits") for l in out[k])
    return probe


def test_schedule_of_image_shapes_compress_latents():
    q = QH.fresh(QH.STATES["A"])
    shapes = [(24, 24, C), (1, C), (40, 50, C)]              # the last one makes the persistent workspace grow
    for step, shape in enumerate(shapes + shapes[:1]):
        probe = _latents_at(shape)
        got, want = QH.outcome(probe, q, inputs("A")), oracle("A", f"latents{shape}", probe, inputs("A"))
        assert want[0] == "ok" and QH.same(got, want), f"step {step} {shape}: got {_brief(got)}, fresh {_brief(want)}"


def test_schedule_of_image_shapes_compress_replay():
    q = QH.fresh(QH.STATES["A"])
    for step, shape in enumerate(QH.IMAGE_SHAPES + QH.IMAGE_SHAPES[:1]):
        probe = lambda q, i, shape=shape: QH.v_replay(q, i, shape)
        got, want = QH.outcome(probe, q, inputs("A")), oracle("A", f"v_replay{shape}", probe, inputs("A"))
        assert want[0] == "ok" and QH.same(got, want), f"step {step} {shape}: got {_brief(got)}, fresh {_brief(want)}"
    replays = list(q._dev_cache["_replays"].values())
    assert {r.mode for r in replays} == {"full"}, "the stub VAE was meant to be captured whole"
    # one capture per shape: the first shape's graph was kept and replayed when the shape returned (two images per visit)
    assert sorted(r.replays for r in replays) == [2, 2, 4], [(r.shape, r.replays) for r in replays]


@pytest.mark.parametrize("kind,method", [("b", "decompress_latents_window"), ("m", "decompress_latents_mapped_window"),
                                         ("b", "decompress_latents_mapped_window")])
def test_schedule_of_windows(kind, method):
    data = files_of("A")[kind][0]
    q = QH.fresh(QH.STATES["A"])
    for step, (region, channels) in enumerate(QH.WINDOWS):
        probe = lambda q, i, region=region, channels=channels: (getattr(q, method)(data, region, channels),)
        got, want = QH.outcome(probe, q, inputs("A")), oracle("A", f"{method}/{kind}/{step}", probe, inputs("A"))
        assert want[0] == "ok" and QH.same(got, want), f"step {step}: got {_brief(got)}, fresh {_brief(want)}"


# ------------------------------------------------------------------------------------------------------------------ d. eviction
def test_more_palette_tags_than_the_codec_cache_holds():
    """Ten distinct (palette, segment) tags through the mapped one-file calls, then the first again: _coder_maps clears itself
    when a ninth arrives."""
    ls = sorted(QH.LAMBS_A)
    m, lv = inputs("A").files[0]
    cls = inputs("A").cls2[0]
    q = QH.fresh(QH.STATES["A"])
    tags = [((ls[k % 6], ls[(k + 1 + k // 6) % 6]), 32 + 16 * k) for k in range(10)]
    assert len(set(tags)) == 10
    for step, (palette, segment) in enumerate(tags + tags[:1]):
        def probe(q, i, palette=palette, segment=segment):
            data = q.compress_latents_to_bytes_mapped(m, lv, palette, cls, segment=segment)
            return data, q.coded_nbytes_mapped(m, lv, palette, cls, segment=segment), q.decompress_latents(data)
        got, want = QH.outcome(probe, q, inputs("A")), oracle("A", f"mapped_tag{palette}{segment}", probe, inputs("A"))
        assert want[0] == "ok" and QH.same(got, want), f"step {step} {palette} {segment}: got {_brief(got)}, fresh {_brief(want)}"
    assert len(q._dev_cache["_coder_maps"][2]) <= 8


def test_more_rate_tags_than_the_codec_cache_holds():
    """Ten distinct (lambdas, segment) tags through the rate calls, one file and batch, then the first again: _coder_stacks
    clears itself when a ninth arrives."""
    ls = sorted(QH.LAMBS_A)
    files = inputs("A").files
    q = QH.fresh(QH.STATES["A"])
    tags = [(tuple(ls[(k + j) % 6] for j in range(2 + k % 3)), 48 + 8 * k) for k in range(10)]
    assert len(set(tags)) == 10
    for step, (lambs, segment) in enumerate(tags + tags[:1]):
        def probe(q, i, lambs=lambs, segment=segment):
            return q.coded_nbytes(*files[0], list(lambs), segment=segment), q.coded_nbytes_batch(files, list(lambs), segment=segment)
        got, want = QH.outcome(probe, q, inputs("A")), oracle("A", f"rate_tag{lambs}{segment}", probe, inputs("A"))
        assert want[0] == "ok" and QH.same(got, want), f"step {step} {lambs} {segment}: got {_brief(got)}, fresh {_brief(want)}"
    assert len(q._dev_cache["_coder_stacks"][2]) <= 8


# ------------------------------------------------------------------------------------------------------------------ e. the control
CODER, KEYED, NAMED = "coder", "keyed", "named"
SLOTS = {
    # slot: (kind, old, new -- a transition after which the new state consults the slot --, the probes that read it)
    "_coder_tables": (CODER, "A", "B", ("to_bytes", "to_bytes_c")),
    "_coder_stacks": (CODER, "A", "B", ("coded_nbytes", "b_to_bytes")),
    "_coder_maps": (CODER, "A", "B", ("to_bytes_mapped", "r_decompress_m")),
    # the two slots of _keyed_dev serve model dicts of NumPy arrays: a non-strict table's, so between two of those
    "level_len": (KEYED, "E", "E2", ("latents", "batch_channel")),
    "entropy_models": (KEYED, "E", "E2", ("latents",)),
    "table_lm": (NAMED, "A", "E", ("latents", "intervals")),
    "sorted": (NAMED, "A", "E", ("latents", "r_decompress_b")),
    "canon": (NAMED, "E", "E2", ("to_bytes", "coded_nbytes")),
    "canon_u16": (NAMED, "E", "E2", ("b_to_bytes", "b_coded_nbytes")),
}


@pytest.mark.parametrize("slot", list(SLOTS))
def test_control_a_stale_cache_entry_is_seen(slot):
    """The probes can see a stale cache at all: the entry of the old state put back after the transition, re-keyed so that the
    lookup accepts it, changes an answer.  Only the numbers change: the planted entry has the live one's shape and dtype."""
    kind, old, new, readers = SLOTS[slot]
    q = QH.fresh(QH.STATES[old])
    warm(q, old)
    assert not disagreements(q, old, inputs(old), only=readers)          # (the slot now holds what these probes last asked for)
    saved = q._dev_cache[slot]
    QH.move(q, QH.STATES[new], QH.STATES[old])
    bad = disagreements(q, new, inputs(new), only=readers)
    assert not bad, "; ".join(bad)
    live = q._dev_cache[slot]
    if kind == CODER:                                                  # (the _code_counts object, add_n_smoothing, the payload)
        # (a payload that cleared itself on the way keeps fewer tags than were asked for: the old entries go under the tags
        # both have -- the probes below ask for them again)
        assert live[0] is q._code_counts and live[0] is not saved[0] and set(saved[2]) & set(live[2])
        q._dev_cache[slot] = (live[0], live[1], {**live[2], **{k: v for k, v in saved[2].items() if k in live[2]}})
    elif kind == KEYED:                                                # (the model arrays, the device table)
        assert live[1].shape == saved[1].shape and live[1].dtype == saved[1].dtype and not torch.equal(live[1], saved[1])
        q._dev_cache[slot] = (live[0], saved[1])
    else:
        assert live.shape == saved.shape and live.dtype == saved.dtype and live is not saved
        assert not torch.equal(live.view(torch.uint8), saved.view(torch.uint8))
        q._dev_cache[slot] = saved
    bad = disagreements(q, new, inputs(new), only=readers)
    assert bad, (f"a stale {slot} changed none of {readers}: either no probe reads the slot (add one to "
                 "tests/quantizer_histories.py) or the slot is dead")
