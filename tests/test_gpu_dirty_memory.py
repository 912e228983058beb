"""No call's answer depends on what its fresh memory held (tests/dirty_memory.py says how the fill works and why these bytes).

A CALL is a catalogue entry.  It is answered four times -- unpatched, and under Fill(0x00), Fill(0x01), Fill(0x3C) -- each time on
objects of its own (a quantizer built unpatched in state A, a new codec, new inputs); the answer is read into plain host values
(stream_order.plain) WHILE THE FILL IS ACTIVE (reading a lazy result allocates too) and the four must be the same: dtype, shape and
every bit (quantizer_histories.same).  A failure names the call, the fill, and the first differing leaf and element.

a. every probe of quantizer_histories.PROBES on a quantizer in state A, the file probes also with device tensors; compress_replay
   additionally with ONE quantizer whose capture was made under one fill and is replayed under the next;
b. every case of test_gpu_stream_order.CASES as call(make(7)) (the module is imported, its cases are not copied);
c. the calls whose stream tests live in their own modules (CALLS below), at the small shapes of those modules, and the four
   combinations of given / fresh `words` x `sizes` of ops.rans_encode_files and ops.rans_map_encode_files;
d. state built on dirty memory: a quantizer taken through build_code_points and build_entropy_models_from_latents entirely under
   a fill (the one-call build, the build with host stages, the build on a table with repeated code points), EntropyModelBuild.run
   with one and two chunks and smoothing 0, 1 and 0.5 (host stages, the native and the Python form) -- also a second run of
   one object under the next fill, on other latents, so that the buffers it reuses hold a real previous answer --, and a
   single-file writer against the batch writer under a fill;
e. the parts a contract leaves open are masked, exactly those, by MASKS; dirty_memory.UNSPECIFIED quotes the sentence;
f. coverage: every allocation site of vbq_amd/*.py is reached by this module under a fill or explained in
   dirty_memory.EXEMPT_SITES (the last test; it prints the three counts);
g. the control: with torch.Tensor.zero_ a no-op around EntropyModelBuild.run the 0x01 and 0x3C answers differ from the unpatched
   one in level_counts (bins are only added to and the length look-up clamps its index: a wrong value and nothing else), and a
   fake call returning torch.empty(4) is reported.  If the control does not fire the module tests nothing, and says so.

WHAT THE MODULE FOUND when it was written: ops.rans_encode_files and ops.rans_map_encode_files zeroed a `words` of their own only
when `sizes` was theirs too -- with `sizes` given, the slots no item names held torch.empty contents
(test_encode_files_given_and_fresh_outputs).  The library's own callers pass both.

It found nothing else: every probe, case and call answered the same under all three fills.  With that fix taken out again,
exactly the two cases with a fresh `words` and a given `sizes` fail (one per entry point, and already unpatched: the process
is old enough by then for the allocator to hand back a block that held another test's words).

MEASURED on an MI355X (155 tests): the module takes 5.5 .. 6.0 s after 9 s of set-up (the library load and the first quantizer);
140 allocation sites, 128 reached under a fill, 14 exempt, none unexplained.  The fixture below prints these figures on every run."""
import contextlib
import os
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dirty_memory as DM  # noqa: E402
import quantizer_histories as QH  # noqa: E402
import stream_order as SO  # noqa: E402
import test_gpu_stream_order as TSO  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
A = QH.STATES["A"]
N4, T4, CH, ROWS = TSO.N4, TSO.T4, TSO.CH, TSO.ROWS
dev = TSO.dev


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    t0 = time.perf_counter()
    yield
    print(f"\n[test_gpu_dirty_memory] {time.perf_counter() - t0:.1f} s; {len(DM.allocation_sites())} allocation sites, "
          f"{len(DM.sites_reached() & DM.allocation_sites())} reached under a fill, {len(DM.EXEMPT_SITES)} exempt")


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """A device error is not a wrong answer: after one, nothing more of this module is launched."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"device error, the rest of the module is not run: {e}", returncode=3)


# ====================================================================================================== the harness
def _fill(byte):
    return contextlib.nullcontext() if byte is None else DM.Fill(byte)


def _tag(byte):
    return "unpatched" if byte is None else f"Fill(0x{byte:02X})"


def four_answers(name, setup, mask=None):
    """setup() -> go, unpatched and once per answer; go() under the fill; -> {None | byte: the plain answer}."""
    out = {}
    for byte in (None,) + DM.FILLS:
        go = setup()
        with _fill(byte):
            got = SO.plain(go())
            torch.cuda.synchronize()
        out[byte] = got if mask is None else mask(got)
    return out


def differences(name, answers):
    """One line per fill whose answer is not the unpatched one."""
    want, lines = answers[None], []
    for byte in DM.FILLS:
        if not QH.same(answers[byte], want):
            zero = "" if byte == 0 or QH.same(answers[0], want) else " (zero-filled memory differs as well)"
            lines.append(f"{name} under {_tag(byte)} differs from the unpatched answer{zero}: "
                         f"{DM.first_difference(answers[byte], want)} (filled against unpatched)")
    return lines


def hold(name, setup, mask=None):
    answers = four_answers(name, setup, mask)
    bad = differences(name, answers)
    assert not bad, "\n".join(bad)
    return answers[None]


def test_fill_on_the_device():
    """Device tensors through the uint8 view on the current stream, page-locked and pageable host tensors on the host."""
    s = torch.cuda.Stream()
    with DM.Fill(0x3C), torch.cuda.stream(s):
        d = torch.empty((3, 5), dtype=torch.float32, device="cuda")
        u = torch.empty((), dtype=torch.uint16, device="cuda")
        like = torch.empty_like(torch.zeros((4, 3), device="cuda").t())
        pinned = torch.empty(7, dtype=torch.int32, pin_memory=True)
        host = torch.empty(7, dtype=torch.int64)
        empty = torch.empty((0, 4), device="cuda")
        got = d.cpu()
    assert pinned.is_pinned() and pinned.tolist() == [1010580540] * 7 and host.tolist() == [0x3C3C3C3C3C3C3C3C] * 7
    assert got.view(torch.uint8).unique().tolist() == [0x3C] and int(u.cpu().view(torch.int16)) == 15420 and empty.numel() == 0
    assert like.cpu().view(torch.int32).unique().tolist() == [1010580540] and like.stride() == (1, 3)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with DM.Fill(0x01), torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            captured = torch.empty(5, dtype=torch.int32, device="cuda")
    captured.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert captured.tolist() == [16843009] * 5                                    # the fill is part of the captured graph


# ====================================================================================================== a. the probes
PROBE_RUNS = list(QH.PROBES) + [name + "[device]" for name in {**QH.ONE_FILE, **QH.BATCHES}]


def _probe_setup(name):
    inp, dinp = TSO.inputs_A()
    probe, i = QH.PROBES[name.replace("[device]", "")], (dinp if name.endswith("[device]") else inp)

    def setup():
        q = QH.fresh(A)
        return lambda: QH.outcome(probe, q, i)
    return setup


@pytest.mark.parametrize("name", PROBE_RUNS)
def test_probe(name):
    want = hold(f"probe:{name}", _probe_setup(name))
    assert want[0] == "ok", want[:3]
    assert QH.same(want, TSO.oracle(name, QH.PROBES[name.replace("[device]", "")], TSO.inputs_A()[name.endswith("[device]")]))


def test_replay_captured_under_one_fill_and_replayed_under_the_next():
    """ONE quantizer: v_replay (a capture and a replay) unpatched, then under each fill in turn -- from the second round on the
    graph and its buffers are those captured under the round before; a second image shape is captured under every fill."""
    inp, _ = TSO.inputs_A()
    want = {sh: SO.plain(QH.outcome(lambda q, i: QH.v_replay(q, i, sh), QH.fresh(A), inp)) for sh in QH.IMAGE_SHAPES[:2]}
    q = QH.fresh(A)
    for byte in DM.FILLS + DM.FILLS[:1]:
        for sh in QH.IMAGE_SHAPES[:2]:
            with DM.Fill(byte):
                got = SO.plain(QH.outcome(lambda q_, i: QH.v_replay(q_, i, sh), q, inp))
                torch.cuda.synchronize()
            assert QH.same(got, want[sh]), f"v_replay {sh} under {_tag(byte)}: {DM.first_difference(got, want[sh])}"
    replays = list(q._dev_cache["_replays"].values())
    assert len(replays) == 2 and all(r.replays == 8 for r in replays), [(r.mode, r.replays) for r in replays]


# ====================================================================================================== b. the catalogued cases
@pytest.mark.parametrize("name", list(TSO.CASES))
def test_case(name):
    fn, _ = TSO.CASES[name]

    def setup():
        call, make = fn()
        return lambda: call(make(7))
    hold(name, setup, MASKS.get(name))


# ====================================================================================================== c. calls of other modules
CALLS = {}


def call(name):
    """Register `setup() -> go`: setup runs unpatched (inputs, fixtures), go() under the fill."""
    def deco(fn):
        assert name not in CALLS and name not in TSO.CASES and name not in QH.PROBES, name
        CALLS[name] = fn
        return fn
    return deco


def _golden(name):
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))


K_ROW, BITS = TSO.K_ROW, TSO.BITS


def _lists(rng, Q, M, V):
    ids = rng.integers(0, V, (Q, M))
    ids[0, -1] = -1                                                              # padding scores -inf
    return ids


@call("records_scores_similarity_rerank_most_similar_bag")
def _():
    from vbq_amd import embeddings as E
    data = TSO._record_file(1)
    rng = np.random.default_rng(9)
    q, ids = rng.normal(0, 1, (3, K_ROW)).astype(F32), _lists(rng, 3, 6, 40)

    def go():
        re = E.RecordEmbeddings(data)
        return (re.scores(q, ids), re.scores(q[0], ids[1], metric="dot"), re.similarity([1, 5, 39], [2, 0, 39]),
                re.rerank(q, ids, k=4), re.rerank(q, dev(ids)), re.most_similar(q, k=3), re.most_similar(ids=[2, 0], k=3, metric="dot"),
                re.bag([[0, 1, 5], [2, -1, 39]]), re.bag([4, 4, 7, 1], [0, 1], mode="mean"), re.rows([3, 1, 39, 3]), re.tensor())
    return go


@call("dense_scores_similarity_rerank_most_similar_bag")
def _():
    from vbq_amd import embeddings as E
    rng = np.random.default_rng(9)
    q, ids = rng.normal(0, 1, (3, 7)).astype(F32), _lists(rng, 3, 6, 301)

    def go():
        emb = TSO._emb(7)
        return (E.scores(emb, q, ids), E.scores(emb, q[0], ids[1], metric="dot"), E.similarity(emb, [1, 5, 300], [2, 0, 300]),
                E.rerank(emb, q, ids, k=4), E.rerank(emb, q, dev(ids)), E.most_similar(emb, q, k=5),
                E.most_similar(emb, q, k=2, metric="dot", exclude=[[1, -1], [7, 8], [0, 0]]), E.bag(emb, [[0, 1, 5], [2, -1, 300]]),
                E.bag(emb, [4, 4, 7, 1], [0, 1], mode="mean"), E.bag(emb, [4, 4, 7, 1], [0, 1], weights=[0.5, 1.0, 2.0, 1.5]))
    return go


def _fhat(K, N, R, seed):
    import test_gpu_budget_sweep as TBS
    return TBS._scores(np.random.default_rng(seed), N, R, K)


@call("budget_dp")
def _():
    from vbq_amd import ops
    fhat = _fhat(7, 4, 6, 1)
    return lambda: (ops.budget_dp(dev(fhat), 7, 13), ops.budget_dp(dev(fhat), 7, 0), ops.budget_dp(dev(fhat), 7, 28))


@call("budget_dp_sweep")
def _():
    from vbq_amd import ops
    fhat = _fhat(7, 4, 6, 2)
    return lambda: (ops.budget_dp_sweep(dev(fhat), 7, [0, 5, 13, 28]), ops.budget_dp_sweep(dev(fhat), 7, [13], curve_len=4),
                    ops.budget_dp_sweep(dev(fhat), 7, [], curve_len=29))


@call("budget_dp_sweep_workspace_path")
def _():
    """The shapes of test_gpu_budget_sweep.py::test_workspace_path_with_one_slice_and_several_rounds: the back-pointers do not fit
    the LDS; a workspace of one slice (five rounds; the test's own torch.empty, dirty as well), then the call's own."""
    from vbq_amd import _lib_budget, ops
    K, N, top, R = 300, 4, 600, 5
    per_row = (K * (top + 1) + 15) // 16 * 16
    assert _lib_budget.lib().vbqb_budget_sweep_workspace_bytes(R, K, N, top + 1) == R * per_row
    fhat, budgets = _fhat(K, N, R, 5), [0, 299, 300, 600]
    return lambda: (ops.budget_dp_sweep(dev(fhat), K, budgets, workspace=torch.empty(per_row, dtype=torch.uint8, device="cuda")),
                    ops.budget_dp_sweep(dev(fhat), K, budgets, curve_len=3), ops.budget_dp(dev(fhat), K, 600))


@call("quantize_rows_to_budget_budgets_curve")
def _():
    import vbq_amd
    from vbq_amd import rows_budget
    book = TSO._book4()
    books = np.stack([book * F32(s) for s in (0.5, 1.0, 1.5, 2.0, 3.0)])         # one code book per column
    per_row = np.array([BITS, 0, 3, K_ROW * N4, 7, BITS, 1, 12, 5])

    def go():
        m, s = TSO._rows(7)
        return (vbq_amd.quantize_rows_to_budget(m, s, BITS, table=book, N=N4), vbq_amd.quantize_rows_to_budget(m, s, per_row, table=books, N=N4),
                rows_budget.quantize_rows_to_budgets(m, s, [BITS, 0, 20, BITS], table=book, N=N4),
                rows_budget.quantize_rows_to_budgets(m.cpu().numpy(), s.cpu().numpy(), [3], table=books, N=N4),
                rows_budget.budget_curve(m, s, table=book, N=N4), rows_budget.budget_curve(m, s, table=books, N=N4, max_bits=7))
    return go


@call("record_files")
def _():
    from vbq_amd import embeddings as E
    book = TSO._book4()
    m, s = (t.cpu().numpy() for t in TSO._rows(3, 40))
    curve = E.records_distortion_curve(m, s, book, N4)
    target, limit = float(np.sort(curve)[len(curve) // 3]), len(E.compress_to_records(m, s, BITS, book, N4))
    return lambda: (E.compress_to_records(m, s, BITS, book, N4), E.compress_to_records_sweep(m, s, [BITS, 0, 20, BITS], book, N4),
                    E.records_distortion_curve(dev(m), dev(s), book, N4), E.compress_to_records_quality(m, s, book, target, N4),
                    E.compress_to_records_budget(m, s, book, limit, N4), E.decompress(E.compress_to_records(m, s, 3, book, N4)))


def _samples(B, C, seed=3):
    import test_gpu_kmeans as TK
    return TK._samples(B, C, seed)


@call("kmeans_prefix_sums_fit_channels_sse_curve")
def _():
    from vbq_amd import kmeans1d
    x, one = _samples(257, 3), _samples(300, 1, seed=4)
    return lambda: (kmeans1d.prefix_sums(x), kmeans1d.prefix_sums(dev(one)), kmeans1d.fit_channels(x, [6, 2, 17, 2, 1]),
                    kmeans1d.fit_channels(dev(one), [3], add_n_smoothing=0.5), kmeans1d.sse_curve(x, 17))


@call("kmeans_fit_channels_with_value_rows_in_the_workspace")
def _():
    import kmeans_reference as KR
    from vbq_amd import kmeans1d
    n = KR.ROWS_IN_LDS_MAX_N + 1
    assert n == 4863
    x = _samples(n, 3, seed=5)
    return lambda: (kmeans1d.fit_channels(x, [1, 3, 2]), kmeans1d.sse_curve(dev(x), 3))


@call("kmeans1d_dp_with_a_nan_channel")
def _():
    """Channel 1 of three holds a NaN: its outputs are masked (MASKS), its neighbours and the status word are not."""
    import kmeans_reference as KR
    import test_gpu_kmeans as TK
    from vbq_amd import kmeans1d
    n, C = 257, 3
    S1, S2, shift = (a.copy() for a in TK._inputs(n, C))
    x = TK._channel(n, 1)[0].copy()
    x[100] = np.nan
    shift[1], S1[1], S2[1] = KR.sums_of(np.sort(x))

    def go():
        status = torch.zeros(1, dtype=torch.uint32, device="cuda")
        return kmeans1d.kmeans1d_dp(dev(S1), dev(S2), dev(shift), [1, 5, 16], status=status) + (status,)
    return go


@call("nearest_code_channels")
def _():
    import test_gpu_kmeans as TK
    from vbq_amd import kmeans1d
    rng = np.random.default_rng(255)
    codes, x = TK._code_rows(rng, 65, 255), (rng.standard_normal((65, 65)) * 16).astype(F32)
    start = rng.integers(1, 1000, (65, 255)).astype(np.int64)

    def go():
        counts = dev(start)
        return kmeans1d.nearest_code_channels(dev(x), dev(codes), counts=counts) + (counts,) + kmeans1d.nearest_code_channels(dev(x[:1]), dev(codes))
    return go


@call("optimal_kmeans_wrapper_fit_and_compress")
def _():
    import test_gpu_kmeans as TK
    import vbq_amd
    levels = [2, 4, 6]
    rng = np.random.default_rng(9)
    X, X2 = rng.random((2, 8, 8, 3)).astype(F32), rng.random((2, 8, 8, 3)).astype(F32)

    def go():
        w = vbq_amd.ChannelwiseOptimalKmeansWrapper(3, levels)
        w.fit(X, TK._StubVAE(), 1.0)
        one = vbq_amd.OptimalKmeansQuantizer(4)
        one.fit(X[..., 1].reshape(-1))
        return (w.code_points, w.code_lengths, w.compress(X2, TK._StubVAE(), levels, clip=True), w.compress(X2, TK._StubVAE(), levels, clip=False),
                one.code_points, one.code_lengths, one.quantize(X2[..., 1].reshape(-1)))
    return go


@call("baseline_quantizers_fit_and_quantize")
def _():
    from vbq_amd import baselines
    x = np.random.default_rng(2).normal(0, 1, 1031).astype(F32)

    def go():
        out = []
        for cls in (baselines.UniformQuantizer, baselines.KmeansQuantizer):
            b = cls(16)
            if cls is baselines.KmeansQuantizer:                                   # (its fit is scikit-learn's)
                b.code_points, b.code_lengths = np.random.default_rng(3).normal(0, 1, 16), np.arange(16.0)
                out.append(b._vq(dev(x), True))
            else:
                b.fit(x)
                out += [b.code_points, b.code_lengths]
            out.append(b.quantize(x))
        return tuple(out)
    return go


@pytest.mark.parametrize("segment", [None, 5, 1000])
def test_compressed_embeddings_on_the_committed_fixtures(segment):
    """VBQe: the file, the exact lengths, the budget rule, CompressedEmbeddings.tensor / rows (whole rows per segment, rows that
    straddle segments) on g13, and the three-dimensional rows of g7."""
    from vbq_amd import embeddings as E
    g, g7 = _golden("g13_notebook_chain.npz"), _golden("g7_notebook.npz")
    means, stds, cp = g["means"][:600], g["stds"][:600], g["codepoints"]
    m7, s7 = g7["means"].reshape(250, 3, 4), g7["stds"].reshape(250, 3, 4)
    V = means.shape[0]
    betas = [0.6, 17.0, 1e3]
    limit = int(np.sort(E.coded_nbytes(means, stds, betas, cp, segment=segment))[1])

    def setup():
        def go():
            data = E.compress_to_bytes(means, stds, 17.0, cp, segment=segment)
            ce = E.CompressedEmbeddings(data)
            d7 = E.compress_to_bytes(m7, s7, 1.0, g7["codepoints"])
            return (data, ce.tensor(), ce.rows([V - 1, 0, 5, 5, 5, V - 1]), ce.rows(torch.tensor([2, 1])), E.decompress(data),
                    E.coded_nbytes(means, stds, betas, cp, segment=segment), E.compress_to_budget(means, stds, cp, limit, betas=betas, segment=segment),
                    d7, E.CompressedEmbeddings(d7).rows([249, 0, 7]), E.compress_coordinates(means, stds, 17.0, codepoints=cp))
        return go
    hold(f"compressed_embeddings[segment={segment}]", setup)


@call("xi_encoder_and_mode_encoders")
def _():
    """utils.encode_vectorized (the g4 recipe of tests/test_gpu_stream_order.py) and utils.encode_mode_dp / encode_mode, which
    build their level tables in NumPy arrays of their own (utils.py:179-218), on the first cases of the g14 fixture."""
    import budget_reference as BR
    from vbq_amd import utils as U
    g14 = _golden("g14_budget_dp.npz")
    cases = list(BR.g14_cases(g14))[:2]
    z = np.random.default_rng(7).normal(0, 1.5, 301)
    sq, unsq = (lambda v: 1.0 / (1.0 + np.exp(-v))), (lambda e: np.log(e / (1 - e)))

    def go():
        out = [tuple(U.encode_vectorized(lambda zs: -0.5 * (zs - z) ** 2, z, 0.05, sq, unsq, max_bits_per_coord=9).items())]
        left, right = np.empty((10, 301)), np.empty((10, 301))
        U.get_all_N_bit_intervals(sq(z), 9, left, right)
        out += [left, right]
        for c in cases:
            f, squash, unsquash = BR.gaussian_callables(c["mu"], c["sigma"], c["prior_scale"])
            out.append(U.encode_mode_dp(f, c["mu"], c["N"], squash, unsquash, c["zero_bit_mode_hat"]))
            out.append(U.encode_mode(f, c["mu"], float(g14["em_lambdas"][0]), squash, unsquash, c["zero_bit_mode_hat"],
                                     max_bits_per_coord=int(g14["em_max_bits"])))
        return tuple(out)
    return go


class NumpyEncoderVAE(QH.StubVAE):
    """Its encoder wants the NumPy image: compress_replay captures from the latents on (mode "latents")."""

    def encode(self, X):
        if isinstance(X, torch.Tensor):
            raise TypeError("this encoder wants the NumPy image")
        return super().encode(X)


class NumpyVAE:
    """The FakeVAE of tests/test_gpu_api.py with latents that depend on the image: NumPy on both sides, no capture at all
    (mode "eager": compress + utils.evaluation_reads per image)."""

    def __init__(self, shape):
        stub = QH.StubVAE(shape)
        self.means, self.logvars = stub.means.cpu().numpy(), stub.logvars.cpu().numpy()

    def encode(self, X):
        return self.means + np.asarray(X, F32).mean(dtype=F32), self.logvars

    def decode(self, Z):
        Z = np.asarray(Z)
        return (0.1 * Z.mean(axis=-1, keepdims=True) + 0.5).repeat(3, axis=-1)


@call("compress_replay_in_its_other_modes")
def _():
    inp, _ = TSO.inputs_A()
    shape = QH.IMAGE_SHAPES[1]
    X = QH.image(shape)
    q = QH.fresh(A)

    def go():
        out = []
        for vae, mode in ((NumpyEncoderVAE(shape), "latents"), (NumpyVAE(shape), "eager")):
            out += [TSO._replay_answer(q, vae, x, inp.lambs) for x in (X, (0.5 * X).astype(F32), X)]
            rp = next(r for r in q._dev_cache["_replays"].values() if r.vae is vae)
            assert rp.mode == mode, (rp.mode, mode, rp.errors)
        # what the eager form does per image when the results stay on the device: compress + utils.evaluation_reads
        from vbq_amd import utils
        res = q.compress(X, QH.StubVAE(shape), inp.lambs)
        return tuple(out) + (utils.evaluation_reads(res, inp.lambs, {}),)
    return go


@call("encode_stage_above_one_gib")
def _():
    """The staging buffer of a batch above 1 GiB is pageable memory of the call's own (quantizer.py, _encode_stage); no batch
    of a test is that large, so the buffer is asked for directly.  Its contents are the plan's to write: only what it is
    is compared."""
    q = QH.fresh(A)

    def go():
        st = q._encode_stage((1 << 30) + 1)
        small = q._encode_stage(100)
        return st.numel(), str(st.dtype), bool(st.is_pinned()), small.numel(), bool(small.is_pinned())
    return go


@call("bmshj_inverse_cdf")
def _():
    xi = np.random.default_rng(4).uniform(0.02, 0.98, (37, CH)).astype(F32)

    def go():
        p = TSO._bmshj()
        return p.inverse_cdf(xi), p.inverse_cdf(dev(xi)), p.cdf(xi), p.pdf(dev(xi))
    return go


@call("metrics_from_numpy_images")
def _():
    from vbq_amd import metrics
    a, b = (t.cpu().numpy() for t in TSO._images(7, (2, 24, 20, 3)))
    return lambda: (metrics.mse(a, b), metrics.psnr(a, b), metrics.ms_ssim(a, b, weights=[0.3, 0.7]),
                    metrics.mse(a.astype(F32) / 255, b.astype(F32) / 255))


@call("coder_packed_forms")
def _():
    """RansCodec.pack_device / unpack_device / decode: the tail of the payload past `total` and the words of a segment past its size
    are left open (MASKS)."""
    from vbq_amd.coder import RansCodec
    idx = np.random.default_rng(7).integers(0, T4, (TSO.STREAMS, TSO.SYMS)).astype(np.uint16)

    def go():
        codec = RansCodec(TSO._freq(1, (TSO.STREAMS,)), N=N4, segment=TSO.SEG)
        words, sizes = codec.encode(dev(idx))
        payload, total, offsets = codec.pack_device(words, sizes)
        sz, packed = codec.encode_packed(dev(idx))
        w2, s2, status = codec.unpack_device(dev(packed), dev(sz.astype(np.uint16)), TSO.SYMS)
        return (words, sizes, payload, total, offsets, sz, packed, w2, s2, status, codec.decode(w2, s2, TSO.SYMS),
                codec.decode_packed(dev(packed), dev(sz.astype(np.uint16)), TSO.SYMS))
    return go


def _valid_words(words, sizes):
    """Padded words u16 [..., seg + 2] with everything past a segment's size set to 0."""
    keep = np.arange(words.shape[-1])[None, :] < sizes.reshape(-1).astype(np.int64)[:, None]
    return np.where(keep.reshape(words.shape), words, 0).astype(words.dtype)


def _mask_coder_packed_forms(got):
    got = list(got)
    total = int(got[3].astype(np.uint64)[0])
    got[2] = got[2][:total].copy()                                              # pack_device: the first `total` words are valid
    got[7] = _valid_words(got[7], got[8])                                       # unpack_device: words past a segment's size
    return tuple(got)


def _mask_nan_channel(got):
    """kmeans1d_dp -> (starts [S], codes [S], counts [S], sse, status): row 1 of every array is the NaN channel."""
    def cut(a):
        a = a.copy()
        a[1] = 0
        return a
    starts, codes, counts, sse, status = got
    assert all(1 <= int(s[1].min()) and int(s[1].max()) <= 257 for s in starts), "starts of the NaN channel outside [1, n]"
    return tuple(cut(a) for a in starts), tuple(cut(a) for a in codes), tuple(cut(a) for a in counts), cut(sse), status


MASKS = {"coder_packed_forms": _mask_coder_packed_forms, "kmeans1d_dp_with_a_nan_channel": _mask_nan_channel}
"""Call -> what sets the part its contract leaves open to a fixed value; the keys are those of dirty_memory.UNSPECIFIED."""


def test_masks_are_the_unspecified_parts():
    assert set(MASKS) == set(DM.UNSPECIFIED), sorted(set(MASKS) ^ set(DM.UNSPECIFIED))
    assert all(name in CALLS or name in TSO.CASES or name in QH.PROBES for name in MASKS)


@pytest.mark.parametrize("name", list(CALLS))
def test_call(name):
    hold(name, CALLS[name], MASKS.get(name))


# ---- ops.rans_encode_files / ops.rans_map_encode_files: given / fresh words x sizes
WORD, SIZE = 0xABCD, 0xFFFFFFFF
GIVEN = [(w, s) for w in (False, True) for s in (False, True)]


def _encode_files_batches():
    """A segment batch (tests/test_gpu_encode_files.py, "rows-and-tables") and a mapped one (tests/test_gpu_mapped_batch.py),
    each with the last listed segment taken off the list and two slots past the plan's: slots no item names."""
    import test_gpu_encode_files as TEF
    import test_gpu_mapped_batch as TMB
    rows, tables, n_tables, C_, seg, bits, canon = TEF.KERNEL_CASES["rows-and-tables"]
    k = TEF.Batch(rows, tables, n_tables, C_, seg, bits, seed=15, canon=canon, tight=True)
    m = TMB.fitted_batch(**TMB.MIXED, bits=bits, seed=11, tight=True)
    return k, m


def _unlisted(plan, C_):
    """(items with the last listed segment taken off, the slots of that segment in every channel)."""
    f, g = (int(v) for v in plan.items[plan.items[:, 0] >= 0][-1])
    items = plan.items.copy()
    items[np.flatnonzero((items[:, 0] == f) & (items[:, 1] == g))] = -1
    return items, [int(plan.seg_base[f]) + c * int(plan.nseg[f]) + g for c in range(C_)]


@pytest.mark.parametrize("mapped", [False, True], ids=["rans_encode_files", "rans_map_encode_files"])
@pytest.mark.parametrize("given_words,given_sizes", GIVEN, ids=[f"words-{'given' if w else 'fresh'}-sizes-{'given' if s else 'fresh'}"
                                                                 for w, s in GIVEN])
def test_encode_files_given_and_fresh_outputs(mapped, given_words, given_sizes):
    """"slots no item names keep what `words` / `sizes` held (new ones are zeroed)": under every fill a fresh `words` / `sizes` is
    zero in the unlisted slots and a given one holds the caller's WORD / SIZE there, whatever the other one is; the listed
    slots equal the answer with both given (the form tests/test_gpu_encode_files.py holds against the checker)."""
    from vbq_amd import ops
    k, m = _encode_files_batches()
    b = m if mapped else k
    items, off = _unlisted(b.plan, b.C)
    M = b.plan.M + 2
    untouched = np.array(off + [b.plan.M, b.plan.M + 1])
    listed = np.setdiff1d(np.arange(M), untouched)

    def run(words, sizes):
        d_items = torch.from_numpy(items).cuda()
        files = torch.from_numpy(b.files).cuda()
        if mapped:
            return ops.rans_map_encode_files(b.d_idx, b.d_cls, files, torch.from_numpy(b.pal_rows).cuda(), d_items, b.d_freq, M, seg=b.seg,
                                             max_classes=b.max_classes, N=b.bits, canon=b.d_canon, words=words, sizes=sizes)
        return ops.rans_encode_files(b.d_idx, files, d_items, b.d_freq, M, seg=b.seg, N=b.bits, canon=b.d_canon, words=words, sizes=sizes)

    def setup():
        def go():
            words = torch.from_numpy(np.full((M, b.seg + 2), WORD, np.uint16)).cuda() if given_words else None
            sizes = torch.from_numpy(np.full(M, SIZE, np.uint32)).cuda() if given_sizes else None
            return run(words, sizes)
        return go

    # (nothing is masked: "Slots that no item names, and the words of a slot past its size, are left untouched", include/vbq.h --
    # they hold WORD in a given buffer and 0 in a fresh one)
    answers = four_answers("encode_files", setup)
    both = SO.plain(run(torch.from_numpy(np.full((M, b.seg + 2), WORD, np.uint16)).cuda(), torch.from_numpy(np.full(M, SIZE, np.uint32)).cuda()))
    both = (both[0].view(np.uint16), both[1].view(np.uint32))
    for byte, (words, sizes, status) in answers.items():
        where = f"{_tag(byte)}, words {'given' if given_words else 'fresh'}, sizes {'given' if given_sizes else 'fresh'}"
        words, sizes = words.view(np.uint16), sizes.view(np.uint32)              # (plain answers hold unsigned tensors as signed views)
        assert not status.any(), where
        assert np.array_equal(sizes[listed], both[1][listed]), where
        assert np.array_equal(_valid_words(words[listed], sizes[listed]), _valid_words(both[0][listed], both[1][listed])), where
        past = np.arange(b.seg + 2)[None, :] >= sizes[listed].astype(np.int64)[:, None]
        assert np.all(words[listed][past] == (WORD if given_words else 0)), f"{where}: words past a slot's size"
        assert np.all(words[untouched].view(np.uint16) == (WORD if given_words else 0)), \
            f"{where}: unlisted slots of words hold {np.unique(words[untouched].view(np.uint16))[:4]}"
        assert np.all(sizes[untouched].view(np.uint32) == (SIZE if given_sizes else 0)), \
            f"{where}: unlisted slots of sizes hold {np.unique(sizes[untouched].view(np.uint32))[:4]}"
    assert not differences("encode_files", answers)


# ====================================================================================================== d. state built on dirty memory
HALF = QH.State("half", None, "A", QH.LAMBS_A, 0.5, None)
"""Smoothing 0.5 cannot be tabulated: both -log2 steps of the build are host stages (pinned staging of their own)."""


def _built(state, byte, tmp):
    with _fill(byte):
        q = QH.fresh(state)
        lambs = list(q.lambs)
        path = os.path.join(tmp, f"{state.name}_{_tag(byte)}.npz")
        q.save(path)
        with np.load(path, allow_pickle=False) as z:
            saved = tuple((k, z[k]) for k in sorted(z.files))
        out = (q.all_code_points, q.code_points_by_channel, q._search_grids, tuple(np.concatenate(c) for c in q.code_points_by_bits),
               tuple(np.asarray(q.entropy_models[l]) for l in lambs), tuple(np.asarray(q.raw_code_length_entropy_models[l]) for l in lambs),
               tuple(np.asarray(q._code_counts[l]) for l in lambs), saved)
        out = SO.plain(out)
        torch.cuda.synchronize()
    return q, out


@pytest.mark.parametrize("state", [A, HALF, QH.STATES["E"], QH.STATES["R"]], ids=lambda s: s.name)
def test_quantizer_built_under_a_fill(state, tmp_path):
    """Tables, both model dicts, _code_counts and every array of the saved .npz equal those of a quantizer built unpatched; then
    the quantizer built on dirty memory writes the files and answers the latents probe of one built unpatched."""
    inp, _ = TSO.inputs_A()
    q0, want = _built(state, None, str(tmp_path))
    probes = ("latents", "to_bytes", "to_bytes_c", "to_bytes_mapped", "codec")
    asked = {p: SO.plain(QH.outcome(QH.PROBES[p], q0, inp)) for p in probes}
    for byte in DM.FILLS:
        q, got = _built(state, byte, str(tmp_path))
        assert QH.same(got, want), f"state {state.name} built under {_tag(byte)}: {DM.first_difference(got, want)}"
        for p in probes:
            with DM.Fill(byte):
                ans = SO.plain(QH.outcome(QH.PROBES[p], q, inp))
            assert QH.same(ans, asked[p]), f"{p} on state {state.name} built under {_tag(byte)}: {DM.first_difference(ans, asked[p])}"
        type(q).load(os.path.join(str(tmp_path), f"{state.name}_{_tag(byte)}.npz"))


BUILD_ROWS, BUILD_LAMBDAS = TSO.BUILD_ROWS, TSO.BUILD_LAMBDAS


def _build_answer(b, x):
    b.run(x[0], x[1])
    out = SO.plain((b.level_counts, b.level_len, b.counts, b.raw_models, b.models))
    b.check()
    return out


@pytest.mark.parametrize("n_chunks,smoothing,python_stage", [(1, 0, False), (2, 0, False), (1, 1, False), (2, 1, False),
                                                             (1, 0.5, False), (2, 0.5, False), (1, 0.5, True)])
def test_entropy_model_build_under_a_fill(n_chunks, smoothing, python_stage):
    """A new object under every fill, and ONE object run again under each fill on the OTHER latents: what it reuses (index
    planes, workspace, histograms, staging) then holds a real previous answer."""
    from vbq_amd.pipeline import EntropyModelBuild
    tab = TSO.tables(N4)[0]
    new = lambda: EntropyModelBuild(BUILD_ROWS, CH, BUILD_LAMBDAS, tab, N=N4, n_chunks=n_chunks, add_n_smoothing=smoothing,
                                    python_host_stage=python_stage)
    xs = {seed: TSO.pair(seed, BUILD_ROWS, planes=True) for seed in (7, 8)}
    want = {seed: _build_answer(new(), xs[seed]) for seed in xs}
    assert not QH.same(want[7], want[8])
    shared = None
    for k, byte in enumerate(DM.FILLS + DM.FILLS):
        seed = (7, 8)[k % 2]
        with DM.Fill(byte):
            b = new()
            assert (b.side is not None) == (n_chunks == 2) and (smoothing != 0.5 or b.has_host_stages)
            assert not python_stage or b.host_stage_kind == "python"
            got = _build_answer(b, xs[seed])
            again = _build_answer(shared, xs[seed]) if shared is not None else got
            torch.cuda.synchronize()
        shared = shared or b
        assert QH.same(got, want[seed]), f"a new build under {_tag(byte)}: {DM.first_difference(got, want[seed])}"
        assert QH.same(again, want[seed]), f"run {k + 1} of one build, under {_tag(byte)}: {DM.first_difference(again, want[seed])}"


def test_entropy_model_build_in_one_call_under_a_fill():
    from vbq_amd.pipeline import EntropyModelBuild
    tab = TSO.tables(N4)[0]

    def setup():
        x = TSO.pair(7, BUILD_ROWS)

        def go():
            b = EntropyModelBuild(BUILD_ROWS, CH, BUILD_LAMBDAS, tab, N=N4)
            b.run_one_call(x[0], x[1])
            return b.level_counts, b.level_len, b.counts, b.raw_models, b.models
        return go
    hold("build_entropy_models", setup)


@pytest.mark.parametrize("byte", DM.FILLS)
def test_single_file_and_batch_writers_agree_under_a_fill(byte):
    """VBQb, VBQc and VBQm: file f of the batch writer is the one-file writer's file, byte for byte, both under the fill."""
    inp, dinp = TSO.inputs_A()
    q = QH.fresh(A)
    with DM.Fill(byte):
        for i in (inp, dinp):
            batch = {"b": QH.b_to_bytes(q, i)[0], "c": QH.b_compact(q, i)[0], "m": QH.b_mapped(q, i)[0]}
            for kind, files in batch.items():
                for f in range(len(i.files)):
                    one = QH.written(q, i, kind, f)
                    assert bytes(files[f]) == bytes(one), f"{_tag(byte)}, {i.form}: file {f} of the {kind!r} batch writer differs " \
                                                           f"from the one-file writer ({DM.first_difference(bytes(files[f]), bytes(one))})"


# ====================================================================================================== g. the control
def test_control_a_missing_zero_fill_is_seen(monkeypatch):
    """zero_ a no-op around run(): pass 1 adds its bit-length histogram onto whatever level_counts held.  Fresh memory that reads
    as zero hides it; 0x01 and 0x3C do not."""
    from vbq_amd.pipeline import EntropyModelBuild
    tab = TSO.tables(N4)[0]
    x = TSO.pair(7, BUILD_ROWS, planes=True)

    def level_counts(byte, broken):
        with _fill(byte):
            b = EntropyModelBuild(BUILD_ROWS, CH, BUILD_LAMBDAS, tab, N=N4, n_chunks=1, add_n_smoothing=1)
            with monkeypatch.context() as m:
                if broken:
                    m.setattr(torch.Tensor, "zero_", lambda self: self)
                b.run(x[0], x[1])
            out = SO.plain((b.level_counts,))
            torch.cuda.synchronize()
        return out
    want = level_counts(None, False)
    seen = {byte: not QH.same(level_counts(byte, True), want) for byte in DM.FILLS}
    assert QH.same(level_counts(0x3C, False), want)
    assert seen[0x01] and seen[0x3C] and not seen[0x00], \
        f"THE CONTROL DID NOT FIRE: a histogram added onto unzeroed memory went unnoticed ({seen}) -- this module is testing nothing"
    base = int(np.frombuffer(bytes([0x3C]) * 8, np.int64)[0])
    assert np.array_equal(level_counts(0x3C, True)[0] - base, want[0])           # a wrong value and nothing else


def test_control_a_call_that_returns_fresh_memory_is_reported():
    def setup():
        return lambda: torch.empty(4, device="cuda")
    answers = four_answers("fake", setup)
    lines = differences("fake", {**answers, None: answers[0]})
    assert len(lines) == 2 and lines[0].startswith("fake under Fill(0x01) differs") and "answer[0]" in lines[0], \
        f"THE CONTROL DID NOT FIRE: a call returning torch.empty(4) was not reported ({lines}) -- this module is testing nothing"
    with pytest.raises(AssertionError, match="fake under Fill"):
        hold("fake", lambda: (lambda: np.empty(3)))


# ====================================================================================================== f. coverage (the last test)
def test_zz_every_allocation_site_is_reached_or_explained():
    sites, reached = DM.allocation_sites(), DM.sites_reached()
    print(f"\n[test_gpu_dirty_memory] {len(sites)} allocation sites, {len(sites & reached)} reached under a fill, "
          f"{len(DM.EXEMPT_SITES)} exempt")
    missing = sorted(sites - reached - set(DM.EXEMPT_SITES))
    assert not missing, "allocation sites no call of this module reaches and dirty_memory.EXEMPT_SITES does not explain (add a " \
                        "call to section c):\n" + "\n".join(f"vbq_amd/{f}:{line}" for f, line in missing)
