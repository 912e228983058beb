"""Byte budgets over batches of compact files on the GPU: coded_nbytes_compact_batch / compress_latents_to_compact_budget_batch
/ compress_latents_to_compact_total_budget / compress_to_compact_budget_batch against the loop of the one-file calls
(coded_nbytes / compress_latents_to_budget with layout="interleaved"): dicts == dicts and bytes == bytes -- mixed shapes and
parts, repeated code points, the lambdas in chunks, and the writers sizing nothing a second time."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from vbq_amd import bitstream as bs  # noqa: E402

pytestmark = pytest.mark.gpu
N, C_ = 10, 32
LAMBS = [2.0 ** -6, 2.0 ** -2, 2.0, 16.0]
SHAPES = [(1, 32, 48, C_), (1, 20, 30, C_), (2, 5, 7, C_), (3, C_), (1, 1, 1, C_)]
PARTS = [64, 1000, 1 << 17]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")


def _gaussian_quantizer(C, seed):
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), C))
    q = ChannelwisePriorCDFQuantizer(C, N)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), scale))
    return q, scale, rng


def _latents(rng, scale, shape):
    m = (scale * rng.standard_normal(shape)).astype(np.float32)
    lv = (2 * (-2 + 0.7 * rng.standard_normal(shape))).astype(np.float32)
    return m, lv


def _on_device(lat):
    return [(torch.from_numpy(m).cuda(), torch.from_numpy(lv).cuda()) for m, lv in lat]


class Shared:
    """The quantizer, the five latents and the one-file results, each one-file call made once and never changed."""

    def __init__(self):
        self.q, scale, rng = _gaussian_quantizer(C_, 11)
        self.lat = [_latents(rng, scale, s) for s in SHAPES]
        self.q.build_entropy_models_from_latents(self.lat[0][0].reshape(-1, C_), self.lat[0][1].reshape(-1, C_), LAMBS,
                                                 add_n_smoothing=1, spread="logvar")
        assert self.q._strict
        self._cache = {}

    def lengths(self, part):
        """[coded_nbytes(latent f, LAMBS, layout="interleaved", part=part) for f]."""
        key = ("nbytes", part)
        if key not in self._cache:
            self._cache[key] = [self.q.coded_nbytes(m, lv, LAMBS, layout="interleaved", part=part) for m, lv in self.lat]
        return self._cache[key]

    def budget_loop(self, part, budgets):
        out = []
        for f, budget in enumerate(budgets):
            key = ("budget", f, int(budget), part)
            if key not in self._cache:
                self._cache[key] = self.q.compress_latents_to_budget(*self.lat[f], int(budget), LAMBS, layout="interleaved",
                                                                     part=part)
            out.append(self._cache[key])
        return out

    def files_at(self, part, lamb):
        key = ("files", part, lamb)
        if key not in self._cache:
            self._cache[key] = [self.q.compress_latents_to_bytes(m, lv, lamb, layout="interleaved", part=part) for m, lv in self.lat]
        return self._cache[key]


@pytest.fixture(scope="module")
def shared():
    return Shared()


def _same_tables(got, want):
    """dict == dict, file by file, the keys in the same order."""
    assert isinstance(got, list) and len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, dict) and list(g) == list(w), f
        assert g == w, (f, g, w)
        assert all(type(v) is int for v in g.values()), f


def _same_files(got, want):
    assert isinstance(got, list) and len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, bytes)
        if g != w:
            first = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
            pytest.fail(f"file {f}: {len(g)} bytes against {len(w)} (lambda {bs.parse_compact(g)[0].lamb} against "
                        f"{bs.parse_compact(w)[0].lamb}), first difference at byte {first}")


def _chosen(files):
    return [bs.parse_compact(data)[0].lamb for data in files]


@pytest.mark.parametrize("part", PARTS)
def test_lengths_of_a_batch_equal_the_list_of_one_file_lengths(shared, part):
    q, lat = shared.q, shared.lat
    want = shared.lengths(part)
    _same_tables(q.coded_nbytes_compact_batch(lat, LAMBS, part=part), want)
    _same_tables(q.coded_nbytes_compact_batch(_on_device(lat), LAMBS, part=part), want)
    _same_tables(q.coded_nbytes_compact_batch(lat, part=part), [{k: w[k] for k in q.lambs} for w in want])     # lambs=None
    picked = [LAMBS[2], LAMBS[0], LAMBS[2]]                       # an order of the caller's, a repeat: each key once, in order
    _same_tables(q.coded_nbytes_compact_batch(lat[1:3], picked, part=part),
                 [{k: w[k] for k in (LAMBS[2], LAMBS[0])} for w in want[1:3]])
    # a length is the length of the file
    assert want[1][LAMBS[1]] == len(shared.files_at(part, LAMBS[1])[1])


def test_the_default_part_is_the_one_file_default(shared):
    q, lat = shared.q, shared.lat
    _same_tables(q.coded_nbytes_compact_batch(lat[:2], LAMBS), [q.coded_nbytes(m, lv, LAMBS, layout="interleaved") for m, lv in lat[:2]])


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("which", ["median", "smallest", "largest", "mixed"])
def test_per_file_budgets_equal_the_loop_of_one_file_budget_calls(shared, part, which):
    q, lat = shared.q, shared.lat
    nb = shared.lengths(part)
    pick = {"median": lambda v: int(np.median(v)), "smallest": min, "largest": max}
    # taken from the lengths: the loop stays within them.  mixed: the three kinds in turn from file to file
    kinds = [which if which != "mixed" else ("largest", "smallest", "median")[f % 3] for f in range(len(nb))]
    budgets = [pick[kind](list(t.values())) for kind, t in zip(kinds, nb)]
    want = shared.budget_loop(part, budgets)
    if which == "mixed":
        assert len(set(_chosen(want))) >= 2                       # (not a test that passes by coding everything at one rate)
    got = q.compress_latents_to_compact_budget_batch(lat, budgets, LAMBS, part=part)
    _same_files(got, want)
    assert all(len(g) <= b for g, b in zip(got, budgets))
    _same_files(q.compress_latents_to_compact_budget_batch(_on_device(lat), np.array(budgets), LAMBS, part=part), want)
    back = q.decompress_latents_compact_batch(got, stack=False)
    for g, z, shape in zip(got, back, SHAPES):
        assert tuple(z.shape) == shape
        assert np.array_equal(z.cpu().numpy().view(np.uint32), np.asarray(q.decompress_latents(g), np.float32).view(np.uint32))


def test_one_budget_for_all_files(shared):
    q, lat, part = shared.q, shared.lat, 1000
    nb = shared.lengths(part)
    budget = max(min(t.values()) for t in nb) + 40                # every file has a fit; the large ones only at large lambdas
    want = shared.budget_loop(part, [budget] * len(lat))
    assert len(set(_chosen(want))) >= 2
    _same_files(q.compress_latents_to_compact_budget_batch(lat, budget, LAMBS, part=part), want)
    _same_files(q.compress_latents_to_compact_budget_batch(lat, np.int64(budget), LAMBS, part=part), want)


def test_a_file_that_nothing_fits_raises_before_anything_is_encoded(shared, monkeypatch):
    from vbq_amd import ops
    q, lat, part = shared.q, shared.lat, 64
    nb = shared.lengths(part)
    budgets = [max(t.values()) for t in nb]
    least = min(nb[2].values())
    budgets[2] = least - 1
    calls = []
    real = ops.rans_il_encode_files
    monkeypatch.setattr(ops, "rans_il_encode_files", lambda *a, **k: calls.append(1) or real(*a, **k))
    with pytest.raises(ValueError, match=rf"file 2: no lambda fits in {least - 1} bytes: the smallest file is {least} bytes"):
        q.compress_latents_to_compact_budget_batch(lat, budgets, LAMBS, part=part)
    assert calls == []
    with pytest.raises(ValueError, match="file 0: no lambda fits in 1 bytes"):
        q.compress_latents_to_compact_budget_batch(lat, 1, LAMBS, part=part)
    assert calls == []
    budgets[2] = least                                            # (the counter counts: with a fit there is one encode launch)
    q.compress_latents_to_compact_budget_batch(lat, budgets, LAMBS, part=part)
    assert calls == [1]


def test_total_budget_takes_one_lambda_for_all_files(shared):
    q, lat, part = shared.q, shared.lat, 1000
    nb = shared.lengths(part)
    sums = {k: sum(t[k] for t in nb) for k in LAMBS}
    assert len(set(sums.values())) == len(LAMBS)
    for budget in (sums[LAMBS[2]], sums[LAMBS[2]] - 1, 10 * sums[LAMBS[0]]):
        lamb, files = q.compress_latents_to_compact_total_budget(lat, budget, LAMBS, part=part)
        assert lamb == bs.smallest_rate_within(sums, budget)
        assert sum(len(f) for f in files) == sums[lamb] <= budget
        _same_files(files, q.compress_latents_to_compact_batch(lat, lamb, part))
        _same_files(files, shared.files_at(part, lamb))
    with pytest.raises(ValueError, match=rf"no lambda fits in 1 bytes: the smallest file is {min(sums.values())} bytes"):
        q.compress_latents_to_compact_total_budget(lat, 1, LAMBS, part=part)
    with pytest.raises(ValueError, match="no files"):
        q.compress_latents_to_compact_total_budget([], 10 ** 9, LAMBS, part=part)


def test_the_budget_writers_size_nothing_twice(shared, monkeypatch):
    from vbq_amd import ops
    q, lat, part = shared.q, shared.lat, 64
    nb = shared.lengths(part)
    budgets = [int(np.median(list(t.values()))) for t in nb]
    want = shared.budget_loop(part, budgets)
    sums = {k: sum(t[k] for t in nb) for k in LAMBS}
    real = ops.rans_il_sizes_files
    monkeypatch.setattr(ops, "rans_il_sizes_files", lambda *a, **k: pytest.fail("the parts were sized a second time"))
    _same_files(q.compress_latents_to_compact_budget_batch(lat, budgets, LAMBS, part=part), want)
    lamb, files = q.compress_latents_to_compact_total_budget(_on_device(lat), sums[LAMBS[1]], LAMBS, part=part)
    assert lamb == bs.smallest_rate_within(sums, sums[LAMBS[1]])
    _same_files(files, shared.files_at(part, lamb))
    # the writer with given lambdas keeps its launches: it sizes its parts itself, once
    calls = []
    monkeypatch.setattr(ops, "rans_il_sizes_files", lambda *a, **k: calls.append(1) or real(*a, **k))
    _same_files(q.compress_latents_to_compact_batch(lat, LAMBS[1], part), shared.files_at(part, LAMBS[1]))
    assert calls == [1]


def test_one_lambda_per_chunk_gives_the_same_table(shared, monkeypatch):
    from vbq_amd import ops, quantizer
    q, lat, part = shared.q, shared.lat, 1000
    want = shared.lengths(part)
    launches = []
    real = ops.rans_il_rates_files
    monkeypatch.setattr(ops, "rans_il_rates_files", lambda *a, **kw: launches.append(kw["sizes"].shape[0]) or real(*a, **kw))
    _same_tables(q.coded_nbytes_compact_batch(lat, LAMBS, part=part), want)
    assert launches == [len(LAMBS)]                               # unchunked: ONE rate launch
    del launches[:]
    monkeypatch.setattr(quantizer, "RATE_SCRATCH_BYTES", 1)
    _same_tables(q.coded_nbytes_compact_batch(lat, LAMBS, part=part), want)
    assert launches == [1] * len(LAMBS)
    budgets = [int(np.median(list(t.values()))) for t in want]
    _same_files(q.compress_latents_to_compact_budget_batch(lat, budgets, LAMBS, part=part), shared.budget_loop(part, budgets))


def test_repeated_code_points():
    """The non-strict path: the rate kernel and the writer map a rank to the canonical rank of its run of equal code points."""
    from scipy.stats import norm
    from vbq_amd import ChannelwisePriorCDFQuantizer

    class Coarse:
        def inverse_cdf(self, xi):
            return np.round(norm.ppf(xi) * np.array([24.0, 64.0])) / np.array([24.0, 64.0])
    q = ChannelwisePriorCDFQuantizer(2, N)
    q.build_code_points(Coarse())
    assert not q._strict
    rng = np.random.default_rng(21)
    shapes = [(1, 40, 50, 2), (7, 9, 2), (1, 2)]
    lat = [(rng.normal(0, 1.1, s).astype(np.float32), (2 * rng.normal(-2, 0.7, s)).astype(np.float32)) for s in shapes]
    lambs = [0.01, 0.3, 4.0]
    q.build_entropy_models_from_latents(lat[0][0].reshape(-1, 2), lat[0][1].reshape(-1, 2), lambs, add_n_smoothing=1, spread="logvar")
    for part in (64, 1000):
        want = [q.coded_nbytes(m, lv, lambs, layout="interleaved", part=part) for m, lv in lat]
        _same_tables(q.coded_nbytes_compact_batch(lat, lambs, part=part), want)
        budgets = [want[0][lambs[1]], want[1][lambs[2]], want[2][lambs[0]]]
        _same_files(q.compress_latents_to_compact_budget_batch(lat, budgets, lambs, part=part),
                    [q.compress_latents_to_budget(m, lv, b, lambs, layout="interleaved", part=part) for (m, lv), b in zip(lat, budgets)])


def test_refusals_before_any_launch(shared, monkeypatch):
    from vbq_amd import ops
    q, lat = shared.q, shared.lat
    import inspect
    wrappers = [n for n, f in vars(ops).items() if inspect.isfunction(f) and f.__module__ == ops.__name__
                and "_lib.lib()" in inspect.getsource(f)]       # every function of ops that calls the library
    assert {"rans_il_rates_files", "rans_il_sizes_files", "rans_il_encode_files", "prep_planes"} <= set(wrappers)
    for name in wrappers:
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("a kernel was launched"))
    bad_pair = (lat[1][0], lat[1][1][..., :-1])
    calls = (lambda **kw: q.coded_nbytes_compact_batch(kw.pop("latents", lat[:2]), kw.pop("lambs", LAMBS), **kw),
             lambda **kw: q.compress_latents_to_compact_budget_batch(kw.pop("latents", lat[:2]), kw.pop("budget", 10 ** 6),
                                                                     kw.pop("lambs", LAMBS), **kw),
             lambda **kw: q.compress_latents_to_compact_total_budget(kw.pop("latents", lat[:2]), kw.pop("budget", 10 ** 6),
                                                                     kw.pop("lambs", LAMBS), **kw))
    for call in calls:
        for part in (0, -3, (1 << 24) + 1):
            with pytest.raises(ValueError, match="part"):
                call(part=part)
        with pytest.raises(ValueError, match="file 1: expected channel-last"):
            call(latents=[lat[0], bad_pair])
        with pytest.raises(ValueError, match="file 1: expected a pair"):
            call(latents=[lat[0], (lat[1][0],)])
        with pytest.raises(KeyError):
            call(lambs=[LAMBS[0], 3.0])
    with pytest.raises(ValueError, match="3 budgets for 2 files"):
        q.compress_latents_to_compact_budget_batch(lat[:2], [100, 100, 100], LAMBS)
    with pytest.raises(ValueError, match="1 budgets for 2 files"):
        q.compress_latents_to_compact_budget_batch(lat[:2], [100], LAMBS)
    for budget in (0, [100, 0], -5):
        with pytest.raises(ValueError, match="at least one byte"):
            q.compress_latents_to_compact_budget_batch(lat[:2], budget, LAMBS)
    with pytest.raises(ValueError, match="at least one byte"):
        q.compress_latents_to_compact_total_budget(lat[:2], 0, LAMBS)
    with pytest.raises(TypeError):
        q.compress_latents_to_compact_budget_batch(lat[:2], 100.0, LAMBS)
    # no files
    assert q.coded_nbytes_compact_batch([], LAMBS) == [] and q.compress_latents_to_compact_budget_batch([], 100, LAMBS) == []
    assert q.compress_to_compact_budget_batch([], None, 100) == []
    # the segment-file batch calls still refuse a compact file, and take no part
    with pytest.raises(TypeError):
        q.coded_nbytes_batch(lat[:2], LAMBS, part=64)


def test_compress_to_compact_budget_batch_encodes_every_image(shared):
    q, lat, part = shared.q, shared.lat, 64
    nb = shared.lengths(part)

    class Stored:
        """A stand-in VAE: `encode(i)` returns the stored latents of image i."""
        def encode(self, i):
            return lat[i]
    order = [4, 0, 2]
    budgets = [nb[4][LAMBS[0]], nb[0][LAMBS[1]], max(nb[2][LAMBS[2]] - 1, min(nb[2].values()))]
    want = [q.compress_to_budget(i, Stored(), b, LAMBS, layout="interleaved", part=part) for i, b in zip(order, budgets)]
    _same_files(q.compress_to_compact_budget_batch(order, Stored(), budgets, LAMBS, part=part), want)
    _same_files(q.compress_latents_to_compact_budget_batch([lat[i] for i in order], budgets, LAMBS, part=part), want)
