"""No kernel's answer depends on what the LDS held (tests/lds_state.py says how the fill works, why these bytes, and where a new
kernel is enrolled).

A CASE launches catalogued kernels through the C entry points, at the smallest shapes at which their LDS paths are live, and is
answered four times: as the process found the LDS, and with lds_fill(0x00), (0x01), (0x3C) enqueued on the call's own stream
directly before EVERY entry-point call of the case (lds_state.Polluted).  Each answer is held, bit for bit, to the reference the
kernel's own test module uses -- the case bodies ARE the runners of those modules (tests/test_gpu_write_footprint.py for most:
the C oracle, NumPy, tests/*_reference.py), imported, not copied; they assert their regime with tests/launch_plans.py before the
launch (solve_kernel, notebook_kernel, transpose_kernel, gather_kernel, np_sums_first_kernel, the *_plan and *_grid rules), in
the runner or in the case.  On top of that every guarded output a case creates (footprint.Guarded, through the footprint module's
G) and whatever the case returns is recorded, and the four recordings must be the same bits: this is what holds the outputs of
the footprint module's runners that a reference bounds only within a tolerance, and hold() asserts that such a recording is not
empty.  The cases marked `recorded=False` use runners of other modules alone, which hand nothing back: there the four answers
are equal because each is compared EXACTLY (np.array_equal on integer views of the bits) with one and the same reference, and
the case's docstring names that comparison.  After the readback assert_covered() proves that every fill of the case reached
every CU, and the case asserts that the entry points it is catalogued for were called.

Multi-workgroup f64 atomic sums have no fixed order of additions: those cases (`bitwise=False`) are held to the tolerance their
own modules use, and the same kernels have a case with ONE workgroup per output (and for k_moments_bc one lane per output)
where the sum is a fixed sequence and is compared bit for bit.

Only the first LDS-using launch of an entry point sees the fill; lds_state.EXEMPT names the kernels no entry point launches
first.  vbq_compress_latents_f32 and vbq_build_entropy_models_f32 are sequences of the kernels catalogued here through their
single-launch entry points; Python-level calls are sequences of entry points and out of scope.

CONTROLS: the LDS carries over (pollute, then lds_probe: every byte of every workgroup, every CU); the comparison sees a
dependence (lds_toy, a deliberately wrong kernel, under the three fills: three different answers, reported by the case
machinery); the fill disturbs nothing else (a guarded output and a guarded bystander around a polluted call).  If a control
does not fire the module tests nothing, and says so.

What the module found and what it costs: EXPERIMENTS.md, "LDS carry-over"; the fixture below prints the figures of every run."""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import footprint as FP  # noqa: E402
import launch_plans as LP  # noqa: E402
import lds_state as LS  # noqa: E402
import test_gpu_write_footprint as WF  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
_STATS = {"cases": 0, "fills": 0}


@pytest.fixture(scope="module", autouse=True)
def _library(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    LS.load(LS.compile_library(str(tmp_path_factory.mktemp("lds_fill"))))
    t0 = time.perf_counter()
    yield
    print(f"\n[test_gpu_lds_state] {time.perf_counter() - t0:.1f} s; {_STATS['cases']} cases, {_STATS['fills']} fills, every one on "
          f"{LS.cu_count()} of {LS.cu_count()} CUs")


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """A device error is not a wrong answer: after one, nothing more of this module is launched."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"device error, the rest of the module is not run: {e}", returncode=3)
    WF._LIVE.clear()
    del LS._PENDING[:]


@pytest.fixture(scope="module")
def env():
    from vbq_amd import _lib, ops

    class Env:
        pass
    e = Env()
    e.ops, e.lib = ops, _lib.lib()
    return e


# ====================================================================================================== the harness
class Recording:
    """Every footprint.Guarded made through the footprint module's G while this is active, in the order they were made."""

    def __enter__(self):
        self.made, self._real = [], WF.G

        def G(*args, **kw):
            g = self._real(*args, **kw)
            self.made.append(g)
            return g
        WF.G = G
        return self

    def __exit__(self, *exc):
        WF.G = self._real
        return False

    def payloads(self):
        return tuple(g.bits().copy() for g in self.made)


def _plain(x):
    if isinstance(x, torch.Tensor):
        a = x.detach().cpu().contiguous()
        a = a.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]) if a.numel() else a
        return a.numpy()
    if isinstance(x, (tuple, list)):
        return tuple(_plain(v) for v in x)
    return x


def _tag(byte):
    return "the LDS as the process found it" if byte is None else f"lds_fill(0x{byte:02X})"


def four_answers(go, entries=(), direct=False):
    """go() as found and under each fill -> {None | byte: (what go returned, every recorded guarded output)}.  `direct`: the fill
    is enqueued here, on the current stream, and not by the entry-point wrappers (for a `go` that calls no product entry point)."""
    out = {}
    for byte in (None,) + LS.FILLS:
        with LS.Polluted(byte) as p, Recording() as rec:
            if direct and byte is not None:
                LS.pollute(byte)
            got = _plain(go())
            torch.cuda.synchronize()
            out[byte] = (got, rec.payloads())
        missing = [e for e in entries if not p.calls.get(e)]
        assert not missing, f"{_tag(byte)}: the case never called {missing}"
        if not direct:
            assert byte is None or len(LS._PENDING) == sum(p.calls.values()), (len(LS._PENDING), p.calls)
        _STATS["fills"] += LS.assert_covered()                      # after the readback: every fill of this run reached every CU
        WF._LIVE.clear()
    return out


def _first_difference(a, b, path="answer"):
    if isinstance(a, tuple) and isinstance(b, tuple):
        if len(a) != len(b):
            return f"{path}: {len(a)} against {len(b)} entries"
        for k, (x, y) in enumerate(zip(a, b)):
            d = _first_difference(x, y, f"{path}[{k}]")
            if d:
                return d
        return None
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray):
        try:
            WF.same(a, b, path)                                     # the footprint module's comparison: dtype, shape, every bit
        except AssertionError as e:
            return str(e)
        return None if a.dtype == b.dtype else f"{path}: {a.dtype} against {b.dtype}"
    return None if (type(a) is type(b) and a == b) else f"{path}: {a!r} against {b!r}"


def differences(name, answers):
    """One line per fill whose answer is not the one the process's own LDS gave."""
    want, lines = answers[None], []
    for byte in LS.FILLS:
        d = _first_difference(answers[byte], want)
        if d:
            zero = "" if byte == 0 or not _first_difference(answers[0], want) else " (a zeroed LDS differs as well)"
            lines.append(f"{name} under {_tag(byte)} differs from the answer on {_tag(None)}{zero}: {d}")
    return lines


def hold(name, go, entries=(), bitwise=True, direct=False, recorded=True):
    answers = four_answers(go, entries, direct)
    if bitwise:
        if recorded:
            empty = [_tag(b) for b, (got, made) in answers.items() if got is None and not made]
            assert not empty, f"{name}: nothing was recorded on {empty} -- the comparison of the four answers would compare nothing"
        bad = differences(name, answers)
        assert not bad, "\n".join(bad)
    _STATS["cases"] += 1
    return answers


# ====================================================================================================== the cases
CASES = {}


def case(name, kernels, entries, bitwise=True, recorded=True):
    """Register go(env) under `name`: it launches `kernels` (each FIRST in one of `entries`) and holds every output to its
    reference itself.  recorded=False: the runners hand nothing back, their own comparison with the reference is exact (the
    docstring says which).  lds_state.COVERED lists the same (kernel, case) pairs; test_the_cases_are_the_catalogue compares."""
    def deco(fn):
        assert name not in CASES, name
        assert recorded or (bitwise and "exact" in (fn.__doc__ or "")), name
        CASES[name] = (tuple(kernels), tuple(entries), bool(bitwise), fn, bool(recorded))
        return fn
    return deco


FAST3, LAM32 = WF.FAST3, WF.LAM32
QUANTIZE, COUNTS = ("vbq_quantize_f32",), ("vbq_level_counts_f32",)


# ---- the solve family: ops.quantize / ops.level_counts, one launch each (k_prepare_penalties of the literal kernels has no LDS)
@case("solve_fast_indices", ["k_quant_fast"], QUANTIZE)
def _(e):
    """K1<0>: tb[], scratch[] and penl[] at one full 512-element workgroup plus one element, N = 10 and N = 4 (T = 31)."""
    WF.run_solve(e.ops, e.lib, 513, 3, FAST3, "K1<0>")
    WF.run_solve(e.ops, e.lib, 513, 3, FAST3, "K1<0>", layout="bc->cb")
    WF.run_solve(e.ops, e.lib, 513, 3, FAST3, "K1<0>", N=4)


@case("solve_fast_values_and_lengths", ["k_quant_fast"], QUANTIZE)
def _(e):
    WF.run_solve(e.ops, e.lib, 513, 3, FAST3, "K1<1>", zhat=True, bits=True)
    WF.run_solve(e.ops, e.lib, 5, 3, FAST3, "K1<1>", zhat=True, bits=True, ll=True)


@case("solve_fast_level_counters", ["k_quant_fast"], COUNTS)
def _(e):
    """K1<2>: the level counters in LDS, flushed by adding onto the caller's int64 bins (a caller length table; N = 7, the dense
    counting kernel)."""
    WF.run_level_counts(e.ops, e.lib, 513, 3, LAM32[::5], "K1<2>", ll=True)
    WF.run_level_counts(e.ops, e.lib, 2049, 3, LAM32[::5], "K1<2>", ll=True, layout="bc->cb")
    WF.run_level_counts(e.ops, e.lib, 513, 3, FAST3, "K1<2>", N=7)


@case("solve_pruned", ["k_quant_pruned"], QUANTIZE)
def _(e):
    WF.run_solve(e.ops, e.lib, 513, 3, [LAM32[5]], "K1p<1>")
    WF.run_solve(e.ops, e.lib, 513, 3, [LAM32[5], LAM32[20]], "K1p<2>")
    WF.run_solve(e.ops, e.lib, 5, 3, [LAM32[5], LAM32[20]], "K1p<2>", N=4)


@case("solve_hull_indices", ["k_quant_hull_idx"], QUANTIZE)
def _(e):
    """K1e: the sweep table, the key look-up table and the permutation bytes in LDS; 32 lambdas, 17 (a partial last word of
    eight sweep points) and 16 permuted."""
    WF.run_solve(e.ops, e.lib, 513, 3, LAM32, "K1e")
    WF.run_solve(e.ops, e.lib, 513, 3, LAM32[:17], "K1e", layout="bc->cb")
    WF.run_solve(e.ops, e.lib, 5, 3, LAM32[15::-1], "K1e")


@case("level_counts_hull", ["k_level_counts_hull"], COUNTS)
def _(e):
    """K1t: H[], corr[], the fix-up queue and its count, n_valid -- all LDS words the kernel must set before it adds to them; one
    element past a workgroup's 512, four workgroups and one element per channel, a lone row, 11 and 32 lambdas."""
    WF.run_level_counts(e.ops, e.lib, 513, 3, LAM32[::3], "K1t")
    WF.run_level_counts(e.ops, e.lib, 2049, 3, LAM32, "K1t", layout="bc->cb")
    WF.run_level_counts(e.ops, e.lib, 1, 3, LAM32[::3], "K1t")


@case("solve_literal_flat", ["k_quant_flat"], QUANTIZE)
def _(e):
    WF.run_solve(e.ops, e.lib, 1025, 3, [0.0, 0.5, 2.0], "flat", zhat=True, bits=True)
    WF.run_solve(e.ops, e.lib, 5, 3, FAST3, "flat", mode="f64", zhat=True, bits=True)


@case("solve_literal_tiled", ["k_quant_tiled"], QUANTIZE)
def _(e):
    """k_quant_tiled: 17 channels (one whole tile of 16 and one channel: the second tile's table rows are partly outside the
    data), 65 rows (one pass of 64 and one row)."""
    WF.run_solve(e.ops, e.lib, 65, 17, FAST3, "tiled", layout="bc", zhat=True, bits=True)
    WF.run_solve(e.ops, e.lib, 65, 17, [0.0, 2.0], "tiled", layout="bc", mode="f64")
    WF.run_solve(e.ops, e.lib, 1, 3, FAST3, "tiled", layout="bc")


@case("n_bit_intervals", ["k_intervals"], ("vbq_n_bit_intervals_f32",))
def _(e):
    WF.test_n_bit_intervals(e.lib)


# ---- K2 and the tiled histogram
@case("histogram_flat_and_tiled", ["k_hist_flat", "k_hist_tiled"], ("vbq_histogram_u16", "vbq_histogram_u16_i32", "vbq_histogram_rows_u16"))
def _(e):
    """K2 (k_hist_flat: planes, C = 3) and k_hist_tiled (channel-last, C = 17: two channel tiles, the second with one channel),
    int64 and int32 counts, a hot last bin, N = 10 and N = 4 (T = 31: the counter words between T and the array's end are never
    flushed), one workgroup per row of bins (4088 rows) and two that add into the same bins (4104), whole calls and row ranges."""
    for N in (10, 4):
        for rows in (4088, 4104):
            WF.test_histogram_adds_into_its_rows_of_bins(e.ops, rows, N)
    # k_hist_tiled again with 8300 rows: 130 passes of 64 rows over 129 workgroups -- one workgroup makes a second pass
    rows, Cc, L = 8300, 17, 2
    assert LP.hist_tiled_grid(rows, Cc, L) == (129, 2, 2)
    for N, tdt, ndt in ((10, torch.int64, np.int64), (4, torch.int32, np.int32)):
        T = 2 ** (N + 1) - 1
        q = np.random.default_rng(rows + N).integers(0, T, (L, Cc, rows)).astype(np.uint16)
        q[:, :, : rows // 2] = T - 1
        g = WF.G((L, Cc, T), tdt).fill(WF.pattern((L, Cc, T), ndt))
        e.ops.histogram(WF.din(np.ascontiguousarray(q.transpose(0, 2, 1))), Cc, N=N, layout="bc", out=g.view)
        WF.check(g, WF.pattern((L, Cc, T), np.int64) + WF._bincounts(q, T), f"histogram bc rows={rows} N={N}")


@case("histogram_with_fused_models", ["k_hist_flat"], ("vbq_histogram_models_u16",))
def _(e):
    """The flush with fused models (L x C = 2048 rows of bins, each workgroup stores its row and the looked-up lengths in one
    flush) and the composed form at C = 3; N = 10 and N = 4."""
    for N in (10, 4):
        WF.test_histogram_models_assigns(e.ops, N, 1024)
    WF.test_histogram_models_assigns(e.ops, 10, 3)


# ---- lookups and layout changes
@case("gather_latents", ["k_gather_latents"], ("vbq_gather_latents_u16",))
def _(e):
    WF.test_gather_latents(e.lib, 5, 4)
    WF.test_gather_latents(e.lib, 36, 8)


@case("gather_latents_vector_tiles", ["k_gather_latents_vec"], ("vbq_gather_latents_u16",))
def _(e):
    """k_gather_latents_vec (B a multiple of 8, C of 4, 16-byte aligned bases): 72 rows are one 64-row tile and a ragged one."""
    N, L, Cc, B = 10, 2, 8, 72
    assert B % 8 == 0 and Cc % 4 == 0 and not LP.lookup_plan(L, Cc, B, N, WF.cus()).nb_lds
    srt, ll, models = WF._rank_tables(Cc, N, L, B)
    q = np.random.default_rng(B).integers(0, 2 ** (N + 1) - 1, (L, Cc, B)).astype(np.uint16)
    WF._gather_latents(e.lib, q, N, srt, None, models, True, True, True, True, 0, "gather_latents_vec")
    WF._gather_latents(e.lib, q, N, srt, ll, models, True, True, False, False, 0, "gather_latents_vec with lengths")


@case("lookup_from_the_lds", ["k_lookup_lds"], ("vbq_gather_latents_u16",))
def _(e):
    WF.test_lookup_from_the_lds(e.lib)


@case("gather_transpose", ["k_gather_transpose"], ("vbq_gather_f32",))
def _(e):
    """The runner makes all four (layout, output layout) pairs: the two that differ take k_gather_transpose (the other two
    k_gather, which has no LDS); 33 x 31 is two tiles of 32 in one direction, the last with one row."""
    assert [LP.gather_kernel(31, a, b) for a, b in ((1, 1), (1, 0), (0, 0), (0, 1))] == ["k_gather", "k_gather_transpose"] * 2
    WF.test_gather(e.ops, e.lib, 33, 31)


@case("transposes", ["k_transpose_batched", "k_transpose_batched_vec"], ("vbq_transpose_f32", "vbq_transpose_planes"))
def _(e):
    """transpose_tile: a ragged vector block of 4-byte elements (68 x 132; scalar for the u16 planes), one of 2-byte elements
    (8 x 72), odd sizes on either side of a tile (63 x 65: two tiles, the last partly outside the data) and a 4 x 4 corner.  The
    runner makes every call with aligned bases and with bases one element off, which are scalar whatever the shape."""
    want = {(68, 132): ("vec", "scalar"), (8, 72): ("vec", "vec"), (63, 65): ("scalar", "scalar"), (4, 4): ("vec", "scalar")}
    for (rows, cols), kernels in want.items():
        assert (LP.transpose_kernel(rows, cols, 4), LP.transpose_kernel(rows, cols, 2)) == kernels
        assert LP.transpose_kernel(rows, cols, 4, aligned=False) == "scalar"
        WF.test_transpose(e.ops, rows, cols)


@case("prep_planes", ["k_prep_planes"], ("vbq_prep_planes_f32",))
def _(e):
    """vbq_prep_planes_f32 has one kernel and no route to assert: k_prep_planes whatever the shape (the vector and scalar forms
    are branches inside it, by the rule of transpose_kernel); a ragged scalar shape and a ragged vector one."""
    assert LP.transpose_kernel(65, 63, 4) == "scalar" and LP.transpose_kernel(68, 132, 4) == "vec"
    for rows, cols in ((65, 63), (68, 132)):
        WF.test_prep_planes(e.ops, rows, cols)


@case("image_metrics", ["k_ssim_tile", "k_normalize_t"], ("vbq_ssim_scale_f64", "vbq_analogy_ranks_f32"))
def _(e):
    """k_ssim_tile (a 20 x 23 image: tiles partly outside it) and k_normalize_t, the first launches of their entry points."""
    WF.test_image_metrics(e.lib, FP.U8_CANARIES[0])


# ---- the notebook solve: the routing table of tests/test_gpu_notebook_variants.py
_NOTEBOOK = []


def _notebook():
    import test_gpu_notebook_variants as NV
    if not _NOTEBOOK:
        _NOTEBOOK.append(NV.Case(seed=2024, n_random=300, N=10))
    return NV, _NOTEBOOK[0]


def _notebook_runs(e, lists, want):
    NV, c = _notebook()
    for betas in lists:
        got = LP.notebook_kernel(10, betas)
        assert got == want or got.startswith(want + "<"), (got, want, betas)
        c.check(e.ops, betas, NV.EVEN, True)
        c.check(e.ops, betas, NV.OFF_ODD, False)


NOTEBOOK = ("vbq_quantize_notebook_f64",)


@case("notebook_pruned", ["k_quant_notebook_pruned"], NOTEBOOK, recorded=False)
def _(e):
    """One and two betas.  Case.check of tests/test_gpu_notebook_variants.py compares indices and the bits of the values with the
    f64 brute force by np.array_equal: exact."""
    _notebook_runs(e, [[0.7], [0.02, 30.0]], "pruned")


@case("notebook_fast", ["k_quant_notebook_fast"], NOTEBOOK, recorded=False)
def _(e):
    """Three and five betas (below the six of the threshold kernel).  Case.check of tests/test_gpu_notebook_variants.py compares
    indices and the bits of the values with the f64 brute force by np.array_equal: exact."""
    from oracle import notebook_cases as NC
    _notebook_runs(e, [NC.log_sweep(3), NC.log_sweep(5)], "fast")


@case("notebook_hull", ["k_quant_notebook_hull"], NOTEBOOK, recorded=False)
def _(e):
    """K1nt at 6, 33 and the notebook's 50 betas (three of its instances).  Case.check of tests/test_gpu_notebook_variants.py
    compares indices and the bits of the values with the f64 brute force by np.array_equal: exact."""
    from oracle import notebook_cases as NC
    _notebook_runs(e, [NC.log_sweep(6), NC.log_sweep(33), NC.NB50], "hull")


@case("notebook_literal", ["k_quant_notebook"], NOTEBOOK, recorded=False)
def _(e):
    """The literal kernel takes what the others refuse: a negative beta, betas outside the fast range.  Case.check of
    tests/test_gpu_notebook_variants.py compares indices and the bits of the values with the f64 brute force: exact."""
    from oracle import notebook_cases as NC
    _notebook_runs(e, [[-0.5, 3.0], NC.log_sweep(7) + [-1e4, 0.0, -1e-3], NC.log_sweep(12) + [1e-13, 1e19]], "literal")


# ---- the rANS coders: every user of a staged table
SEGMENT = ("vbq_rans_encode_u16", "vbq_rans_sizes_u16", "vbq_rans_decode_u16", "vbq_rans_pack_u16", "vbq_rans_unpack_u16",
           "vbq_rans_segment_offsets_u16", "vbq_rans_decode_values_f32")


@case("segment_coder", ["k_rans_encode", "k_rans_sizes", "k_rans_decode", "k_scan_groups", "k_rans_decode_values"], SEGMENT)
def _(e):
    """Tables fitted to the data at N = 7 (the footprint module's runner) and the hand-made tables of tests/adversarial_tables.py
    at N = 4 (T = 31: fc_l[31 .. 2047] is never staged) and N = 1, the 2-byte paths and a second workgroup."""
    import adversarial_tables as AT
    import test_gpu_adversarial_tables as TAT
    WF.test_segment_coder(e.lib, *AT.SEGMENT_SHAPES[0])
    TAT.test_segment_coder_matches_the_checker(*AT.SEGMENT_SHAPES[0], 4)
    TAT.test_segment_coder_matches_the_checker(*AT.SEGMENT_SHAPES[2], 1)


@case("segment_decoders_on_damaged_input", ["k_rans_decode", "k_rans_decode_values"],
      ("vbq_rans_decode_u16", "vbq_rans_decode_values_f32"), recorded=False)
def _(e):
    """Every status bit of the two segment decoders at N = 10 and N = 4, among them a frequency row that sums to 2^15 - 1:
    start[] is never built, and the kernel must not read it.  tests/test_gpu_segment_status.py compares the status words with
    `==` and indices and the bits of the values with np.array_equal against the reference decoder: exact."""
    import test_gpu_segment_status as TSS
    for N in (10, 4):
        TSS.test_segment_decoder_status_bits(N)
        TSS.test_value_decoder_status_bits(N)


@case("interleaved_coder", ["k_il_encode", "k_il_decode"], ("vbq_rans_il_sizes_u16", "vbq_rans_il_encode_u16", "vbq_rans_il_decode_u16"))
def _(e):
    import adversarial_tables as AT
    import interleaved_reference as IR
    import test_gpu_interleaved as TI
    WF.test_interleaved_coder(e.lib, *AT.IL_SHAPES[0])
    TI.test_kernels_match_the_numpy_coder(*IR.CASES[2], 3)           # N = 3: T = 15
    TI.test_kernels_match_the_numpy_coder(*IR.CASES[1], 10)
    # a frequency row that sums to 2^15 - 1: the decoder rejects its parts without building start[] (the module's own fixture, by hand)
    from vbq_amd.coder import RansCodec
    idx, freq, sizes, payload = IR.reference_case(TI.RS, TI.RN, TI.RPART, TI.RNB)
    offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    TI.test_rejects_a_frequency_row_summing_to_one_less((RansCodec(freq.copy(), N=TI.RNB), idx, freq, sizes, payload, offs))


@case("mapped_coder", ["k_rans_map_encode", "k_rans_map_decode"], ("vbq_rans_map_encode_u16", "vbq_rans_map_sizes_u16", "vbq_rans_map_decode_u16"))
def _(e):
    import test_gpu_mapped as TM
    WF.test_mapped_coder(e.lib, "per-symbol")
    TM.test_kernels_match_the_reference_and_the_segment_coder(3, 1003, 4)
    TM.test_kernels_match_the_reference_and_the_segment_coder(2, 1024, 10)
    TM.test_damaged_input_sets_the_status_bits()                    # among them one class's table that does not sum to 2^15


@case("segment_files", ["k_rans_encode_files", "k_rans_sizes_files"], ("vbq_rans_encode_files_u16", "vbq_rans_sizes_files_u16"))
def _(e):
    import test_gpu_budget_batch as BB
    import test_gpu_encode_files as EF
    WF.test_batch_encode_of_segment_files(e.ops)
    for name in ("four-bits", "mismatched-tables"):
        EF.test_kernel_words_and_sizes_equal_the_checker(name)
        BB.test_kernel_totals_equal_the_sum_of_the_checkers_sizes(name)


@case("mapped_files", ["k_rans_map_encode_files", "k_rans_map_rates_files"],
      ("vbq_rans_map_encode_files_u16", "vbq_rans_map_sizes_files_u16", "vbq_rans_map_rates_files_u16"))
def _(e):
    """Palettes of one to four classes in one launch (a block's palette is smaller than the launch's largest), N = 10 and N = 4,
    tables that do not fit the data."""
    import test_gpu_mapped_batch as MB
    import test_gpu_mapped_budget as MG
    WF.test_batch_encode_of_mapped_files(e.ops)
    MB.test_four_bits()
    MB.test_tables_that_do_not_fit_the_data()
    MG.test_totals_equal_the_reference(3, 6)
    MG.test_ten_bits()


@case("compact_files", ["k_il_encode_files", "k_il_decode_files", "k_il_rates_files"],
      ("vbq_rans_il_sizes_files_u16", "vbq_rans_il_encode_files_u16", "vbq_rans_il_decode_files_u16", "vbq_rans_il_rates_files_u16"))
def _(e):
    import test_gpu_compact_files as CF
    import test_gpu_compact_rates_files as CR
    WF.test_batch_of_compact_files(e.ops)
    CF.test_three_files_in_one_launch_match_the_numpy_coder(3)       # N = 3: T = 15
    CF.test_three_files_of_mismatched_tables_match_the_numpy_coder()
    CR.test_three_files_at_three_lambdas_in_one_launch_match_the_numpy_coder(3)
    CR.test_tables_that_do_not_fit_the_data()
    CF.test_a_frequency_row_not_summing_to_2_15_sets_bit_3(CF.Batch(*CF._three(10), 10))


@case("window_decodes", ["k_rans_decode_window", "k_rans_map_decode_window"], ("vbq_rans_decode_window_f32", "vbq_rans_map_decode_window_f32"))
def _(e):
    """fc_l, c_l, start[] and val_l of the window decoder and the palette-sized staging of the mapped one: three files in one
    launch, N = 4 (T = 31), a short last segment, palettes of one, two and four classes, tables that do not fit the data."""
    import test_gpu_mapped_window as TMW
    import test_gpu_window as TW
    WF.test_window_decodes(e.ops)
    for name in ("four-bits", "short-last-segment"):
        TW.test_kernel_boxes_and_channel_lists(name)
    TW.test_kernel_batch_of_three_files_with_mismatched_tables()
    TMW.test_kernel_boxes_and_channel_lists("four-bits")
    TMW.test_kernel_class_maps_and_palettes("seg30-short-last-segment", 3)
    TMW.test_kernel_adversarial_tables()


def _one_less(freq, table, channel):
    """The frequency stack with the largest entry of row (table, channel) lowered by one: that row sums to 2^15 - 1."""
    f = freq.copy()
    f[table, channel, int(np.argmax(f[table, channel]))] -= 1
    assert int(f[table, channel].sum()) == (1 << 15) - 1
    return f


@case("window_decodes_of_a_table_that_does_not_sum", ["k_rans_decode_window", "k_rans_map_decode_window"],
      ("vbq_rans_decode_window_f32", "vbq_rans_map_decode_window_f32"))
def _(e):
    """One row (table, channel 4) of the frequency stack sums to 2^15 - 1: the workgroups of that (file, channel) never build
    start[] and must not read it.  Three files in one launch, N = 10 and N = 4; the file that uses the table reports status bit 3
    and holds 0.0 in channel 4 of its box (every position of the box lies in a listed segment), its other channels and the other
    files hold their values.  The mapped batch has palettes of one, two and four classes; the damaged table is class 1 of the
    second file's two, so the good class's start[] is left unbuilt as well.  The outputs are returned: compared across the runs."""
    import test_gpu_mapped_window as TMW
    import test_gpu_window as TW
    out = []
    for bits in (10, 4):
        k = TW.Coded(TMW.SHAPES3, [2, 0, 1], 3, 8, 64, bits, seed=11)                  # file 1 alone uses table 0
        want = k.want(TMW.REGIONS3).copy()
        got, st, _ = k.decode(TMW.REGIONS3, fill=-7.0)
        assert st == [0, 0, 0] and np.array_equal(TW._bits(got), TW._bits(want))
        k.d_freq = torch.from_numpy(_one_less(k.freq, 0, 4)).cuda()
        want[1][..., 4] = 0.0
        for channels in (None, [7, 4, 4]):
            got, st, _ = k.decode(TMW.REGIONS3, channels, fill=-7.0)
            assert st == [0, 8, 0], (bits, channels, st)
            assert np.array_equal(TW._bits(got), TW._bits(want if channels is None else want[..., channels])), (bits, channels)
            out.append(got)
        rng = np.random.default_rng(17)
        m = TMW.MappedCoded([(TMW.SHAPES3[0], [2], None), (TMW.SHAPES3[1], [0, 3], rng.integers(0, 2, 600).astype(np.uint8)),
                             (TMW.SHAPES3[2], [1, 4, 0, 2], rng.integers(0, 4, 198).astype(np.uint8))], 5, 8, 64, bits, seed=11)
        want = m.want(TMW.REGIONS3).copy()
        got, st, _ = m.decode(TMW.REGIONS3, fill=-7.0)
        assert st == [0, 0, 0] and np.array_equal(TMW._bits(got), TMW._bits(want))
        m.d_freq = torch.from_numpy(_one_less(m.freq, 3, 4)).cuda()                    # table 3: class 1 of file 1, used nowhere else
        want[1][..., 4] = 0.0
        for channels in (None, [7, 4, 4]):
            got, st, _ = m.decode(TMW.REGIONS3, channels, fill=-7.0)
            assert st == [0, 8, 0], (bits, channels, st)
            assert np.array_equal(TMW._bits(got), TMW._bits(want if channels is None else want[..., channels])), (bits, channels)
            out.append(got)
    return tuple(out)


# ---- records, top-k, bags, scores
@case("records", ["k_records_pack", "k_records_unpack"], ("vbq_records_pack_u16", "vbq_records_unpack_f32"))
def _(e):
    for K, N, total in ((65, 4, 100), (130, 10, 601)):
        assert LP.record_fits(K, N, total)
        WF.test_records_pack_and_unpack(e.ops, e.lib, K, N, total)


@case("topk", ["k_topk"], ("vbq_topk_f32", "vbq_records_topk_f32"))
def _(e):
    """Q = 33 (a second block of one query), V = 33 (a last tile partly outside the data), a row split of three, both sources."""
    assert LP.topk_plan(64, 0, 0, 0, False).lds_bytes > 0 and LP.topk_plan(65, 4, 100, 1, True).table_in_lds
    WF.test_topk(e.lib, 3, FP.U8_CANARIES[0])


@case("bags", ["k_bag"], ("vbq_bag_f32", "vbq_records_bag_f32"))
def _(e):
    import test_gpu_bag as TBG
    WF.test_bags(e.ops, 65)
    TBG.test_both_sides_of_the_code_book_choice()                    # the code book through L2 and in the LDS (asserted there)


@case("scores", ["k_scores"], ("vbqx_scores_f32", "vbqx_records_scores_f32"), recorded=False)
def _(e):
    """tests/test_gpu_scores.py compares the bits of every score with the float32 restatement by np.array_equal: exact."""
    import test_gpu_scores as TS
    for i in (1, 4):                                                 # groups of 64 pairs (K = 5) and of 16 (K = 100, a partial group)
        K, N = TS.CASES[i][0], TS.CASES[i][4]
        assert LP.scores_plan(K, N, TS._total_bits(K, N, TS.CASES[i][5]), True) is not None
        TS.test_both_sources_equal_the_exact_restatement(i)
    TS.test_the_group_sizes_the_cases_do_not_reach(40)


# ---- the DPs
@case("budget_dp", ["k_budget_dp"], ("vbq_budget_dp_f64",))
def _(e):
    """Back-pointers in the LDS (K = 1, 7, 100) and in the workspace (K = 300, N = 16, budget 1600: one slice and two)."""
    assert LP.budget_plan(100, 10, 100 * 10 // 3 + 1).bp_in_lds and not LP.budget_plan(300, 16, 1601).bp_in_lds
    WF.test_budget_dp(e.lib, FP.U8_CANARIES[0])


@case("budget_sweep", ["k_budget_sweep"], ("vbqb_budget_sweep_f64",), recorded=False)
def _(e):
    """Every thread plan, the curve with back-pointers in the LDS, and the workspace path.  tests/test_gpu_budget_sweep.py
    compares bits and the u64 views of objectives and curves with budget_dp_rows by np.array_equal: exact."""
    import test_gpu_budget_sweep as TBS
    assert LP.budget_plan(40, 10, 257).bp_in_lds and not LP.budget_plan(300, 4, 601).bp_in_lds
    TBS.test_every_thread_plan_and_the_loop_over_n(65)
    TBS.test_every_thread_plan_and_the_loop_over_n(257)
    TBS.test_curve_is_the_objective_of_a_separate_solve_at_every_budget(7, 4)
    TBS.test_workspace_path_with_one_slice_and_several_rounds()


@case("kmeans_dp", ["k_kmeans1d"], ("vbqk_kmeans1d_f64",), recorded=False)
def _(e):
    """The value rows and the queue in LDS (n = 257 and n = ROWS_IN_LDS_MAX_N) and the rows in the workspace (one more; the
    runner asserts rows_in_lds on both sides).  tests/test_gpu_kmeans.py compares starts, counts and the u64 views of code
    points and sse with tests/kmeans_reference.py by np.array_equal: exact."""
    import kmeans_reference as KR
    import test_gpu_kmeans as TK
    TK._check(257, 3, 4, [1, 2, 4])
    for n in (KR.ROWS_IN_LDS_MAX_N, KR.ROWS_IN_LDS_MAX_N + 1):
        TK.test_one_below_at_and_one_above_each_threshold_of_the_plan(n)


@case("nearest_code", ["k_nearest_code", "k_nearest_code_channels"], ("vbq_nearest_code_f64", "vbqk_nearest_code_channels_f64"))
def _(e):
    """k_nearest_code against the oracle (9 codes), then k_nearest_code_channels against it at 255 codes per channel."""
    import test_gpu_kmeans as TK
    WF.test_comparison_quantizers(e.lib, 257)
    TK.test_nearest_code_of_all_channels_equals_the_loop_over_channels(255)


# ---- BMSHJ
@case("bmshj", ["k_bmshj_cdf_pdf", "k_bmshj_icdf_chain", "k_bmshj_nll_grad"],
      ("vbq_bmshj_cdf_pdf_f32", "vbq_bmshj_icdf_chain_f32", "vbq_bmshj_nll_grad_f32"))
def _(e):
    """The staged parameter table (300 x 7) and the unstaged one; vbq_bmshj_nll_grad_f32 at 1 and 257 rows per channel: ONE
    workgroup per output (2048 rows each), a fixed sequence of additions, compared bit for bit by the recording."""
    assert LP.cdiv(257, 256 * 8) == 1
    WF.test_bmshj_kernels(e.ops, e.lib)


def _nll_grad(e, Cc, n, what):
    import test_gpu_bmshj as TB
    from oracle import bmshj_f64 as R
    params_t = TB._prior(Cc, 10.0, seed=Cc + n, sd=0.2)._params()
    x_cb = TB._nll_data(params_t, Cc, n, seed=n)
    ref, absg = R.nll_grad64(params_t, x_cb)
    lg = R.logits64(params_t.double(), x_cb.double().t())
    bound = torch.cat([1e-4 * absg[:, :43], (1e-5 * absg[:, 43] + (2.0 ** -24 * (1 + torch.exp(lg))).sum(dim=0))[:, None]], 1)
    g = WF.G((Cc, 44), torch.float64).fill(WF.pattern((Cc, 44), np.float64))
    e.ops.bmshj_nll_grad(WF.din(params_t.cpu().numpy()), WF.din(x_cb.cpu().numpy()), out=g.view)
    torch.cuda.synchronize()
    WF._close(g, WF.pattern((Cc, 44), np.float64) + ref.cpu().numpy(), bound.cpu().numpy() + 1e-12, what)


@case("bmshj_nll_grad_of_several_workgroups", ["k_bmshj_nll_grad"], ("vbq_bmshj_nll_grad_f32",), bitwise=False)
def _(e):
    """Three workgroups add into each output: the order is free, the bounds are those of tests/test_gpu_bmshj.py."""
    assert LP.cdiv(4100, 256 * 8) == 3
    _nll_grad(e, 2, 4100, "bmshj_nll_grad C=2 n=4100")


# ---- the reductions
def _moments(e, x, layout, rows, Cc, what):
    """ops.moments onto a pattern, within n 2^-52 of the float64 sums (the footprint module's bound)."""
    per_ch = x.reshape(rows, Cc) if layout == "bc" else x.reshape(Cc, rows).T
    m64 = per_ch.astype(np.float64)
    g = WF.G((Cc, 2), torch.float64).fill(WF.pattern((Cc, 2), np.float64))
    e.ops.moments(WF.din(x), layout=layout, out=g.view)
    want = WF.pattern((Cc, 2), np.float64) + np.stack([m64.sum(0), (m64 * m64).sum(0)], 1)
    bound = rows * Cc * 2.0 ** -52 * (WF.PATTERN + 2 * Cc + np.stack([np.abs(m64).sum(0), (m64 * m64).sum(0)], 1))
    WF._close(g, want, bound, what)


def _values(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(F32)


@case("moments_one_workgroup_per_output", ["k_moments_flat", "k_moments_bc"], ("vbq_moments_f32",))
def _(e):
    """k_moments_flat with one workgroup per channel (513 values each: the scalar loop; 512: the 16-byte loads) and k_moments_bc
    with one workgroup and one lane per channel (C = 256 = the workgroup's lanes): each output is one fixed sequence of
    additions, compared bit for bit."""
    assert LP.moments_flat_grid(513, 3)[0] == 1 and LP.moments_flat_grid(512, 3)[0] == 1
    _moments(e, _values((3, 513), 1), "cb", 513, 3, "moments cb 513 x 3")
    _moments(e, _values((3, 512), 2), "cb", 512, 3, "moments cb 512 x 3")
    gx, stride = LP.moments_bc_grid(7, 256)
    assert gx == 1 and stride == LP.THREADS == 256
    _moments(e, _values((7, 256), 3), "bc", 7, 256, "moments bc 7 x 256")


@case("moments_of_several_workgroups", ["k_moments_flat", "k_moments_bc"], ("vbq_moments_f32",), bitwise=False)
def _(e):
    """Four workgroups per channel (k_moments_flat) and two workgroups whose lanes share three channels (k_moments_bc): free order."""
    assert LP.moments_flat_grid(4096, 2)[0] == 4 and LP.moments_bc_grid(2049, 3)[0] == 2
    _moments(e, _values((2, 4096), 4), "cb", 4096, 2, "moments cb 4096 x 2")
    _moments(e, _values((2049, 3), 5), "bc", 2049, 3, "moments bc 2049 x 3")


def _rd_sums(e, rows, what):
    N, Cc = 10, 3
    tab, mu, sg = WF.solve_data(rows, Cc, N)
    idx = WF.solve_oracle(rows, Cc, N, tuple(FAST3), False, "f32")[0]                  # [L, rows, C]
    srt, rate = WF._sorted_table(tab, N), WF._rank_tables(Cc, N, 3, 5)[2]
    g = WF.G((3, 2), torch.float64).fill(WF.pattern((3, 2), np.float64))
    e.ops.rd_sums(WF.din(mu), WF.din(sg), WF.din(idx), WF.din(srt), Cc, N=N, layout="bc", rate=WF.din(rate), out=g.view)
    z = srt[np.arange(Cc)[None, None, :], idx.astype(np.int64)].astype(np.float64)
    d = ((z - mu) ** 2 / (2.0 * sg.astype(np.float64) ** 2)).sum((1, 2))
    r = rate[np.arange(3)[:, None, None], np.arange(Cc)[None, None, :], idx.astype(np.int64)].astype(np.float64).sum((1, 2))
    eps = rows * Cc * 2.0 ** -52
    WF._close(g, WF.pattern((3, 2), np.float64) + np.stack([d, r], 1), (eps + 8 * 2.0 ** -52) * (WF.PATTERN + 8 + np.stack([d, r], 1)), what)


@case("rd_sums_one_workgroup", ["k_rd_sums"], ("vbq_rd_sums_u16",))
def _(e):
    assert LP.rd_sums_grid(85 * 3, 3, WF.cus())[0] == 1
    _rd_sums(e, 85, "rd_sums 85 x 3")


@case("rd_sums_of_several_workgroups", ["k_rd_sums"], ("vbq_rd_sums_u16",), bitwise=False)
def _(e):
    assert LP.rd_sums_grid(513 * 3, 3, WF.cus())[0] == 7
    _rd_sums(e, 513, "rd_sums 513 x 3")


@case("numpy_order_sums", ["k_np_finish", "k_np_block_sums"], ("vbq_numpy_sum_sq_f32", "vbq_numpy_row_sums_f32"))
def _(e):
    """Below one block of 8192 elements k_np_finish is the call's only launch (its buf[] holds the ragged tail); from one block
    on k_np_block_sums runs first.  NumPy's own order: bit for bit against the C oracle and np.sum."""
    from oracle import c_oracle as CO
    x = _values(3 * 8192 + 1539, 6)
    assert [LP.np_sums_first_kernel(n) for n in (1539, 8192, 2 * 8192 + 1539, 513, 8192 + 300)] == \
        ["k_np_finish", "k_np_block_sums", "k_np_block_sums", "k_np_finish", "k_np_block_sums"]
    for n in (1539, 8192, 2 * 8192 + 1539):
        ws, g = WF.WS(e.lib.vbq_numpy_sum_sq_workspace_bytes(n)), WF.G((1,), torch.float32)
        WF.call(e.lib, "vbq_numpy_sum_sq_f32", WF.ptr(WF.din(x[:n])), n, WF.ptr(g), WF.ptr(ws), ws.nbytes, WF.stream())
        WF.check(g, np.array([CO.numpy_sum_sq_f32(x[:n])]), f"numpy_sum_sq n={n}")
    for r_, n in ((3, 513), (2, 8192 + 300)):
        xr = x[: r_ * n].reshape(r_, n)
        ws, g = WF.WS(e.lib.vbq_numpy_row_sums_workspace_bytes(r_, n)), WF.G((r_,), torch.float32)
        WF.call(e.lib, "vbq_numpy_row_sums_f32", WF.ptr(WF.din(xr)), r_, n, WF.ptr(g), WF.ptr(ws), ws.nbytes, WF.stream())
        WF.check(g, np.array([np.sum(row) for row in xr], F32), f"numpy_row_sums {r_}x{n}")


def test_the_cases_are_the_catalogue():
    listed = {(k, c) for k, cs in LS.COVERED.items() for c in cs}
    mine = {(k, name) for name, (kernels, *_) in CASES.items() for k in kernels}
    assert listed == mine, sorted(listed ^ mine)
    entries = {e for names in LS.stream_entries().values() for e in names}
    for name, (_, wanted, *_) in CASES.items():
        assert wanted and set(wanted) <= entries, (name, sorted(set(wanted) - entries))


@pytest.mark.parametrize("name", list(CASES))
def test_case(name, env):
    _, entries, bitwise, fn, recorded = CASES[name]
    hold(name, lambda: fn(env), entries, bitwise, recorded=recorded)


# ====================================================================================================== the controls
def test_control_the_lds_carries_over():
    """pollute(byte), then lds_probe on the same stream: EVERY probe workgroup finds EVERY one of its 163 840 LDS bytes equal to
    the byte, none equal to another fill's, and fill and probes together saw every CU.  MEASURED on an MI355X (256 CUs), for
    0x00, 0x01 and 0x3C alike: 163 840 of 163 840 bytes in 512 of 512 workgroups, 256 of 256 CUs by the fill and by the probes;
    GRID_FACTOR = 2 and HOLD_TICKS = 250, one fill takes 36 us.  A driver that starts clearing the LDS fails here."""
    want = LS.cu_count()
    for byte in LS.FILLS:
        seen = LS.pollute(byte)
        ids, n = LS.probe(byte)
        other = LS.probe(LS.FILLS[(LS.FILLS.index(byte) + 1) % 3])[1]
        fill_cus, probe_cus = LS.cus_of(seen.cpu().numpy()), set(int(i) for i in ids)
        print(f"\n[lds carry-over] 0x{byte:02X}: bytes matching per workgroup {int(n.min())} .. {int(n.max())} of {LS.LDS_BYTES}; CUs seen "
              f"by the fill {len(fill_cus)}, by the probes {len(probe_cus)}, together {len(fill_cus | probe_cus)} of {want}")
        assert n.size == LS.GRID_FACTOR * want and int(n.min()) == LS.LDS_BYTES == int(n.max()), \
            f"THE LDS DID NOT CARRY OVER under 0x{byte:02X}: {int((n != LS.LDS_BYTES).sum())} of {n.size} probe workgroups found other " \
            f"bytes (fewest matching: {int(n.min())}) -- the cases of this module test nothing"
        assert int(other.max()) == 0
        assert len(fill_cus | probe_cus) == want and len(fill_cus) == want
    assert LS.assert_covered() == 3


def test_control_the_comparison_sees_a_dependence():
    """lds_toy sums 1 KiB of LDS it never wrote: under the three fills its answers are three different numbers (exactly 256 x the
    fill's u32), and the case machinery reports the mismatch.  This stands in for a wrong product kernel."""
    answers = four_answers(LS.toy, direct=True)
    for byte in LS.FILLS:
        got = answers[byte][0].view(np.uint32)
        assert got.size == LS.cu_count() and np.all(got == LS.toy_sum(byte)), (hex(byte), np.unique(got)[:4], LS.toy_sum(byte))
    assert len({LS.toy_sum(b) for b in LS.FILLS}) == 3
    lines = differences("toy", {**answers, None: answers[0]})
    assert len(lines) == 2 and lines[0].startswith("toy under lds_fill(0x01) differs") and "answer[0]" in lines[0], \
        f"THE CONTROL DID NOT FIRE: a kernel that reads LDS it never wrote was not reported ({lines}) -- this module is testing nothing"
    with pytest.raises(AssertionError, match="toy under lds_fill"):
        hold("toy", LS.toy, direct=True)


def test_control_the_fill_disturbs_nothing_else(env):
    """One catalogued call (ops.transpose, 63 x 65) with the fill on its stream: the guards of its output and a guarded bystander
    that no call was given come back intact, and the output is NumPy's transpose."""
    x = WF._values((63, 65), F32, 11)
    bystander = WF.G((4096,), torch.float32)
    g = WF.G((65, 63), torch.float32, 1)
    with LS.Polluted(0x3C) as p:
        env.ops.transpose(WF.din(x, 1), out=g.view)
        torch.cuda.synchronize()
    assert p.calls["vbq_transpose_f32"] == 1 and LS.assert_covered() == 1
    WF.check(g, x.T, "transpose under a fill")
    bystander.assert_untouched("a buffer no call was given")
