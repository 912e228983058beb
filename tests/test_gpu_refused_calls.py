"""A C call that is refused has enqueued nothing (include/vbq.h, "Refusals"): the bytes.

Every case hands an entry point live allocations of exactly the documented sizes (tests/footprint.py: canary, payload, canary)
-- so a call that is wrongly ACCEPTED is still a valid call and nothing can fault -- with the outputs and the workspace filled
with the canary and the outputs that are "ADDED to" with a fixed non-zero pattern.  After the call and a synchronise the return
code and vbq_last_error() are the refusal's and EVERY BYTE of every allocation is what it was.  Then the same buffers go to the
corrected, valid call, whose result equals the C oracle's (oracle/c_oracle.py): the error state is not sticky, and the buffers
were good ones.

The refusals are the ones that used to come late: a lambda outside the fast kernels' range in the SECOND chunk of 32 (counting
mode, VBQ_LAYOUT_BC_TO_CB), the composite calls' inner refusals (a lambda, a bit depth that is not built) behind the planes
kernel and the memset -- and, as a baseline, one refusal per family that always was the first check.  The static half is
tests/test_refusal_order_host.py.  No tolerance anywhere."""
import ctypes as C
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import footprint as FP  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from oracle import vbq_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
ROWS, CH = 130, 2
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
BC, CB, BC_TO_CB = 0, 1, 2
GOOD = 0.37                                          # what the offending lambda is corrected to
LAM32 = [float(v) for v in 2.0 ** np.linspace(-8, 7.5, 32)]
PATTERN = 1000


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    from vbq_amd import _lib
    t0 = time.perf_counter()
    yield _lib.lib()
    print(f"\n[test_gpu_refused_calls] {time.perf_counter() - t0:.1f} s")


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """A device error is not a failing comparison: after one, nothing more of this module is launched."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"device error, the rest of the module is not run: {e}", returncode=3)
    _LIVE.clear()


# ------------------------------------------------------------------------------------------------------------------ helpers
_LIVE = []


def G(shape, dtype, fill=None):
    g = FP.Guarded(shape, dtype, DEV)
    if fill is not None:
        g.fill(fill)
    _LIVE.append(g)
    return g


def din(a):
    """An input: the array in a guarded allocation of its own (a refused call leaves inputs alone too)."""
    a = np.ascontiguousarray(a)
    dtype = {np.dtype(v): k for k, v in FP._NP.items()}[a.dtype]
    return G(a.shape, dtype, a)


def ptr(g):
    return None if g is None else C.c_void_p(g.ptr)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def doubles(v):
    return (C.c_double * len(v))(*[float(x) for x in v])


def pattern(shape, dtype=np.int64):
    return (PATTERN + np.arange(int(np.prod(shape)))).reshape(shape).astype(dtype)


def refused(lib, name, args, code, text, buffers, what):
    """The call returns `code` with `text` in vbq_last_error(), and every byte of every allocation is what it was."""
    buffers = [b for b in buffers if b is not None]
    torch.cuda.synchronize()
    before = [b.raw.cpu().numpy().copy() for b in buffers]
    r = getattr(lib, name)(*args)
    torch.cuda.synchronize()
    msg = lib.vbq_last_error().decode("utf-8", "replace")
    assert r == code, f"{what}: {name} returned {r}, expected the refusal {code} ({msg!r})"
    assert text in msg, f"{what}: vbq_last_error() is {msg!r}, expected it to hold {text!r}"
    for k, (b, was) in enumerate(zip(buffers, before)):
        now = b.raw.cpu().numpy()
        bad = np.flatnonzero(now != was)
        assert bad.size == 0, (f"{what}: the refused {name} changed {bad.size} bytes of allocation {k} ({b.np_dtype.name} {b.shape}), "
                               f"the first at byte {int(bad[0]) - b.start} of the payload: 0x{int(was[bad[0]]):02x} -> 0x{int(now[bad[0]]):02x}")


def accepted(lib, name, args, what):
    r = getattr(lib, name)(*args)
    torch.cuda.synchronize()
    assert r == 0, f"{what}: the corrected {name} returned {r}: {lib.vbq_last_error()!r}"


def same(g, want, what, prefix=False):
    """The guards are intact and the payload equals `want` bit for bit (prefix: its leading elements, the rest still canary)."""
    g.assert_outside_intact(what)
    got = g.host().reshape(-1)
    want = np.ascontiguousarray(want, got.dtype).reshape(-1)
    if prefix:
        rest = g.bits().reshape(-1)[want.size:]
        assert np.all(rest == rest.dtype.type(g.pattern)), f"{what}: elements behind the result were written"
        got = got[:want.size]
    assert got.size == want.size, (what, got.size, want.size)
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.flatnonzero(got.view(u) != want.view(u))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} elements differ from the oracle, the first at {int(bad[0])}: " \
                          f"{got[bad[0]]!r} against {want[bad[0]]!r}"


_DATA = {}


def data(N, rows=ROWS, Cc=CH):
    """(table f32 [C, T] level-major, mu, sigma f32 [rows, C]), once per shape."""
    key = (N, rows, Cc)
    if key not in _DATA:
        rng = np.random.default_rng(77 + N)
        scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), Cc))
        orc = O.ChannelwiseOracle(Cc, N)
        orc.build_code_points(O.factored_gaussian_icdf(np.zeros(Cc), scale))
        mu = (scale * rng.normal(0, 1.0, (rows, Cc))).astype(F32)
        sg = np.clip(np.exp(rng.normal(-2, 0.7, (rows, Cc))), 1e-4, 10).astype(F32)
        _DATA[key] = (np.ascontiguousarray(orc.all_code_points, F32), mu, sg)
    return _DATA[key]


def level_len(L, Cc, N):
    rng = np.random.default_rng(L * 100 + Cc + N)
    return (np.arange(N + 1, dtype=F32)[None, None] + rng.uniform(0, 3, (L, Cc, N + 1))).astype(F32)


def level_counts_of(idx_lrc, N):
    """int64 [L, C, N + 1]: the bit levels of the oracle's rank indices [L, rows, C], counted."""
    lev = O.levels_of_sorted_ranks(N)[idx_lrc]
    L, _, Cc = idx_lrc.shape
    return np.stack([[np.bincount(lev[l, :, c], minlength=N + 1) for c in range(Cc)] for l in range(L)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ counting mode
@pytest.mark.parametrize("N,with_lengths", [(10, False), (10, True), (6, False)],
                         ids=["N10-raw-K1t", "N10-length-table-K1", "N6-raw-K1"])
def test_level_counts_with_a_bad_lambda_in_the_second_chunk(lib, N, with_lengths):
    """vbq_level_counts_f32, 33 lambdas, lam[32] = 0.0: the first chunk of 32 is eligible on its own (N = 10 with raw lengths:
    K1t; with a length table, or at N = 6: k_quant_fast in counting mode) and its counts are ADDED into d_level_counts."""
    tab, mu, sg = data(N)
    lam = LAM32 + [0.0]
    L = len(lam)
    ll = level_len(L, CH, N) if with_lengths else None
    g_mu, g_sg, g_tab, g_ll = din(mu.T), din(sg.T), din(tab), None if ll is None else din(ll)
    start = pattern((L, CH, N + 1))
    g_lc = G((L, CH, N + 1), torch.int64, start)
    nbytes = lib.vbq_quantize_workspace_bytes(CH, L, N)
    ws = G((nbytes,), torch.uint8)
    what = f"level_counts N={N} lengths={with_lengths}"

    def args(lam):
        return (ptr(g_mu), ptr(g_sg), ROWS, CH, CB, ptr(g_tab), ptr(g_ll), doubles(lam), L, N, ptr(g_lc), ptr(ws), nbytes, 0, stream())
    refused(lib, "vbq_level_counts_f32", args(lam), UNSUPPORTED, "served by the fast f32 kernel only",
            [g_mu, g_sg, g_tab, g_ll, g_lc, ws], what)
    lam[32] = GOOD
    accepted(lib, "vbq_level_counts_f32", args(lam), what)
    want = CO.quantize(mu, sg, tab, lam, N=N, level_len=ll)
    same(g_lc, start + level_counts_of(want, N), what)
    ws.assert_outside_intact(what + " workspace")


# ------------------------------------------------------------------------------------------------------------------ BC_TO_CB
@pytest.mark.parametrize("entry", ["vbq_quantize_f32", "vbq_quantize_rows_f32"])
def test_transposing_solve_with_a_bad_lambda_in_the_second_chunk(lib, entry):
    """VBQ_LAYOUT_BC_TO_CB, 33 lambdas, lam[32] = 1e25: the first chunk's planes were written before the second chunk was
    refused.  The refusal needs a call that K1p does not serve -- K1p takes one or two lambdas of ANY size when indices are the
    only output and no workgroup count is asked for --: vbq_quantize_f32 asks for Z_hat and lengths too, vbq_quantize_rows_f32
    for two workgroups per CU.  With indices alone vbq_quantize_f32 serves the same lambdas, and must."""
    N = 10
    tab, mu, sg = data(N)
    lam = LAM32 + [1e25]
    L = len(lam)
    rows_call = entry == "vbq_quantize_rows_f32"
    g_mu, g_sg, g_tab = din(mu), din(sg), din(tab)
    g_i = G((L, CH, ROWS), torch.uint16)
    g_z, g_b = (None, None) if rows_call else (G((L, CH, ROWS), torch.float32), G((L, CH, ROWS), torch.float32))
    nbytes = lib.vbq_quantize_workspace_bytes(CH, L, N)
    ws = G((nbytes,), torch.uint8)

    def args(lam, z=g_z, b=g_b, wg=2):
        head = (ptr(g_mu), ptr(g_sg), ROWS, CH, BC_TO_CB, ptr(g_tab), None, doubles(lam), L, N, 0, ptr(g_i), ptr(z), ptr(b), ptr(ws), nbytes)
        return head + ((0, ROWS, wg, 0, stream()) if rows_call else (stream(),))
    refused(lib, entry, args(lam), UNSUPPORTED, "VBQ_LAYOUT_BC_TO_CB is served by the fast f32 kernel only",
            [g_mu, g_sg, g_tab, g_i, g_z, g_b, ws], entry)
    if not rows_call:                                # indices alone: the last chunk is K1p's, whatever its lambda
        accepted(lib, entry, args(lam, None, None), entry + " indices only")
        same(g_i, CO.quantize(mu, sg, tab, lam, N=N).transpose(0, 2, 1), entry + " indices only, lam[32] = 1e25")
    lam[32] = GOOD
    accepted(lib, entry, args(lam), entry)
    idx, zh, bt = CO.quantize(mu, sg, tab, lam, N=N, want_zhat=True, want_bits=True)
    same(g_i, idx.transpose(0, 2, 1), entry + " indices")
    if not rows_call:
        same(g_z, zh.transpose(0, 2, 1), entry + " Z_hat")
        same(g_b, bt.transpose(0, 2, 1), entry + " lengths")
    ws.assert_outside_intact(entry + " workspace")


def test_tiled_solve_at_a_depth_built_for_planes_only(lib):
    """vbq_quantize_f32, VBQ_LAYOUT_BC, C = 2, N = 11: the channel-last tiles hold 16 tables of at most 2047 points."""
    N = 11
    tab, mu, sg = data(N)
    lam = [0.05, 0.7, 9.0]
    L = len(lam)
    g_mu, g_sg, g_tab, g_i = din(mu.T), din(sg.T), din(tab), G((L, CH, ROWS), torch.uint16)
    nbytes = lib.vbq_quantize_workspace_bytes(CH, L, N)
    ws = G((nbytes,), torch.uint8)

    def args(layout):
        return (ptr(g_mu), ptr(g_sg), ROWS, CH, layout, ptr(g_tab), None, doubles(lam), L, N, 0, ptr(g_i), None, None, ptr(ws), nbytes, stream())
    refused(lib, "vbq_quantize_f32", args(BC), UNSUPPORTED, "built for channel-major planes only", [g_mu, g_sg, g_tab, g_i, ws], "N = 11, bc")
    accepted(lib, "vbq_quantize_f32", args(CB), "N = 11, cb")                   # the same memory, read as the planes it holds
    same(g_i, CO.quantize(mu, sg, tab, lam, N=N).transpose(0, 2, 1), "N = 11, cb")
    ws.assert_outside_intact("N = 11 workspace")


# ------------------------------------------------------------------------------------------------------------------ composites
def _luts(rows):
    """Two code-length tables of rows + 1 entries: any values do (the models are looked up in them), these are the build's own."""
    n = np.arange(rows + 1, dtype=F32)
    return -np.log2((n + 1) / F32(rows + 11)), -np.log2((n + 1) / F32(rows + 2047))


def _build_expected(mu, sg, tab, lam, N, lut1, lut2):
    """include/vbq.h's statement of the build, from the C oracle: pass 1 at raw lengths, n + lut1[count], pass 2, lut2[count]."""
    T = 2 ** (N + 1) - 1
    L, Cc = len(lam), mu.shape[1]
    lc = level_counts_of(CO.quantize(mu, sg, tab, lam, N=N), N)
    raw_models = lut1[lc]
    ll = (np.arange(N + 1, dtype=F32)[None, None] + raw_models).astype(F32)
    idx2 = CO.quantize(mu, sg, tab, lam, N=N, level_len=ll)
    counts = np.stack([[np.bincount(idx2[l, :, c], minlength=T) for c in range(Cc)] for l in range(L)]).astype(np.int64)
    return lc, ll, raw_models, counts, lut2[counts]


def _build_case(lib, N_alloc, what):
    """The buffers of vbq_build_entropy_models_f32 at their documented sizes for N_alloc; the table's leading [C, T(10)] floats
    hold the N = 10 table (what a corrected call at N = 10 reads).  -> (args(lam, N), buffers, outputs, inputs)."""
    tab10, mu, sg = data(10)
    T = 2 ** (N_alloc + 1) - 1
    L = 2
    table = np.full(CH * T, 0.5, F32)
    table[:tab10.size] = tab10.reshape(-1)
    lut1, lut2 = _luts(ROWS)
    g_mu, g_sg, g_tab, g_l1, g_l2 = din(mu), din(sg), din(table), din(lut1), din(lut2)
    g_lc = G((L, CH, N_alloc + 1), torch.int64)
    g_ll, g_rm = G((L, CH, N_alloc + 1), torch.float32), G((L, CH, N_alloc + 1), torch.float32)
    g_cnt, g_mod = G((L, CH, T), torch.int64), G((L, CH, T), torch.float32)
    nbytes = lib.vbq_build_entropy_models_workspace_bytes(ROWS, CH, L, N_alloc)
    ws = G((nbytes,), torch.uint8)

    def args(lam, N):
        return (ptr(g_mu), ptr(g_sg), 0, ROWS, CH, ptr(g_tab), doubles(lam), L, N, ptr(g_l1), ROWS + 1, ptr(g_l2), ROWS + 1, ptr(g_lc),
                ptr(g_ll), ptr(g_rm), ptr(g_cnt), 0, ptr(g_mod), ptr(ws), nbytes, 0, stream())
    return args, [g_mu, g_sg, g_tab, g_l1, g_l2, g_lc, g_ll, g_rm, g_cnt, g_mod, ws], (g_lc, g_ll, g_rm, g_cnt, g_mod, ws), (mu, sg, tab10, lut1, lut2)


def _build_corrected(lib, args, outputs, inputs, lam, what, prefix):
    g_lc, g_ll, g_rm, g_cnt, g_mod, ws = outputs
    mu, sg, tab10, lut1, lut2 = inputs
    accepted(lib, "vbq_build_entropy_models_f32", args(lam, 10), what)
    lc, ll, rm, counts, models = _build_expected(mu, sg, tab10, lam, 10, lut1, lut2)
    for g, want, name in ((g_lc, lc, "level_counts"), (g_ll, ll, "level_len"), (g_rm, rm, "raw_models"), (g_cnt, counts, "counts"),
                          (g_mod, models, "models")):
        same(g, want, f"{what} {name}", prefix=prefix)
    ws.assert_outside_intact(what + " workspace")


def test_build_entropy_models_with_a_lambda_pass_1_refuses(lib):
    """vbq_build_entropy_models_f32 with lambdas [0.5, 0.0]: pass 1 refuses 0.0 -- after the planes were written into the
    workspace and the caller's d_level_counts was zeroed, before the fix.  None of d_level_counts, d_level_len, d_raw_models,
    d_counts, d_models and the workspace changes."""
    args, buffers, outputs, inputs = _build_case(lib, 10, "build [0.5, 0.0]")
    refused(lib, "vbq_build_entropy_models_f32", args([0.5, 0.0], 10), UNSUPPORTED, "served by the fast f32 kernel only", buffers,
            "build [0.5, 0.0]")
    _build_corrected(lib, args, outputs, inputs, [0.5, 0.25], "build [0.5, 0.25]", prefix=False)


def test_build_entropy_models_at_a_depth_that_is_not_built(lib):
    """N = 13 passes the call's own bound N <= 15; the library has kernels for 4 ... 12."""
    args, buffers, outputs, inputs = _build_case(lib, 13, "build N = 13")
    refused(lib, "vbq_build_entropy_models_f32", args([0.5, 0.25], 13), UNSUPPORTED, "N=13 not built", buffers, "build N = 13")
    _build_corrected(lib, args, outputs, inputs, [0.5, 0.25], "build N = 10 in the buffers of N = 13", prefix=True)


def test_compress_latents_at_a_depth_that_is_not_built(lib):
    tab10, mu, sg = data(10)
    srt10 = np.empty_like(tab10)
    srt10[:, O.level_major_to_rank(10)] = tab10
    T13 = 2 ** 14 - 1
    lam = [0.05, 0.7, 9.0]
    L = len(lam)
    tables = []
    for t in (tab10, srt10):
        full = np.full(CH * T13, 0.5, F32)
        full[:t.size] = t.reshape(-1)
        tables.append(full)
    g_mu, g_sg, g_tab, g_srt = din(mu), din(sg), din(tables[0]), din(tables[1])
    g_z, g_raw = G((L, ROWS, CH), torch.float32), G((L, ROWS, CH), torch.int32)
    nbytes = lib.vbq_compress_latents_workspace_bytes(ROWS, CH, L, 13)
    ws = G((nbytes,), torch.uint8)

    def args(N):
        return (ptr(g_mu), ptr(g_sg), 0, ROWS, CH, ptr(g_tab), ptr(g_srt), None, None, doubles(lam), L, N, ptr(g_z), ptr(g_raw), None,
                ptr(ws), nbytes, stream())
    refused(lib, "vbq_compress_latents_f32", args(13), UNSUPPORTED, "N=13 not built", [g_mu, g_sg, g_tab, g_srt, g_z, g_raw, ws],
            "compress_latents N = 13")
    accepted(lib, "vbq_compress_latents_f32", args(10), "compress_latents N = 10")
    _, zh, bt = CO.quantize(mu, sg, tab10, lam, N=10, want_zhat=True, want_bits=True)
    same(g_z, zh, "compress_latents Z_hat")
    same(g_raw, bt.astype(np.int32), "compress_latents raw_num_bits")
    ws.assert_outside_intact("compress_latents workspace")


# ------------------------------------------------------------------------------------------------------------------ baselines
def test_baseline_histogram_with_an_unknown_layout(lib):
    """K2's first checks: a layout that does not exist.  The counts, which the call ADDS to, keep their pattern."""
    N = 10
    tab, mu, sg = data(N)
    lam = [0.05, 0.7, 9.0]
    L, T = len(lam), 2 ** (N + 1) - 1
    idx = CO.quantize(mu, sg, tab, lam, N=N).transpose(0, 2, 1)                                # [L, C, rows]
    start = pattern((L, CH, T))
    g_i, g_cnt = din(idx), G((L, CH, T), torch.int64, start)

    def args(layout):
        return (ptr(g_i), ROWS, CH, layout, L, N, ptr(g_cnt), stream())
    refused(lib, "vbq_histogram_u16", args(7), INVALID, "unknown layout", [g_i, g_cnt], "histogram layout 7")
    accepted(lib, "vbq_histogram_u16", args(CB), "histogram cb")
    same(g_cnt, start + CO.histogram(idx, CH, N=N, layout=1), "histogram cb")


def test_baseline_row_sums_with_a_short_workspace(lib):
    """The reductions' first checks: a workspace one byte short of vbq_numpy_row_sums_workspace_bytes."""
    rng = np.random.default_rng(5)
    x = rng.normal(0, 3, (3, 1000)).astype(F32)
    g_x, g_out = din(x), G((3,), torch.float32)
    nbytes = lib.vbq_numpy_row_sums_workspace_bytes(3, 1000)
    assert nbytes > 1
    ws = G((nbytes,), torch.uint8)

    def args(given):
        return (ptr(g_x), 3, 1000, ptr(g_out), ptr(ws), given, stream())
    refused(lib, "vbq_numpy_row_sums_f32", args(nbytes - 1), WORKSPACE, "workspace", [g_x, g_out, ws], "row sums, short workspace")
    accepted(lib, "vbq_numpy_row_sums_f32", args(nbytes), "row sums")
    same(g_out, np.array([np.sum(r) for r in x], F32), "row sums against np.sum")            # (the kernel restates NumPy's own order)
    ws.assert_outside_intact("row sums workspace")
