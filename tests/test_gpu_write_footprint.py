"""Every kernel writes only the output it was given.

The oracle modules compare output tensors; a kernel that also stores somewhere else passes them (tests/footprint.py says
why).  Here every output of every entry point of include/vbq.h that writes device memory on one GPU is a footprint.Guarded
view -- guard | offset | payload | guard of one allocation, all canary -- and every caller workspace a guarded_workspace of
EXACTLY the bytes its vbq_*_workspace_bytes function returned.  After the call the guards must be intact, the part of the
payload the header does not give to the call must still be canary, and the part it does give must equal the reference the
kernel's own test module uses (the C oracle for the solves, NumPy for layouts, lookups and counts, tests/*_reference.py for
coders, records, top-k and bags).  Accumulating outputs start from a known non-zero pattern that is not the canary; their
region is pattern + counts.  Cases run with 256-byte aligned bases and with every output and input one element off such a base,
wherever the header states no stronger alignment.  Shapes are the smallest that reach each store path; the docstrings name it.

footprint.COVERED names, per entry point, the tests below that guard it; tests/test_write_footprint_host.py holds that table
against the header."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import adversarial_tables as AT  # noqa: E402
import bag_reference as BG  # noqa: E402
import budget_reference as BR  # noqa: E402
import footprint as FP  # noqa: E402
import interleaved_reference as IR  # noqa: E402
import launch_plans as LP  # noqa: E402
import records_reference as RR  # noqa: E402
import solve_cases as SC  # noqa: E402
import topk_reference as TR  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from oracle import notebook_cases as NC  # noqa: E402
from oracle import vbq_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
OFFSETS = (0, 1)
LAM32 = [float(v) for v in 2.0 ** np.linspace(-8, 7.5, 32)]
PATTERN = 1000                       # accumulating outputs start from PATTERN + their flat index: non-zero, not the canary


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    from vbq_amd import ops as _ops
    t0 = time.perf_counter()
    yield _ops
    print(f"\n[test_gpu_write_footprint] {time.perf_counter() - t0:.1f} s")


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """A device error is not a failing canary: after one, nothing more of this module is launched."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"device error, the rest of the module is not run: {e}", returncode=3)
    _LIVE.clear()


@pytest.fixture(scope="module")
def lib(ops):
    from vbq_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ helpers
def G(shape, dtype, off=0, guard=1024, u8=FP.U8_CANARIES[0]):
    return FP.Guarded(shape, dtype, DEV, off, guard, u8)


def WS(nbytes, u8=FP.U8_CANARIES[0]):
    return FP.guarded_workspace(nbytes, DEV, 256, u8)


_LIVE = []          # inputs handed over as raw pointers must outlive the call: kept until the test ends


def din(a, off=0):
    """The array on the device, its base `off` elements past a 256-byte boundary."""
    _LIVE.append(FP.shifted(a, off, DEV))
    return _LIVE[-1]


def ptr(t):
    if isinstance(t, FP.Guarded):
        return C.c_void_p(t.ptr)
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(lib, name, *args):
    r = getattr(lib, name)(*args)
    assert r == 0, (name, r, lib.vbq_last_error())
    torch.cuda.synchronize()


def doubles(v):
    return (C.c_double * len(v))(*[float(x) for x in v])


def ubits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, want, what):
    """Equal as bit patterns (f32 / f64: -0.0 and 0.0 differ, a NaN equals itself)."""
    want = np.ascontiguousarray(want, got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(ubits(got) != ubits(want))
    assert bad.size == 0, f"{what}: {len(bad)} of {got.size} elements differ, first at {tuple(bad[0])}: " \
                          f"got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"


def check(g, want, what, mask=None):
    """The guards are intact; the payload (inside `mask` when given, the rest still canary) equals `want`."""
    g.assert_outside_intact(what)
    got = g.host()
    if mask is None:
        same(got, want, what)
    else:
        mask = np.broadcast_to(np.asarray(mask, bool), g.shape)
        g.assert_only(mask, what)
        same(got[mask], np.ascontiguousarray(want, got.dtype)[mask], what)


def pattern(shape, dtype):
    return (PATTERN + np.arange(int(np.prod(shape)))).reshape(shape).astype(dtype)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ====================================================================================================== A. the solve family
@functools.lru_cache(maxsize=None)
def solve_data(rows, Cc, N):
    """(table f32 [C, T] level-major, mu, sigma f32 [rows, C]): Gaussian code books of random scales, latents around them."""
    rng = np.random.default_rng(1000 * rows + 10 * Cc + N)
    scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), Cc))
    orc = O.ChannelwiseOracle(Cc, N)
    orc.build_code_points(O.factored_gaussian_icdf(np.zeros(Cc), scale))
    mu = (scale * rng.normal(0, 1.0, (rows, Cc))).astype(F32)
    sg = np.clip(np.exp(rng.normal(-2, 0.7, (rows, Cc))), 1e-4, 10).astype(F32)
    tab = np.ascontiguousarray(orc.all_code_points, F32)
    for a in (tab, mu, sg):
        a.setflags(write=False)
    return tab, mu, sg


def caller_level_len(L, Cc, N):
    rng = np.random.default_rng(L * 100 + Cc + N)
    return (np.arange(N + 1, dtype=F32)[None, None] + rng.uniform(0, 3, (L, Cc, N + 1))).astype(F32)


@functools.lru_cache(maxsize=None)
def solve_oracle(rows, Cc, N, lam, ll, mode):
    """oracle.c_oracle.quantize -> (idx u16, zhat f32, bits f32), each [L, rows, C]; computed once per case."""
    tab, mu, sg = solve_data(rows, Cc, N)
    out = CO.quantize(mu, sg, tab, list(lam), N=N, level_len=caller_level_len(len(lam), Cc, N) if ll else None,
                      mode={"f32": 0, "f64": 1}[mode], want_zhat=True, want_bits=True, threads=4)
    for a in out:
        a.setflags(write=False)
    return out


def run_solve(ops, lib, rows, Cc, lam, expect, *, N=10, layout="cb", mode="f32", ll=False, zhat=False, bits=False, off=0,
              rows_range=None, wg=0, u8=FP.U8_CANARIES[0]):
    """One ops.quantize call into guarded outputs and an exactly sized guarded workspace; `expect` is the kernel
    launch_plans.solve_kernel routes it to.  Every output has at least one whole canary block of L-plane size after plane
    L - 1 and before plane 0.  With rows_range only those rows of every lambda plane may change."""
    tab, mu, sg = solve_data(rows, Cc, N)
    lam = list(lam)
    L = len(lam)
    got_kernel = LP.solve_kernel(N, lam, layout, Cc, mode=mode, level_len=ll, want_zhat=zhat, want_bits=bits,
                                 workgroups_per_cu=wg, elements=rows * Cc)
    assert got_kernel == expect, (got_kernel, expect)
    planes = layout != "bc"
    m_in, s_in = (mu.T, sg.T) if layout == "cb" else (mu, sg)
    oshape = (L, Cc, rows) if planes else (L, rows, Cc)
    guard = max(1024, Cc * rows * 4)
    gi = G(oshape, torch.uint16, off, guard)
    gz = G(oshape, torch.float32, off, guard) if zhat else None
    gb = G(oshape, torch.float32, off, guard) if bits else None
    ws = WS(lib.vbq_quantize_workspace_bytes(Cc, L, N), u8)
    lld = din(caller_level_len(L, Cc, N), off) if ll else None
    ops.quantize(din(m_in, off), din(s_in, off), din(tab, off), lam, N=N, level_len=lld, layout=layout, mode=mode,
                 out_idx=gi.view, out_zhat=None if gz is None else gz.view, out_bits=None if gb is None else gb.view,
                 workspace=ws.view, rows=rows_range, workgroups_per_cu=wg)
    torch.cuda.synchronize()
    what = f"{expect} rows={rows} C={Cc} L={L} N={N} {layout} {mode} off={off} range={rows_range} wg={wg}"
    mask = None
    if rows_range is not None:
        inside = (np.arange(rows) >= rows_range[0]) & (np.arange(rows) < rows_range[1])
        mask = inside[None, None, :] if planes else inside[None, :, None]
    want = solve_oracle(rows, Cc, N, tuple(lam), ll, mode)
    for g, w in zip((gi, gz, gb), want):
        if g is not None:
            check(g, w.transpose(0, 2, 1) if planes else w, what, mask)
    ws.assert_outside_intact(what + " workspace")


SOLVE_ROWS = (1, 2, 5, 511, 513)         # a lone element, odd plane strides, one element past 256 threads x 2 elements
FAST3 = [LAM32[3], LAM32[11], LAM32[20]]


def _planes_cases(ops, lib, lam, expect, **kw):
    for rows in SOLVE_ROWS:
        for layout in ("cb", "bc->cb"):
            for off in OFFSETS:
                run_solve(ops, lib, rows, 3, lam, expect, layout=layout, off=off, **kw)


def test_fast_kernel_indices_only(ops, lib):
    """K1<0> (k_quant_fast, MODE 0): three lambdas in the fast range, planes [3, R] and channel-last in / planes out, R in
    {1, 2, 5, 511, 513}: the dword store of an index pair with every other plane half a pair off (odd R), a lone element, and
    one element past a workgroup's 512.  Inside: the C oracle."""
    _planes_cases(ops, lib, FAST3, "K1<0>")


@pytest.mark.parametrize("zhat,bits", [(True, False), (False, True), (True, True)])
def test_fast_kernel_with_zhat_and_lengths(ops, lib, zhat, bits):
    """K1<1>: the float2 stores of Z_hat and of the lengths, each alone and both, same shapes.  Inside: the C oracle."""
    _planes_cases(ops, lib, FAST3, "K1<1>", zhat=zhat, bits=bits)


@pytest.mark.parametrize("L", [1, 2])
def test_pruned_kernel(ops, lib, L):
    """K1p<1>, K1p<2> (k_quant_pruned): the paired index stores of the descent.  Inside: the C oracle."""
    _planes_cases(ops, lib, [LAM32[5], LAM32[20]][:L], f"K1p<{L}>")


@pytest.mark.parametrize("L", [16, 17, 24, 31, 32])
def test_hull_index_kernel(ops, lib, L):
    """K1e (k_quant_hull_idx): stores through a buffer descriptor without a hardware bounds check, plane number unpacked from
    permutation bytes.  L = 16 and 32 are the two fixed instances, 17, 24, 31 the general one whose last word of eight sweep
    points is partial; eligible subsets of the 32-point sweep, sorted and permuted.  Inside: the C oracle."""
    rng = np.random.default_rng(L)
    sorted_sweep = sorted(LAM32[i] for i in rng.permutation(32)[:L])
    permuted = [sorted_sweep[i] for i in rng.permutation(L)]
    for lam in (sorted_sweep, permuted):
        assert LP.sweep_eligible(lam)
        _planes_cases(ops, lib, lam, "K1e")


@pytest.mark.parametrize("N", [4, 12])
def test_fast_kernel_other_depths(ops, lib, N):
    """K1<0> at the smallest and the largest table (N = 12: planes only; T = 31 and 8191 change the plane strides of nothing but
    the tables, the paired index stores are the same code at another depth).  Inside: the C oracle."""
    for layout in ("cb",) if N > 10 else ("cb", "bc->cb"):
        for rows in (5, 513):
            for off in OFFSETS:
                run_solve(ops, lib, rows, 3, FAST3, "K1<0>", N=N, layout=layout, off=off)


@pytest.mark.parametrize("rows", [4, 5, 1024, 1025])
def test_literal_flat_kernel(ops, lib, rows):
    """k_quant_flat: the 16-byte stores taken on vec_ok (rows a multiple of 4, aligned bases) and the scalar tail / fall-back
    (rows 5 and 1025, bases one element off); a sweep that contains 0.0 (outside the fast range) and VBQ_MODE_F64_SCORE.
    Inside: the C oracle in the same mode."""
    for off in OFFSETS:
        run_solve(ops, lib, rows, 3, [0.0, 0.5, 2.0], "flat", off=off, zhat=True, bits=True)
        run_solve(ops, lib, rows, 3, [0.0, 0.5, 2.0], "flat", off=off)
        run_solve(ops, lib, rows, 3, FAST3, "flat", off=off, mode="f64", zhat=True, bits=True)


@pytest.mark.parametrize("Cc", [3, 16, 17, 33])
def test_literal_tiled_kernel(ops, lib, Cc):
    """k_quant_tiled (channel-last): one partial tile of channels, one whole, one whole and one channel, two and one; rows 1,
    63 and 65 around the 64 rows of one pass.  Inside: the C oracle."""
    for rows in (1, 63, 65):
        for off in OFFSETS:
            run_solve(ops, lib, rows, Cc, FAST3, "tiled", layout="bc", off=off, zhat=True, bits=True)
            run_solve(ops, lib, rows, Cc, [0.0, 2.0], "tiled", layout="bc", off=off, mode="f64")


RANGES = [(1, 2), (3, 500), (511, 513), (7, 7)]


@pytest.mark.parametrize("rows_range", RANGES)
def test_row_ranges_leave_the_other_rows_alone(ops, lib, rows_range):
    """vbq_quantize_rows_f32 at R = 513 into canary-filled full-size outputs: afterwards every element of every lambda plane
    outside [row_begin, row_end) is still canary -- pass 2 runs K2 on chunk i while K1 writes chunk i + 1, so a spill is a
    race.  K1<1> on the default grid and on 4 resident workgroups per CU, K1p, K1e, the literal flat kernel.  Inside: the C
    oracle's rows."""
    for off in OFFSETS:
        for wg in (0, 4):
            run_solve(ops, lib, 513, 3, FAST3, "K1<1>", zhat=True, bits=True, off=off, rows_range=rows_range, wg=wg)
            run_solve(ops, lib, 513, 3, FAST3, "K1<1>", layout="bc->cb", zhat=True, bits=True, off=off, rows_range=rows_range,
                      wg=wg)
        run_solve(ops, lib, 513, 3, [LAM32[5], LAM32[20]], "K1p<2>", off=off, rows_range=rows_range)
        run_solve(ops, lib, 513, 3, LAM32[:17], "K1e", off=off, rows_range=rows_range)
        run_solve(ops, lib, 513, 3, LAM32, "K1e", layout="bc->cb", off=off, rows_range=rows_range)
        run_solve(ops, lib, 513, 3, [0.0, 0.5, 2.0], "flat", zhat=True, bits=True, off=off, rows_range=rows_range)


@pytest.mark.parametrize("rows_range", [(1, 2), (63, 65)])
def test_row_ranges_channel_last(ops, lib, rows_range):
    """The same for k_quant_tiled at R = 65, C = 17 (channel-last: a row range is a contiguous block of every lambda plane, the
    rows before and after it stay canary).  Inside: the C oracle's rows."""
    for off in OFFSETS:
        run_solve(ops, lib, 65, 17, FAST3, "tiled", layout="bc", zhat=True, bits=True, off=off, rows_range=rows_range)


def run_level_counts(ops, lib, rows, Cc, lam, expect, *, N=10, layout="cb", ll=False, off=0, u8=FP.U8_CANARIES[0]):
    tab, mu, sg = solve_data(rows, Cc, N)
    L = len(lam)
    assert LP.solve_kernel(N, list(lam), layout, Cc, level_len=ll, counting=True, elements=rows * Cc) == expect
    g = G((L, Cc, N + 1), torch.int64, off).fill(pattern((L, Cc, N + 1), np.int64))
    ws = WS(lib.vbq_quantize_workspace_bytes(Cc, L, N), u8)
    m_in, s_in = (mu.T, sg.T) if layout == "cb" else (mu, sg)
    lld = din(caller_level_len(L, Cc, N), off) if ll else None
    ops.level_counts(din(m_in, off), din(s_in, off), din(tab, off), list(lam), N=N, level_len=lld, layout=layout, out=g.view,
                     workspace=ws.view)
    torch.cuda.synchronize()
    idx = solve_oracle(rows, Cc, N, tuple(lam), ll, "f32")[0]
    lev = O.levels_of_sorted_ranks(N)[idx]
    counts = np.stack([[np.bincount(lev[l, :, c], minlength=N + 1) for c in range(Cc)] for l in range(L)])
    what = f"level_counts {expect} rows={rows} L={L} N={N} {layout} off={off}"
    check(g, pattern((L, Cc, N + 1), np.int64) + counts, what)
    ws.assert_outside_intact(what + " workspace")


def test_level_counts(ops, lib):
    """vbq_level_counts_f32 adds into int64 [L, C, N + 1]: K1t (an eligible raw-length sweep at N = 10), K1<2> (a caller length
    table) and N = 7 (the dense counting kernel); the output starts from a pattern, the region is pattern + np.bincount of the C
    oracle's levels.  The solve workspace is exactly vbq_quantize_workspace_bytes."""
    for rows in (5, 513):
        for layout in ("cb", "bc->cb"):
            for off in OFFSETS:
                run_level_counts(ops, lib, rows, 3, LAM32[::3], "K1t", layout=layout, off=off)
                run_level_counts(ops, lib, rows, 3, LAM32[::5], "K1<2>", layout=layout, ll=True, off=off)
                run_level_counts(ops, lib, rows, 3, FAST3, "K1<2>", N=7, layout=layout, off=off)


@pytest.mark.parametrize("u8", FP.U8_CANARIES)
def test_solve_workspace_is_exactly_what_was_asked_for(ops, lib, u8):
    """The caller workspace of vbq_quantize_f32 / vbq_quantize_rows_f32 / vbq_level_counts_f32 at exactly
    vbq_quantize_workspace_bytes, with either byte canary behind it: the literal kernels' penalty table (33 lambdas: two
    chunks), the sweep tables of K1e and K1t."""
    lam33 = [0.0] + LAM32
    tab, mu, sg = solve_data(65, 3, 10)
    assert LP.solve_kernels(10, lam33, "cb", 3, elements=195) == ["flat", "K1p<1>"]
    L = len(lam33)
    gi = G((L, 3, 65), torch.uint16, 1)
    ws = WS(lib.vbq_quantize_workspace_bytes(3, L, 10), u8)
    ops.quantize(din(mu.T, 1), din(sg.T, 1), din(tab), lam33, N=10, layout="cb", out_idx=gi.view, workspace=ws.view)
    torch.cuda.synchronize()
    check(gi, solve_oracle(65, 3, 10, tuple(lam33), False, "f32")[0].transpose(0, 2, 1), "33 lambdas")
    ws.assert_outside_intact("33 lambdas: workspace")
    run_solve(ops, lib, 513, 3, LAM32, "K1e", u8=u8)
    run_solve(ops, lib, 65, 17, FAST3, "tiled", layout="bc", mode="f64", u8=u8)
    run_solve(ops, lib, 513, 3, FAST3, "K1<1>", zhat=True, rows_range=(3, 500), wg=4, u8=u8)
    run_level_counts(ops, lib, 513, 3, LAM32, "K1t", u8=u8)


# ============================================================================================ B. layout changes and lookups
TILE_SHAPES = [(1, 1), (4, 4), (64, 64), (68, 132), (8, 72), (63, 65), (65, 63)]
"""(rows, cols) of the 64 x 64 tile walk of vbq_transpose.hip: a lone element and a 4 x 4 corner (scalar block), one whole
tile (whole-tile vector block), (68, 132) and (8, 72) (multiples of 4 / 8 with ragged tiles: the ragged vector block), and odd
sizes on either side of a tile (scalar block, two tiles)."""


def _values(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.float32:
        return rng.standard_normal(shape).astype(F32)
    return rng.integers(0, 2047, shape).astype(dtype)


@pytest.mark.parametrize("rows,cols", TILE_SHAPES)
def test_transpose(ops, rows, cols):
    """vbq_transpose_f32 and vbq_transpose_planes (u16, f32, i32; a batch of 2, so that a store past plane 0 would fall on plane
    1's first element, which is compared too).  Inside: NumPy's transpose."""
    for off in OFFSETS:
        x = _values((rows, cols), F32, rows * cols)
        g = G((cols, rows), torch.float32, off)
        ops.transpose(din(x, off), out=g.view)
        check(g, x.T, f"transpose {rows}x{cols} off={off}")
        for tdt, ndt in ((torch.uint16, np.uint16), (torch.float32, F32), (torch.int32, np.int32)):
            x = _values((2, rows, cols), ndt, rows + cols)
            g = G((2, cols, rows), tdt, off, guard=max(1024, rows * cols * 4))
            ops.transpose_planes(din(x, off), out=g.view)
            check(g, x.transpose(0, 2, 1), f"transpose_planes {ndt.__name__} {rows}x{cols} off={off}")


def test_control_an_overrun_into_the_guard_is_caught(lib):
    """Control, on the device: vbq_transpose_f32 is told that its input has one row more than the guarded output was made for,
    so its [3, 6] result runs 12 bytes past the [3, 5] payload -- into the guard behind it, memory of this test's own
    allocation.  The check must name the first of those bytes.  (tests/test_write_footprint_host.py plants its bytes by hand;
    this one is a kernel's store, read back from device memory.)"""
    rows, cols = 5, 3
    x = (np.arange((rows + 1) * cols, dtype=F32) + 1).reshape(rows + 1, cols)
    g = G((cols, rows), torch.float32)
    assert cols * 4 <= g.trail
    call(lib, "vbq_transpose_f32", ptr(din(x)), rows + 1, cols, ptr(g), stream())
    with pytest.raises(AssertionError, match=rf"byte offset {cols * rows * 4} relative to the payload .* 12 guard bytes damaged"):
        g.assert_outside_intact("control")
    same(g.raw[g.start:g.end + cols * 4].cpu().numpy().view(F32), x.T.reshape(-1), "what the call wrote")


@pytest.mark.parametrize("rows,cols", TILE_SHAPES)
def test_prep_planes(ops, rows, cols):
    """vbq_prep_planes_f32, the same tile walk with two outputs, all three spreads.  Inside: NumPy's transpose; sigma is the
    spread itself, np.sqrt of it (IEEE), or torch.exp(.) ** 0.5 on the device (what tests/test_gpu_api.py pins the launch's
    sqrtf(expf(.)) to)."""
    for off in OFFSETS:
        mu = _values((rows, cols), F32, 3 * rows + cols)
        for spread in ("sigma", "variance", "logvar"):
            sp = _values((rows, cols), F32, 5 * rows + cols)
            sp = sp if spread == "logvar" else np.abs(sp) + F32(0.01)
            d_sp = din(sp, off)
            gm, gs = G((cols, rows), torch.float32, off), G((cols, rows), torch.float32, off)
            ops.prep_planes(din(mu, off), d_sp, spread=spread, out_mu=gm.view, out_sigma=gs.view)
            want = {"sigma": lambda: sp, "variance": lambda: np.sqrt(sp),
                    "logvar": lambda: (torch.exp(d_sp) ** 0.5).cpu().numpy()}[spread]()
            check(gm, mu.T, f"prep_planes mu {spread} {rows}x{cols} off={off}")
            check(gs, want.T, f"prep_planes sigma {spread} {rows}x{cols} off={off}")


def _rank_tables(Cc, N, L, seed):
    """(idx-independent) sorted code points f32 [C, T], per-lambda length table [L, C, N + 1], per-lambda models [L, C, T]."""
    rng = np.random.default_rng(seed)
    T = 2 ** (N + 1) - 1
    srt = np.sort(rng.standard_normal((Cc, T)).astype(F32), axis=1)
    ll = (rng.random((L, Cc, N + 1)) * 20).astype(F32)
    models = (rng.random((L, Cc, T)) * 14.5 + 0.5).astype(F32)
    return srt, ll, models


@pytest.mark.parametrize("rows,Cc", [(31, 33), (32, 32), (33, 31)])
def test_gather(ops, lib, rows, Cc):
    """vbq_gather_f32 around the 32 x 33 tile of k_gather_transpose: same-layout output (both layouts) and the transposing
    output (both directions), one table for all lambdas and one per lambda.  Inside: NumPy fancy indexing."""
    N, L = 10, 2
    T = 2 ** (N + 1) - 1
    srt, _, models = _rank_tables(Cc, N, L, rows)
    q = np.random.default_rng(Cc).integers(0, T, (L, Cc, rows)).astype(np.uint16)        # planes [L, C, rows]
    l_, c_ = np.arange(L)[:, None, None], np.arange(Cc)[None, :, None]
    for tab, per_lambda in ((srt, 0), (models, 1)):
        want_cb = tab[l_, c_, q] if per_lambda else tab[c_, q]                           # [L, C, rows]
        for layout, out_layout in ((1, 1), (1, 0), (0, 0), (0, 1)):
            idx = q if layout == 1 else np.ascontiguousarray(q.transpose(0, 2, 1))
            want = want_cb if out_layout == 1 else want_cb.transpose(0, 2, 1)
            for off in OFFSETS:
                g = G(want.shape, torch.float32, off, guard=max(1024, rows * Cc * 4))
                call(lib, "vbq_gather_f32", ptr(din(idx, off)), rows, Cc, layout, L, N, ptr(din(tab, off)), per_lambda, ptr(g),
                     out_layout, stream())
                check(g, want, f"gather {rows}x{Cc} layout {layout}->{out_layout} per_lambda={per_lambda} off={off}")


def _gather_latents(lib, q, N, srt, ll, models, want_z, want_raw, want_nb, want_qi, off, what):
    """One vbq_gather_latents_u16 call on planes q [L, C, B] into guarded channel-last outputs, against NumPy lookups."""
    L, Cc, B = q.shape
    l_, c_ = np.arange(L)[:, None, None], np.arange(Cc)[None, :, None]
    lev = O.levels_of_sorted_ranks(N)[q]
    guard = max(1024, B * Cc * 4)
    gz = G((L, B, Cc), torch.float32, off, guard) if want_z else None
    graw = G((L, B, Cc), torch.int32 if ll is None else torch.float32, off, guard) if want_raw else None
    gnb = G((L, B, Cc), torch.float32, off, guard) if want_nb else None
    gqi = G((L, B, Cc), torch.uint16, off, guard) if want_qi else None
    call(lib, "vbq_gather_latents_u16", ptr(din(q, off)), B, Cc, L, N, ptr(din(srt, off)) if want_z else None,
         None if ll is None else ptr(din(ll, off)), ptr(din(models, off)) if want_nb else None, ptr(gz), ptr(graw), ptr(gnb),
         ptr(gqi), stream())
    t = lambda a: a.transpose(0, 2, 1)
    if gz is not None:
        check(gz, t(srt[c_, q]), what + " Z_hat")
    if graw is not None:
        check(graw, t(lev if ll is None else ll[l_, c_, lev]), what + " raw_num_bits")
    if gnb is not None:
        check(gnb, t(models[l_, c_, q]), what + " num_bits")
    if gqi is not None:
        check(gqi, t(q), what + " idx")


@pytest.mark.parametrize("B,Cc", [(1, 1), (4, 4), (5, 4), (4, 5), (36, 8)])
def test_gather_latents(lib, B, Cc):
    """vbq_gather_latents_u16 with every combination of its four outputs, raw_num_bits as int32 levels and as f32 lengths: a
    lone element, sizes that allow k_gather_latents_vec (multiples of 4) and sizes that do not, more than one 32-row tile.
    Inside: NumPy fancy indexing of the same tables."""
    N, L = 10, 2
    srt, ll, models = _rank_tables(Cc, N, L, B)
    q = np.random.default_rng(B * 10 + Cc).integers(0, 2 ** (N + 1) - 1, (L, Cc, B)).astype(np.uint16)
    for combo in range(1, 16):
        wz, wr, wn, wq = (bool(combo >> k & 1) for k in range(4))
        for with_ll in ((False, True) if wr else (False,)):
            for off in OFFSETS:
                _gather_latents(lib, q, N, srt, ll if with_ll else None, models, wz, wr, wn, wq, off,
                                f"gather_latents B={B} C={Cc} outputs={combo:04b} level_len={with_ll} off={off}")


def test_lookup_from_the_lds(lib):
    """k_lookup_lds at the smallest shape tests/launch_plans.py gives it: one lambda, four channels, 3072 rows -- num_bits
    leaves the generic kernel (kLdsMinLookupsNb rows, B and C multiples of 4), the other three outputs stay with it."""
    N, L, Cc, B = 10, 1, 4, LP.LDS_MIN_LOOKUPS_NB
    p = LP.lookup_plan(L, Cc, B, N, cus())
    assert p.nb_lds and not p.z_lds and not LP.lookup_plan(L, Cc, B - 4, N, cus()).nb_lds
    srt, _, models = _rank_tables(Cc, N, L, 7)
    q = np.random.default_rng(8).integers(0, 2 ** (N + 1) - 1, (L, Cc, B)).astype(np.uint16)
    for off in OFFSETS:
        _gather_latents(lib, q, N, srt, None, models, True, True, True, True, off, f"lookup_lds off={off}")
        _gather_latents(lib, q, N, srt, None, models, False, False, True, False, off, f"lookup_lds alone off={off}")


def _sorted_table(tab, N):
    srt = np.empty_like(tab)
    srt[:, O.level_major_to_rank(N)] = tab
    return srt


@pytest.mark.parametrize("u8", FP.U8_CANARIES)
def test_compress_latents_in_an_exact_workspace(lib, u8):
    """vbq_compress_latents_f32 (planes, solve, fused lookups in one call) with guarded outputs and a 256-byte aligned
    workspace of exactly vbq_compress_latents_workspace_bytes: B = 37 rows, C = 3, three lambdas, with and without caller
    lengths and entropy models.  Inside: the C oracle's solve and NumPy lookups."""
    N, B, Cc = 10, 37, 3
    tab, mu, sg = solve_data(B, Cc, N)
    srt = _sorted_table(tab, N)
    L = len(FAST3)
    _, _, models = _rank_tables(Cc, N, L, 11)
    nbytes = lib.vbq_compress_latents_workspace_bytes(B, Cc, L, N)
    for with_tables in (False, True):
        idx, zh, bt = solve_oracle(B, Cc, N, tuple(FAST3), with_tables, "f32")
        ll = caller_level_len(L, Cc, N) if with_tables else None
        for off in OFFSETS:
            ws = WS(nbytes, u8)
            gz = G((L, B, Cc), torch.float32, off)
            graw = G((L, B, Cc), torch.float32 if with_tables else torch.int32, off)
            gnb = G((L, B, Cc), torch.float32, off) if with_tables else None
            call(lib, "vbq_compress_latents_f32", ptr(din(mu, off)), ptr(din(sg, off)), 0, B, Cc, ptr(din(tab, off)),
                 ptr(din(srt, off)), None if ll is None else ptr(din(ll, off)), ptr(din(models, off)) if with_tables else None,
                 doubles(FAST3), L, N, ptr(gz), ptr(graw), ptr(gnb), ptr(ws), nbytes, stream())
            what = f"compress_latents tables={with_tables} off={off}"
            check(gz, zh, what + " Z_hat")
            check(graw, bt, what + " raw_num_bits")
            if gnb is not None:
                check(gnb, models[np.arange(L)[:, None, None], np.arange(Cc)[None, None, :], idx.astype(np.int64)],
                      what + " num_bits")
            ws.assert_outside_intact(what + " workspace")


@pytest.mark.parametrize("u8", FP.U8_CANARIES)
def test_build_entropy_models_in_an_exact_workspace(lib, u8):
    """vbq_build_entropy_models_f32 (six launches) with its five outputs guarded and a workspace of exactly
    vbq_build_entropy_models_workspace_bytes: B = 201 rows, C = 3, two lambdas (6 rows of bins: K2's composed path).  Inside, by
    the header's own statement of the build: pass 1 = np.bincount of the C oracle's levels at raw lengths, lengths =
    n + lut_levels[count], pass 2 = np.bincount of the C oracle's ranks under those lengths, models = lut_ranks[count]."""
    N, B, Cc = 10, 201, 3
    T = 2 ** (N + 1) - 1
    lam = [LAM32[8], LAM32[18]]
    L = len(lam)
    tab, mu, sg = solve_data(B, Cc, N)
    lut1 = -np.log2((np.arange(B + 1, dtype=F32) + 1) / F32(B + (N + 1)))
    lut2 = -np.log2((np.arange(B + 1, dtype=F32) + 1) / F32(B + T))
    idx1 = CO.quantize(mu, sg, tab, lam, N=N)
    lev = O.levels_of_sorted_ranks(N)[idx1]
    lc = np.stack([[np.bincount(lev[l, :, c], minlength=N + 1) for c in range(Cc)] for l in range(L)]).astype(np.int64)
    raw_models = lut1[lc]
    level_len = (np.arange(N + 1, dtype=F32)[None, None] + raw_models).astype(F32)
    idx2 = CO.quantize(mu, sg, tab, lam, N=N, level_len=level_len)
    counts = np.stack([[np.bincount(idx2[l, :, c], minlength=T) for c in range(Cc)] for l in range(L)]).astype(np.int64)
    nbytes = lib.vbq_build_entropy_models_workspace_bytes(B, Cc, L, N)
    for i32 in (0, 1):
        for off in OFFSETS:
            ws = WS(nbytes, u8)
            g_lc, g_ll, g_rm = (G((L, Cc, N + 1), dt, off) for dt in (torch.int64, torch.float32, torch.float32))
            g_cnt, g_mod = G((L, Cc, T), torch.int32 if i32 else torch.int64, off), G((L, Cc, T), torch.float32, off)
            call(lib, "vbq_build_entropy_models_f32", ptr(din(mu, off)), ptr(din(sg, off)), 0, B, Cc, ptr(din(tab, off)),
                 doubles(lam), L, N, ptr(din(lut1, off)), B + 1, ptr(din(lut2, off)), B + 1, ptr(g_lc), ptr(g_ll), ptr(g_rm),
                 ptr(g_cnt), i32, ptr(g_mod), ptr(ws), nbytes, 0, stream())
            what = f"build_entropy_models i32={i32} off={off}"
            check(g_lc, lc, what + " level_counts")
            check(g_rm, raw_models, what + " raw_models")
            check(g_ll, level_len, what + " level_len")
            check(g_cnt, counts, what + " counts")
            check(g_mod, lut2[counts], what + " models")
            ws.assert_outside_intact(what + " workspace")


# ============================================================================================== C. K2 and the length tables
def _bincounts(idx_lcr, T):
    L, Cc, _ = idx_lcr.shape
    return np.stack([[np.bincount(idx_lcr[l, c], minlength=T) for c in range(Cc)] for l in range(L)]).astype(np.int64)


def _hist_flat_workgroups(rows, Cc, L):
    """launch_hist, planes: workgroups per (lambda, channel) row -- the thread count read from vbq_hist.hip itself."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vbq_amd", "csrc", "vbq_hist.hip")).read()
    threads = int(re.search(r"#define VBQ_HIST_THREADS (\d+)", src).group(1))
    return max(1, min(LP.cdiv(rows // 8, threads), 2048 // (Cc * L) + 1))


@pytest.mark.parametrize("rows", [7, 8, 4088, 4104])
@pytest.mark.parametrize("N", [10, 4])
def test_histogram_adds_into_its_rows_of_bins(ops, rows, N):
    """vbq_histogram_u16 / _i32 / _rows_u16: hist_flush stores ceil(T / 512) bins per thread behind an `i < T` test, and T is
    odd, so every (lambda, channel) row of bins starts at an odd element.  Planes with C = 3 (rows 7 and 8: without / with one
    8-index vector; 4088: 511 vectors, one workgroup of 512 threads; 4104: two workgroups per row, which add into the same
    bins) and channel-last at C = 17 (two channel tiles).  The counts start from a pattern; the region is
    pattern + np.bincount."""
    assert _hist_flat_workgroups(rows, 3, 2) == (2 if rows == 4104 else 1)
    T, L = 2 ** (N + 1) - 1, 2
    for layout, Cc in (("cb", 3), ("bc", 17)):
        q = np.random.default_rng(rows + Cc + N).integers(0, T, (L, Cc, rows)).astype(np.uint16)
        q[:, :, : rows // 2] = T - 1                                       # a hot bin: the last one of every row
        idx = q if layout == "cb" else np.ascontiguousarray(q.transpose(0, 2, 1))
        want = _bincounts(q, T)
        for tdt, ndt in ((torch.int64, np.int64), (torch.int32, np.int32)):
            for off in OFFSETS:
                g = G((L, Cc, T), tdt, off).fill(pattern((L, Cc, T), ndt))
                ops.histogram(din(idx, off), Cc, N=N, layout=layout, out=g.view)
                check(g, pattern((L, Cc, T), np.int64) + want, f"histogram {layout} rows={rows} N={N} {ndt.__name__} off={off}")
                g = G((L, Cc, T), tdt, off).fill(pattern((L, Cc, T), ndt))
                a, b = rows // 3, rows - 1
                ops.histogram(din(idx, off), Cc, N=N, layout=layout, out=g.view, rows=(a, b))
                check(g, pattern((L, Cc, T), np.int64) + _bincounts(q[:, :, a:b], T),
                      f"histogram rows [{a}, {b}) {layout} rows={rows} N={N} {ndt.__name__} off={off}")


@pytest.mark.parametrize("N", [10, 4])
@pytest.mark.parametrize("Cc", [1024, 3])
def test_histogram_models_assigns(ops, N, Cc):
    """vbq_histogram_models_u16, fused (L = 2, C = 1024: 2048 rows of bins, each workgroup stores its row and the looked-up
    lengths in one flush) and composed (C = 3), with and without lut / models, int64 and int32 counts; the outputs are
    ASSIGNED, so they start as canary.  Inside: np.bincount and lut[counts]."""
    T, L, rows = 2 ** (N + 1) - 1, 2, 9
    q = np.random.default_rng(N + Cc).integers(0, T, (L, Cc, rows)).astype(np.uint16)
    q[:, :, :4] = T - 1
    want = _bincounts(q, T)
    lut = (-np.log2((np.arange(rows + 1, dtype=F32) + 1) / F32(rows + T))).astype(F32)
    for tdt in (torch.int64, torch.int32):
        for with_models in (True, False):
            for off in OFFSETS:
                gc = G((L, Cc, T), tdt, off)
                gm = G((L, Cc, T), torch.float32, off) if with_models else None
                ops.histogram_models(din(q, off), Cc, gc.view, N=N, lut=din(lut, off) if with_models else None,
                                     models=gm.view if with_models else None)
                what = f"histogram_models C={Cc} N={N} {tdt} models={with_models} off={off}"
                check(gc, want, what + " counts")
                if gm is not None:
                    check(gm, lut[want], what + " models")


@pytest.mark.parametrize("n", [4, 5, 1024, 1027])
def test_code_lengths_from_counts(ops, n):
    """vbq_code_lengths_from_counts: the float4 stores of k_lut_models_v4 and their scalar tail, each output alone and both,
    int64 and int32 counts, with and without the level period.  Inside: NumPy's lut[count] and level + lut[count]."""
    rng = np.random.default_rng(n)
    lut = rng.random(50).astype(F32) * 10
    for ndt in (np.int64, np.int32):
        counts = rng.integers(0, 50, n).astype(ndt)
        for period in (0, 11):
            level = (np.arange(n) % period if period else np.zeros(n)).astype(F32)
            for want_len, want_model in ((True, False), (False, True), (True, True)):
                for off in OFFSETS:
                    gl = G((n,), torch.float32, off) if want_len else None
                    gm = G((n,), torch.float32, off) if want_model else None
                    ops.code_lengths_from_counts(din(counts, off), din(lut, off), level_period=period, want_len=want_len,
                                                 want_model=want_model, out_len=None if gl is None else gl.view,
                                                 out_model=None if gm is None else gm.view)
                    what = f"code_lengths n={n} {ndt.__name__} period={period} off={off}"
                    if gl is not None:
                        check(gl, level + lut[counts], what + " len")
                    if gm is not None:
                        check(gm, lut[counts], what + " model")


def _close(g, want, bound, what):
    g.assert_outside_intact(what)
    err = np.abs(g.host().astype(np.float64) - want)
    assert np.all(err <= bound), (what, err.max(), np.max(bound))


@pytest.mark.parametrize("u8", FP.U8_CANARIES)
def test_small_outputs_of_the_reductions(ops, lib, u8):
    """The few-element outputs of vbq_moments_f32, vbq_rd_sums_u16 (f64, added to: a pattern first), vbq_numpy_sum_sq_f32,
    vbq_numpy_row_sums_f32 (exact workspaces; d_x of the first 16-byte aligned as the header demands), vbq_index_max_u16 (MAX-ed
    into) and vbq_check_inputs_f32 (added to).  Inside: float64 NumPy sums within n 2^-52 of the sum of magnitudes for the
    two f64 reductions (their order is not specified), bit for bit for the NumPy-order sums (the C oracle and np.sum), exact
    integers for the rest."""
    N, rows, Cc = 10, 513, 3
    tab, mu, sg = solve_data(rows, Cc, N)
    eps = rows * Cc * 2.0 ** -52
    for off in OFFSETS:
        for layout in ("bc", "cb"):
            x = mu if layout == "bc" else np.ascontiguousarray(mu.T)
            g = G((Cc, 2), torch.float64, off).fill(pattern((Cc, 2), np.float64))
            ops.moments(din(x, off), layout=layout, out=g.view)
            m64 = mu.astype(np.float64)
            want = pattern((Cc, 2), np.float64) + np.stack([m64.sum(0), (m64 * m64).sum(0)], 1)
            bound = eps * (PATTERN + 8 + np.stack([np.abs(m64).sum(0), (m64 * m64).sum(0)], 1))
            _close(g, want, bound, f"moments {layout} off={off}")
        # rd_sums on planes, L = 3
        idx = solve_oracle(rows, Cc, N, tuple(FAST3), False, "f32")[0]                   # [L, rows, C]
        srt = _sorted_table(tab, N)
        rate = _rank_tables(Cc, N, 3, 5)[2]
        g = G((3, 2), torch.float64, off).fill(pattern((3, 2), np.float64))
        ops.rd_sums(din(mu, off), din(sg, off), din(idx, off), din(srt, off), Cc, N=N, layout="bc", rate=din(rate, off),
                    out=g.view)
        z = srt[np.arange(Cc)[None, None, :], idx.astype(np.int64)].astype(np.float64)
        d = ((z - mu) ** 2 / (2.0 * sg.astype(np.float64) ** 2)).sum((1, 2))
        r = rate[np.arange(3)[:, None, None], np.arange(Cc)[None, None, :], idx.astype(np.int64)].astype(np.float64).sum((1, 2))
        want = pattern((3, 2), np.float64) + np.stack([d, r], 1)
        # the distortion term is computed from f32 inputs; one rounded subtraction, square and quotient per element in f64
        _close(g, want, (eps + 8 * 2.0 ** -52) * (PATTERN + 8 + np.stack([d, r], 1)), f"rd_sums off={off}")
        # the NumPy-order sums
        x = mu.reshape(-1)
        for n in (1, 5, 1539):
            ws = WS(lib.vbq_numpy_sum_sq_workspace_bytes(n), u8)
            g = G((1,), torch.float32, off)
            call(lib, "vbq_numpy_sum_sq_f32", ptr(din(x[:n], 0)), n, ptr(g), ptr(ws), ws.nbytes, stream())
            check(g, np.array([CO.numpy_sum_sq_f32(x[:n])]), f"numpy_sum_sq n={n} off={off}")
            ws.assert_outside_intact(f"numpy_sum_sq n={n} workspace")
        for r_, n in ((1, 1), (3, 513), (5, 300)):
            xr = x[: r_ * n].reshape(r_, n)
            ws = WS(lib.vbq_numpy_row_sums_workspace_bytes(r_, n), u8)
            g = G((r_,), torch.float32, off)
            call(lib, "vbq_numpy_row_sums_f32", ptr(din(xr, off)), r_, n, ptr(g), ptr(ws), ws.nbytes, stream())
            check(g, np.array([np.sum(row) for row in xr], F32), f"numpy_row_sums {r_}x{n} off={off}")
            ws.assert_outside_intact(f"numpy_row_sums {r_}x{n} workspace")
        # scans
        flat = idx.reshape(-1)
        for n in (1, 5, 1025):
            for start in (3, 60000):
                g = G((1,), torch.uint32, off).fill(np.array([start], np.uint32))
                call(lib, "vbq_index_max_u16", ptr(din(flat[:n], off)), n, ptr(g), stream())
                check(g, np.array([max(start, int(flat[:n].max()))]), f"index_max n={n} off={off}")
            bad_mu, bad_sg = x[:n].copy(), sg.reshape(-1)[:n].copy()
            bad_mu[::3] = np.nan
            bad_sg[::2] = -1.0
            g = G((2,), torch.uint32, off).fill(pattern((2,), np.uint32))
            call(lib, "vbq_check_inputs_f32", ptr(din(bad_mu, off)), ptr(din(bad_sg, off)), n, ptr(g), stream())
            check(g, pattern((2,), np.int64) + np.array([len(bad_mu[::3]), len(bad_sg[::2])]), f"check_inputs n={n} off={off}")


# ========================================================================================================== D. one-file coders
def _fitted_streams(S, n, N, seed):
    """(idx u16 [S, n], freq u16 [S, T]): rounded normals of several spreads, tables fitted to the data they code."""
    from vbq_amd.coder import quantize_frequencies
    T = 2 ** (N + 1) - 1
    rng = np.random.default_rng(seed)
    idx = np.stack([np.clip(np.rint(T / 2 + rng.normal(0, (2.0, 25.0, 300.0)[s % 3], n)), 0, T - 1) for s in range(S)])
    idx = idx.astype(np.uint16)
    freq = quantize_frequencies(_bincounts(idx[None], T)[0], 1)
    return idx, np.ascontiguousarray(freq, np.uint16)


STATUS_SEED = 1 << 30                 # status words are OR-ed into: they start from a bit no call sets


def _status(off):
    return G((1,), torch.uint32, off).fill(np.array([STATUS_SEED], np.uint32))


@pytest.mark.parametrize("n,seg", AT.SEGMENT_SHAPES)
def test_segment_coder(lib, n, seg):
    """vbq_rans_encode / sizes / decode / pack / unpack / segment_offsets / decode_values at the (n, seg) of
    adversarial_tables.SEGMENT_SHAPES (the 2-byte paths, the 16-byte paths, a second workgroup), three streams with tables
    fitted to the data.  Regions: the padded words array as a whole (its valid words are compared with the C checker's), the
    first `total` words of pack's payload, exactly [S, n] of a decode.  Inside: oracle.c_oracle.rans_encode / the data."""
    N, S = 7, 3
    T = 2 ** (N + 1) - 1
    idx, freq = _fitted_streams(S, n, N, n + seg)
    w_ref, s_ref = CO.rans_encode(idx, freq, seg)
    nseg = s_ref.shape[1]
    M = S * nseg
    valid = np.arange(seg + 2)[None, None, :] < s_ref[..., None].astype(np.int64)
    blob = w_ref[valid]
    offs = (np.cumsum(s_ref.reshape(-1).astype(np.int64)) - s_ref.reshape(-1)).astype(np.int64)
    values = ((np.arange(T, dtype=F32) + F32(0.5)) * F32(-1.25)).astype(F32)
    for off in OFFSETS:
        what = f"segment coder n={n} seg={seg} off={off}"
        d_idx, d_freq = din(idx, off), din(freq, off)
        gw, gs = G((S, nseg, seg + 2), torch.uint16, off), G((S, nseg), torch.uint32, off)
        call(lib, "vbq_rans_encode_u16", ptr(d_idx), S, n, N, seg, ptr(d_freq), ptr(gw), ptr(gs), stream())
        check(gs, s_ref, what + " encode sizes")
        gw.assert_outside_intact(what + " encode words")
        same(gw.host()[valid], blob, what + " encode words")
        gs2 = G((S, nseg), torch.uint32, off)
        call(lib, "vbq_rans_sizes_u16", ptr(d_idx), S, n, N, seg, ptr(d_freq), ptr(gs2), stream())
        check(gs2, s_ref, what + " sizes")
        gi, st = G((S, n), torch.uint16, off), _status(off)
        call(lib, "vbq_rans_decode_u16", ptr(din(w_ref, off)), ptr(din(s_ref, off)), S, n, N, seg, ptr(d_freq), ptr(gi), ptr(st),
             stream())
        check(gi, idx, what + " decode")
        check(st, [STATUS_SEED], what + " decode status")
        gp, go, gt = G((M * (seg + 2),), torch.uint16, off), G((M,), torch.int64, off), G((1,), torch.uint64, off)
        call(lib, "vbq_rans_pack_u16", ptr(din(w_ref, off)), ptr(din(s_ref, off)), S, n, seg, ptr(gp), ptr(go), ptr(gt), stream())
        check(gt, [blob.size], what + " pack total")
        check(go, offs, what + " pack offsets")
        check(gp, np.concatenate([blob, np.zeros(M * (seg + 2) - blob.size, np.uint16)]), what + " pack payload",
              np.arange(M * (seg + 2)) < blob.size)
        gw, gs, go, st = G((S, nseg, seg + 2), torch.uint16, off), G((S, nseg), torch.uint32, off), G((M,), torch.int64, off), \
            _status(off)
        call(lib, "vbq_rans_unpack_u16", ptr(din(blob, off)), blob.size, ptr(din(s_ref.astype(np.uint16), off)), S, n, seg,
             ptr(gw), ptr(gs), ptr(go), ptr(st), stream())
        check(gs, s_ref, what + " unpack sizes")
        check(go, offs, what + " unpack offsets")
        check(st, [STATUS_SEED], what + " unpack status")
        gw.assert_outside_intact(what + " unpack words")
        same(gw.host()[valid], blob, what + " unpack words")
        go, st = G((nseg,), torch.int64, off), _status(off)
        sizes0 = s_ref[0].astype(np.uint16)
        blob0 = w_ref[0][valid[0]]
        call(lib, "vbq_rans_segment_offsets_u16", ptr(din(sizes0, off)), nseg, seg, blob0.size, ptr(go), ptr(st), stream())
        check(go, offs[:nseg], what + " segment_offsets")
        check(st, [STATUS_SEED], what + " segment_offsets status")
        d_blob0, d_sizes0, d_offs0 = din(blob0, off), din(sizes0, off), din(offs[:nseg], off)
        gv, st = G((n,), torch.float32, off), _status(off)
        call(lib, "vbq_rans_decode_values_f32", ptr(d_blob0), blob0.size, ptr(d_sizes0), ptr(d_offs0), n, seg, N,
             ptr(din(freq[0], off)), ptr(din(values, off)), None, 0, ptr(gv), ptr(st), stream())
        check(gv, values[idx[0]], what + " decode_values")
        check(st, [STATUS_SEED], what + " decode_values status")
        listed = np.array([nseg - 1, 0, nseg // 2, 0], np.int64)             # any order, a repeat, the short last segment
        gv, st = G((len(listed) * seg,), torch.float32, off), _status(off)
        call(lib, "vbq_rans_decode_values_f32", ptr(d_blob0), blob0.size, ptr(d_sizes0), ptr(d_offs0), n, seg, N,
             ptr(din(freq[0], off)), ptr(din(values, off)), ptr(din(listed, off)), len(listed), ptr(gv), ptr(st), stream())
        want, mask = np.zeros(len(listed) * seg, F32), np.zeros(len(listed) * seg, bool)
        for i, g_ in enumerate(listed):
            a, b = g_ * seg, min(n, (g_ + 1) * seg)
            want[i * seg: i * seg + b - a], mask[i * seg: i * seg + b - a] = values[idx[0, a:b]], True
        check(gv, want, what + " decode_values listed", mask)
        check(st, [STATUS_SEED], what + " decode_values listed status")


@pytest.mark.parametrize("n,part", AT.IL_SHAPES)
def test_interleaved_coder(lib, n, part):
    """vbq_rans_il_sizes / il_encode / il_decode at adversarial_tables.IL_SHAPES: the payload is exactly the sum of the sizes
    (the encoder writes every part backwards from its end), the decode exactly [S, n].  Inside: tests/interleaved_reference.py."""
    N, S = 7, 3
    idx, freq = _fitted_streams(S, n, N, n + part)
    s_ref, p_ref = IR.encode(idx, freq, part)
    s_ref, p_ref = np.ascontiguousarray(s_ref, np.uint32), np.ascontiguousarray(p_ref, np.uint16)
    P = s_ref.size
    offs = (np.cumsum(s_ref.astype(np.int64)) - s_ref).astype(np.int64)
    for off in OFFSETS:
        what = f"interleaved coder n={n} part={part} off={off}"
        d_idx, d_freq = din(idx, off), din(freq, off)
        gs = G((P,), torch.uint32, off)
        call(lib, "vbq_rans_il_sizes_u16", ptr(d_idx), S, n, N, part, ptr(d_freq), ptr(gs), stream())
        check(gs, s_ref, what + " sizes")
        gp = G((p_ref.size,), torch.uint16, off)
        call(lib, "vbq_rans_il_encode_u16", ptr(d_idx), S, n, N, part, ptr(d_freq), ptr(din(s_ref, off)), ptr(din(offs, off)),
             ptr(gp), p_ref.size, stream())
        check(gp, p_ref, what + " payload")
        gi, st = G((S, n), torch.uint16, off), _status(off)
        call(lib, "vbq_rans_il_decode_u16", ptr(din(p_ref, off)), p_ref.size, ptr(din(s_ref, off)), ptr(din(offs, off)), S, n, N,
             part, ptr(d_freq), ptr(gi), ptr(st), stream())
        check(gi, idx, what + " decode")
        check(st, [STATUS_SEED], what + " decode status")


@pytest.mark.parametrize("name", AT.MAPPED_MAPS)
def test_mapped_coder(lib, name):
    """vbq_rans_map_encode / map_sizes / map_decode at adversarial_tables.mapped_case(3, 1003, 7, ...): a class change at every
    symbol (the scalar path) and constant over aligned groups of eight (the vector path).  Inside: tests/mapped_reference.py."""
    P, n, N = 3, 1003, 7
    seg, S = AT.MAPPED_SEG, AT.MAPPED_S
    planes, freq, cls, idx, w_ref, s_ref = (np.array(a) for a in AT.mapped_case(P, n, N, name))
    s_ref = s_ref.astype(np.uint32)
    nseg = s_ref.shape[1]
    valid = np.arange(seg + 2)[None, None, :] < s_ref[..., None].astype(np.int64)
    for off in OFFSETS:
        what = f"mapped coder {name} off={off}"
        d_planes, d_cls, d_freq = din(planes, off), din(cls, off), din(freq, off)
        gw, gs = G((S, nseg, seg + 2), torch.uint16, off), G((S, nseg), torch.uint32, off)
        call(lib, "vbq_rans_map_encode_u16", ptr(d_planes), P, ptr(d_cls), P, S, n, N, seg, ptr(d_freq), ptr(gw), ptr(gs),
             stream())
        check(gs, s_ref, what + " encode sizes")
        gw.assert_outside_intact(what + " encode words")
        same(gw.host()[valid], w_ref.astype(np.uint16)[valid], what + " encode words")
        gs = G((S, nseg), torch.uint32, off)
        call(lib, "vbq_rans_map_sizes_u16", ptr(d_planes), P, ptr(d_cls), P, S, n, N, seg, ptr(d_freq), ptr(gs), stream())
        check(gs, s_ref, what + " sizes")
        gi, st = G((S, n), torch.uint16, off), _status(off)
        call(lib, "vbq_rans_map_decode_u16", ptr(din(w_ref.astype(np.uint16), off)), ptr(din(s_ref, off)), ptr(d_cls), P, S, n, N,
             seg, ptr(d_freq), ptr(gi), ptr(st), stream())
        check(gi, idx, what + " decode")
        check(st, [STATUS_SEED], what + " decode status")


# ======================================================================================================= E. notebook kernels
@functools.lru_cache(maxsize=None)
def _notebook_case():
    pts, lens, means, stds, _ = NC.case(np.random.default_rng(77), 200, 10)
    return pts, lens, means, stds


@pytest.mark.parametrize("count", [1, 2, 3, 6, 50, 64, 65])
def test_notebook_kernels(lib, count):
    """vbq_quantize_notebook_f64 at n in {1, 2, 63, 65}: K1np<1>, K1np<2> (1, 2 betas), K1n fast (3), K1nt (6, 50, 64) and a
    second chunk of one beta (65), with and without the value planes; a lone element, a pair, one short of and one past a
    wave.  Guards before plane 0 and after the last plane of the index AND the value planes.  Inside: the f64 brute force
    oracle.c_oracle.compress_coordinates, bit for bit."""
    pts, lens, means, stds = _notebook_case()
    betas = NC.log_sweep(count)
    r2s = O.level_major_to_rank(10)
    for n in (1, 2, 63, 65):
        ref = [CO.compress_coordinates(means[:n], stds[:n], b, pts, lens) for b in betas]
        want_idx = np.stack([r2s[slot] for _, slot in ref])
        want_val = np.stack([v for v, _ in ref])
        for values in (True, False):
            for off in OFFSETS:
                gi = G((count, n), torch.uint16, off)
                gv = G((count, n), torch.float32, off) if values else None
                call(lib, "vbq_quantize_notebook_f64", ptr(din(means[:n], off)), ptr(din(stds[:n], off)), n, ptr(din(pts, off)),
                     doubles(betas), count, 10, ptr(gi), ptr(gv), stream())
                what = f"notebook {count} betas n={n} values={values} off={off}"
                check(gi, want_idx, what + " idx")
                if gv is not None:
                    check(gv, want_val, what + " values")


# ==================================================================================================== F. records, top-k, bags
def _table(rng, n_tables, N):
    return np.sort(rng.standard_normal((n_tables, 2 ** (N + 1) - 1)).astype(F32), axis=1)


RECORD_SHAPES = [(1, 10, 7), (63, 10, 200), (65, 4, 100), (130, 10, 601)]        # (K, N, total_bits)


@pytest.mark.parametrize("K,N,total", RECORD_SHAPES)
def test_records_pack_and_unpack(ops, lib, K, N, total):
    """vbq_records_pack_u16 (one wave per row, the LDS image written with coalesced stores: records of 1 to 36 words) and
    vbq_records_unpack_f32 (every row, and listed rows in any order with a repeat; values and indices, each alone and both; one
    code book and one per column).  Inside: tests/records_reference.py and NumPy lookups."""
    rng = np.random.default_rng(K + N)
    R = 5
    idx = RR.random_indices(rng, R, K, N, total)
    words = RR.pack(idx, N, total).astype(np.uint32)
    RW = RR.record_words(K, N, total)
    row_ids = np.array([4, 0, 2, 0], np.int64)
    for off in OFFSETS:
        g, st = G((R, RW), torch.uint32, off), _status(off)
        ops.records_pack(din(idx, off), total, N, status=st.view, out=g.view)
        check(g, words, f"records_pack K={K} off={off}")
        check(st, [STATUS_SEED], "records_pack status")
        for n_tables in (1, K):
            table = _table(rng, n_tables, N)
            col = np.arange(K) if n_tables == K else np.zeros(K, np.int64)
            for ids in (None, row_ids):
                sel = idx if ids is None else idx[ids]
                rows = sel.shape[0]
                for wv, wi in ((True, False), (False, True), (True, True)):
                    gv = G((rows, K), torch.float32, off) if wv else None
                    gq = G((rows, K), torch.uint16, off) if wi else None
                    st = _status(off)
                    call(lib, "vbq_records_unpack_f32", ptr(din(words, off)), R, K, N, total, ptr(din(table, off)) if wv else None,
                         n_tables, None if ids is None else ptr(din(ids, off)), rows if ids is not None else 0, ptr(gv), ptr(gq),
                         ptr(st), stream())
                    what = f"records_unpack K={K} tables={n_tables} listed={ids is not None} off={off}"
                    if gv is not None:
                        check(gv, table[col[None, :], sel.astype(np.int64)], what + " values")
                    if gq is not None:
                        check(gq, sel, what + " idx")
                    check(st, [STATUS_SEED], what + " status")


@pytest.mark.parametrize("u8", FP.U8_CANARIES)
@pytest.mark.parametrize("max_workgroups", [1, 3])
def test_topk(lib, max_workgroups, u8):
    """vbq_topk_f32 / vbq_records_topk_f32: ids int64 [Q, k], scores f32 [Q, k] and the workspace at exactly
    vbq_topk_workspace_bytes, one workgroup per block of 32 queries and a row split of three; Q = 33 is a second block of one
    query, k = 64 the widest result.  Inside: tests/topk_reference.accept (the float64 order within the stated bounds)."""
    for K, V, Q, k in ((5, 31, 32, 10), (64, 33, 33, 64)):
        emb, q, exclude = TR.case_data(K, V, Q)
        for metric_name, metric in (("dot", 0), ("cosine", 1)):
            for off in OFFSETS:
                what = f"topk K={K} V={V} Q={Q} k={k} {metric_name} max_workgroups={max_workgroups} off={off}"
                nbytes = lib.vbq_topk_workspace_bytes(V, K, Q, k, max_workgroups)
                ws, gi, gs = WS(nbytes, u8), G((Q, k), torch.int64, off), G((Q, k), torch.float32, off)
                call(lib, "vbq_topk_f32", ptr(din(emb, off)), V, K, ptr(din(q, off)), Q, k, metric, ptr(din(exclude, off)),
                     exclude.shape[1], ptr(gi), ptr(gs), max_workgroups, ptr(ws), nbytes, stream())
                for g in (gi, gs, ws):
                    g.assert_outside_intact(what)
                TR.accept(gi.host(), gs.host(), q, emb, k, metric_name, exclude)
    # the record source: rows of N = 4 records, one code book
    K, N, total, V, Q, k = 65, 4, 100, 33, 33, 10
    rng = np.random.default_rng(9)
    idx = RR.random_indices(rng, V, K, N, total)
    words = RR.pack(idx, N, total).astype(np.uint32)
    table = _table(rng, 1, N)
    emb = table[0][idx.astype(np.int64)]
    q = rng.standard_normal((Q, K)).astype(F32)
    for off in OFFSETS:
        nbytes = lib.vbq_topk_workspace_bytes(V, K, Q, k, max_workgroups)
        ws, gi, gs, st = WS(nbytes, u8), G((Q, k), torch.int64, off), G((Q, k), torch.float32, off), _status(off)
        call(lib, "vbq_records_topk_f32", ptr(din(words, off)), V, K, N, total, ptr(din(table, off)), 1, ptr(din(q, off)), Q, k, 0,
             None, 0, ptr(gi), ptr(gs), ptr(st), max_workgroups, ptr(ws), nbytes, stream())
        for g in (gi, gs, ws):
            g.assert_outside_intact(f"records_topk off={off}")
        check(st, [STATUS_SEED], "records_topk status")
        TR.accept(gi.host(), gs.host(), q, emb, k, "dot", None)


@pytest.mark.parametrize("K", [1, 63, 65])
def test_bags(ops, K):
    """vbq_bag_f32 / vbq_records_bag_f32: f32 [n_bags, K] with K one lane, one short of a wave and one past it; bags of several
    entries, one entry, a padding entry and an EMPTY bag (its row is written: zeros); sum, mean, max and the weighted sum.
    Inside: tests/bag_reference.py, bit for bit."""
    rng = np.random.default_rng(K)
    V, N, total = 40, 4, min(4 * K, 2 * K + 1)
    idx = RR.random_indices(rng, V, K, N, total)
    words = RR.pack(idx, N, total).astype(np.uint32)
    table = _table(rng, 1, N)
    emb = table[0][idx.astype(np.int64)]
    ids = np.array([3, 7, 7, 39, -1, 0, 12, 5, 5, 5, 21], np.int64)
    offsets = np.array([0, 4, 4, 5, 6, 11], np.int64)                        # bag 1 is empty, bag 2 holds only padding
    weights = rng.standard_normal(ids.size).astype(F32)
    B = offsets.size - 1
    for mode, w in (("sum", None), ("mean", None), ("max", None), ("sum", weights)):
        want, _ = BG.bag(emb, ids, offsets, w, mode)
        for off in OFFSETS:
            d_w = None if w is None else din(w, off)
            what = f"bag K={K} {mode} weighted={w is not None} off={off}"
            g, st = G((B, K), torch.float32, off), _status(off)
            ops.bag(din(emb, off), din(ids, off), din(offsets, off), weights=d_w, mode=mode, status=st.view, out=g.view)
            check(g, want, what)
            check(st, [STATUS_SEED], what + " status")
            g, st = G((B, K), torch.float32, off), _status(off)
            ops.records_bag(din(words, off), K, N, total, din(table, off), din(ids, off), din(offsets, off), weights=d_w,
                            mode=mode, status=st.view, out=g.view)
            check(g, want, what + " (records)")
            check(st, [STATUS_SEED], what + " (records) status")


# ================================================================================================================ G. the rest
def _scores(rng, N, R, K):
    """Scores shaped like the real ones (tests/test_gpu_budget_dp.py): 0 at some depth, falling off steeply above it."""
    err = np.abs(rng.standard_normal((1, R, K))) * 2.0 ** (-np.arange(N + 1))[:, None, None] * rng.uniform(0.5, 2, (N + 1, R, K))
    return -0.5 * (err / np.exp(-3 + rng.standard_normal((1, R, K)))) ** 2


@functools.lru_cache(maxsize=None)
def _workspace_path_case():
    K, N, budget, R = 300, 16, 1600, 7
    fhat = _scores(np.random.default_rng(5), N, R, K)
    return fhat, BR.budget_dp_rows(fhat, budget)


def _budget_dp(lib, fhat, budget, nbytes, off, u8, what, want=None):
    N, R, K = fhat.shape[0] - 1, fhat.shape[1], fhat.shape[2]
    gb, go, st, ws = G((R, K), torch.int32, off), G((R,), torch.float64, off), _status(off), WS(nbytes, u8)
    call(lib, "vbq_budget_dp_f64", ptr(din(fhat, off)), R, K, N, budget, ptr(gb), ptr(go), ptr(st), ptr(ws), nbytes, stream())
    want_bits, want_obj = BR.budget_dp_rows(fhat, budget) if want is None else want
    check(gb, want_bits, what + " bits")
    check(go, want_obj, what + " objective")
    check(st, [STATUS_SEED], what + " status")
    ws.assert_outside_intact(what + " workspace")


@pytest.mark.parametrize("u8", FP.U8_CANARIES)
def test_budget_dp(lib, u8):
    """vbq_budget_dp_f64: bits int32 [rows, K] and objective f64 [rows] at K in {1, 7, 100} with the workspace
    vbq_budget_dp_workspace_bytes names (none: the back-pointers stay in LDS), and the workspace path of
    test_workspace_path_and_several_rounds_of_workgroups (K = 300, N = 16, budget 1600, 7 rows) with exactly one slice per
    row and with exactly two slices (four rounds).  Inside: tests/budget_reference.budget_dp_rows, bit for bit."""
    for K in (1, 7, 100):
        N, R = 10, 3
        fhat = _scores(np.random.default_rng(K), N, R, K)
        for budget in sorted({N, K * N // 3}):
            for off in OFFSETS:
                _budget_dp(lib, fhat, budget, lib.vbq_budget_dp_workspace_bytes(R, K, N, budget), off, u8,
                           f"budget_dp K={K} budget={budget} off={off}")
    K, N, budget, R = 300, 16, 1600, 7
    per_row = (K * (budget + 1) + 15) // 16 * 16
    assert lib.vbq_budget_dp_workspace_bytes(R, K, N, budget) == R * per_row
    fhat, want = _workspace_path_case()
    for nbytes in (R * per_row, 2 * per_row):
        _budget_dp(lib, fhat, budget, nbytes, 1, u8, f"budget_dp workspace of {nbytes} bytes", want)


@pytest.mark.parametrize("E", [1, 5, 257])
def test_budget_patience(lib, E):
    """vbq_budget_patience_f64: bits int32 [E] and g f64 [E].  Inside: tests/budget_reference.patience_scan, bit for bit."""
    N = 10
    fhat = _scores(np.random.default_rng(E), N, 1, E)[:, 0, :]
    for lamb, patience in ((0.05, 3), (2.0, 1)):
        want_b, want_g = BR.patience_scan(fhat, lamb, patience)
        for off in OFFSETS:
            gb, gg = G((E,), torch.int32, off), G((E,), torch.float64, off)
            call(lib, "vbq_budget_patience_f64", ptr(din(fhat, off)), E, N, C.c_double(lamb), patience, ptr(gb), ptr(gg), stream())
            check(gb, want_b, f"budget_patience E={E} off={off} bits")
            check(gg, want_g, f"budget_patience E={E} off={off} g")


@pytest.mark.parametrize("n", [1, 5, 257])
def test_argmax_candidates(lib, n):
    """vbq_argmax_candidates_f32: j int32, Z_hat and lengths f32, each [L, n], every subset of them, L = 3 and 9 (a second chunk
    of lambdas, of one), both score modes, shared and per-lambda lengths.  Inside: np.argmax of oracle.rd_f64.score."""
    from oracle import rd_f64 as R
    rng = np.random.default_rng(n)
    M = 21
    mu = (rng.integers(-40, 40, n) / 8).astype(F32)
    sg = np.exp(rng.normal(-1, 1, n)).astype(F32)
    P = (mu[None] + rng.integers(-256, 256, (M, n)) / 64).astype(F32)
    for L in (3, 9):
        lam = list(np.geomspace(1e-3, 10.0, L) * np.sqrt(2.0))
        for per_lambda in (0, 1):
            lens = rng.integers(0, 12, (L, M, n) if per_lambda else (M, n)).astype(F32)
            for mode_name, mode in (("f32", 0), ("f64", 1)):
                j = np.stack([np.argmax(R.score(P, lens[i] if per_lambda else lens, mu[None], sg[None], lam[i], mode_name), axis=0)
                              for i in range(L)])
                want = (j, np.stack([np.take_along_axis(P, j[i][None], 0)[0] for i in range(L)]),
                        np.stack([np.take_along_axis(lens[i] if per_lambda else lens, j[i][None], 0)[0] for i in range(L)]))
                for combo in range(1, 8):
                    for off in OFFSETS:
                        gs = [G((L, n), dt, off) if combo >> b & 1 else None
                              for b, dt in enumerate((torch.int32, torch.float32, torch.float32))]
                        call(lib, "vbq_argmax_candidates_f32", ptr(din(P, off)), ptr(din(lens, off)), per_lambda, ptr(din(mu, off)),
                             ptr(din(sg, off)), n, doubles(lam), L, M, mode, ptr(gs[0]), ptr(gs[1]), ptr(gs[2]), stream())
                        for g, w in zip(gs, want):
                            if g is not None:
                                check(g, w, f"argmax_candidates n={n} L={L} {mode_name} per_lambda={per_lambda} {combo:03b} "
                                            f"off={off}")


@pytest.mark.parametrize("K", [1, 5, 257])
def test_xi_intervals_and_select(lib, K):
    """vbq_xi_intervals_f64 (left / right f64 [N + 1, K]) and vbq_xi_select_f64 (z_hat, xi_hat, f_z_hat f64 [K], num_bits int64
    [K]).  Inside: oracle.vbq_oracle.xi_intervals and NumPy's argmax as utils.py:288-303 writes the selection."""
    N = 16
    rng = np.random.default_rng(K)
    xi = rng.random(K)
    L_, R_ = O.xi_intervals(xi, N)
    ends = np.stack([L_, R_])
    unsq = np.log(ends / (1 - ends))
    F = -0.5 * ((unsq - rng.standard_normal(K)) / 0.3) ** 2
    lamb = 0.05
    cols = np.arange(K)
    am = np.argmax(F, axis=0)
    sel = (am, np.arange(N + 1)[:, None], cols[None, :])
    reg = F[sel] - lamb * np.arange(N + 1)[:, None]
    nb = np.argmax(reg, axis=0)
    for off in OFFSETS:
        gl, gr = G((N + 1, K), torch.float64, off), G((N + 1, K), torch.float64, off)
        call(lib, "vbq_xi_intervals_f64", ptr(din(xi, off)), K, N, ptr(gl), ptr(gr), stream())
        check(gl, L_, f"xi_intervals K={K} off={off} left")
        check(gr, R_, f"xi_intervals K={K} off={off} right")
        gz, gx, gf, gn = (G((K,), dt, off) for dt in (torch.float64, torch.float64, torch.float64, torch.int64))
        call(lib, "vbq_xi_select_f64", ptr(din(F, off)), ptr(din(ends, off)), ptr(din(unsq, off)), K, N, C.c_double(lamb), ptr(gz),
             ptr(gn), ptr(gx), ptr(gf), stream())
        for g, w, name in ((gz, unsq[sel][nb, cols], "z_hat"), (gx, ends[sel][nb, cols], "xi_hat"), (gn, nb, "num_bits"),
                           (gf, reg[nb, cols], "f_z_hat")):
            check(g, w, f"xi_select K={K} off={off} {name}")


@pytest.mark.parametrize("n", [1, 5, 257])
def test_comparison_quantizers(lib, n):
    """vbq_uniform_quantize_f32 (index and value f32 [n], counts int64 [levels] added to) and vbq_nearest_code_f64 (index int32,
    value f64, counts int64 [n_codes] added to), every subset of the outputs.  Inside: oracle.vbq_oracle.uniform_quantize /
    nearest_code; the counts start from a pattern."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal(max(n, 2)).astype(F32)
    levels = 7
    fit = O.uniform_fit(x, levels)
    x = x[:n]
    wq, wI, _ = O.uniform_quantize(x, fit)
    offset = F32(fit["min"] + fit["delta"] / 2)
    codes = np.sort(rng.standard_normal(9))
    cq, cI = O.nearest_code(x, codes)
    for combo in range(1, 8):
        for off in OFFSETS:
            gi, gv = (G((n,), torch.float32, off) if combo >> b & 1 else None for b in range(2))
            gc = G((levels,), torch.int64, off).fill(pattern((levels,), np.int64)) if combo & 4 else None
            call(lib, "vbq_uniform_quantize_f32", ptr(din(x, off)), n, C.c_float(float(fit["min"])), C.c_float(float(fit["delta"])),
                 C.c_float(float(offset)), levels, ptr(gi), ptr(gv), ptr(gc), stream())
            what = f"uniform_quantize n={n} {combo:03b} off={off}"
            counts = pattern((levels,), np.int64) + np.bincount(wI.astype(np.int32), minlength=levels)
            for g, w in ((gi, wI), (gv, wq), (gc, counts)):
                if g is not None:
                    check(g, w, what)
            gi = G((n,), torch.int32, off) if combo & 1 else None
            gv = G((n,), torch.float64, off) if combo & 2 else None
            gc = G((9,), torch.int64, off).fill(pattern((9,), np.int64)) if combo & 4 else None
            call(lib, "vbq_nearest_code_f64", ptr(din(x, off)), n, ptr(din(codes, off)), 9, ptr(gi), ptr(gv), ptr(gc), stream())
            what = f"nearest_code n={n} {combo:03b} off={off}"
            for g, w in ((gi, cI), (gv, cq), (gc, pattern((9,), np.int64) + np.bincount(cI, minlength=9))):
                if g is not None:
                    check(g, w, what)


def test_n_bit_intervals(lib):
    """vbq_n_bit_intervals_f32: left / right f32 [C, N + 1, rows] at rows 1, 5 and 513 (the planes of the levels are rows apart:
    odd strides).  Inside: oracle.vbq_oracle.get_all_N_bit_intervals on the padded search grids."""
    N, Cc = 10, 3
    for rows in (1, 5, 513):
        tab, mu, _ = solve_data(rows, Cc, N)
        want_l, want_r = O.get_all_N_bit_intervals(SC.search_grids(tab, N), mu)
        for off in OFFSETS:
            gl, gr = G((Cc, N + 1, rows), torch.float32, off), G((Cc, N + 1, rows), torch.float32, off)
            call(lib, "vbq_n_bit_intervals_f32", ptr(din(mu.T, off)), rows, Cc, ptr(din(tab, off)), N, ptr(gl), ptr(gr), stream())
            check(gl, want_l, f"n_bit_intervals rows={rows} off={off} left")
            check(gr, want_r, f"n_bit_intervals rows={rows} off={off} right")


@pytest.mark.parametrize("n", [1, 4, 7, 1000])
def test_packed_counters(lib, n):
    """vbq_pack_counts_3x21 / vbq_unpack_counts_3x21: (n + 2) / 3 words whose last one holds one, two or three fields, and the
    n counts back (the last word's missing fields must not be stored).  Inside: the three 21-bit fields in NumPy."""
    c = np.random.default_rng(n).integers(0, 1 << 19, n).astype(np.int32)
    nw = (n + 2) // 3
    f = np.zeros(3 * nw, np.uint64)
    f[:n] = c
    words = (f[0::3] | f[1::3] << np.uint64(21) | f[2::3] << np.uint64(42)).view(np.int64)
    for off in OFFSETS:
        gw, fl = G((nw,), torch.int64, off), _status(off)
        call(lib, "vbq_pack_counts_3x21", ptr(din(c, off)), n, ptr(gw), 2, ptr(fl), stream())
        check(gw, words, f"pack_counts n={n} off={off}")
        check(fl, [STATUS_SEED], f"pack_counts n={n} off={off} overflow flag")
        gc = G((n,), torch.int32, off)
        call(lib, "vbq_unpack_counts_3x21", ptr(din(words, off)), n, ptr(gc), stream())
        check(gc, c, f"unpack_counts n={n} off={off}")


def test_bmshj_kernels(ops, lib):
    """The BMSHJ2018 prior kernels.  vbq_bmshj_cdf_pdf_f32: each of its three outputs alone and all together, unstaged (37 x 5)
    and staged (300 x 7) -- inside: oracle/bmshj_f64.py within the bounds of tests/test_gpu_bmshj.py.  vbq_bmshj_nll_grad_f32
    adds into f64 [C, 44]: a pattern first, inside the same module's bounds around pattern + reference.  vbq_bmshj_icdf_step_f32
    / _chain_f32 update left / right in place and write mid and the flags: their own module has no closed-form reference (it
    pins the chain to the step loop), so the inside is the plain call on fresh tensors, bit for bit."""
    import test_gpu_bmshj as TB
    from oracle import bmshj_f64 as R
    for rows, Cc in ((37, 5), (300, 7)):
        params_t = TB._prior(Cc, 10.0, seed=Cc)._params()
        params = params_t.cpu().numpy()
        rng = np.random.default_rng(rows)
        x = (rng.standard_normal((rows, Cc)) * 3).astype(F32)
        x_t = torch.from_numpy(x).cuda()
        c64, p64 = R.cdf64(params_t, x_t), R.pdf64(params_t, x_t)
        pmax = R.pdf_max64(params_t, x_t)
        bounds = (TB.CDF_TOL, (TB.PDF_TOL * pmax).expand_as(p64).cpu().numpy(),
                  (TB.PDF_TOL * pmax / (p64 + 1e-10) + 1e-6).cpu().numpy())
        wants = (c64.cpu().numpy(), p64.cpu().numpy(), torch.log(p64 + 1e-10).cpu().numpy())
        for combo in (1, 2, 4, 7):
            for off in OFFSETS:
                gs = [G((rows, Cc), torch.float32, off) if combo >> b & 1 else None for b in range(3)]
                call(lib, "vbq_bmshj_cdf_pdf_f32", ptr(din(params, off)), ptr(din(x, off)), rows, Cc, ptr(gs[0]), ptr(gs[1]),
                     ptr(gs[2]), stream())
                for g, w, b in zip(gs, wants, bounds):
                    if g is not None:
                        _close(g, w, b, f"bmshj_cdf_pdf {rows}x{Cc} {combo:03b} off={off}")
        # bisection: one step, then a chain of five
        xi = (rng.random((rows, Cc)) * 0.998 + 0.001).astype(F32)
        for off in OFFSETS:
            for chain in (0, 5):
                nflag = (chain + 1, 2) if chain else (2,)
                flags0 = np.zeros(nflag, np.uint32)
                if not chain:
                    flags0[:] = [0, 0x7f800000]
                gl = G((rows, Cc), torch.float32, off).fill(np.full((rows, Cc), -8.0, F32))
                gr = G((rows, Cc), torch.float32, off).fill(np.full((rows, Cc), 8.0, F32))
                gm, gf = G((rows, Cc), torch.float32, off), G(nflag, torch.uint32, off).fill(flags0)
                plain = [torch.full((rows, Cc), -8.0, device=DEV), torch.full((rows, Cc), 8.0, device=DEV),
                         torch.zeros((rows, Cc), device=DEV), din(flags0)]
                for left, right, mid, flags in ((gl.view, gr.view, gm.view, gf.view), plain):
                    if chain:
                        ops.bmshj_icdf_chain(din(params, off), din(xi, off), left, right, mid, flags, chain, 1e-9, True)
                    else:
                        ops.bmshj_icdf_step(din(params, off), din(xi, off), left, right, mid, flags)
                torch.cuda.synchronize()
                for g, t, name in zip((gl, gr, gm, gf), plain, ("left", "right", "mid", "flags")):
                    t = t.view(torch.int32) if t.dtype == torch.uint32 else t
                    check(g, t.cpu().numpy(), f"bmshj_icdf {'chain' if chain else 'step'} {rows}x{Cc} off={off} {name}")
    for Cc, n in ((1, 1), (3, 257)):
        params_t = TB._prior(Cc, 10.0, seed=Cc + n, sd=0.2)._params()
        x_cb = TB._nll_data(params_t, Cc, n, seed=n)
        ref, absg = R.nll_grad64(params_t, x_cb)
        lg = R.logits64(params_t.double(), x_cb.double().t())
        bound = torch.cat([1e-4 * absg[:, :43], (1e-5 * absg[:, 43] + (2.0 ** -24 * (1 + torch.exp(lg))).sum(dim=0))[:, None]], 1)
        for off in OFFSETS:
            g = G((Cc, 44), torch.float64, off).fill(pattern((Cc, 44), np.float64))
            ops.bmshj_nll_grad(din(params_t.cpu().numpy(), off), din(x_cb.cpu().numpy(), off), out=g.view)
            torch.cuda.synchronize()
            _close(g, pattern((Cc, 44), np.float64) + ref.cpu().numpy(), bound.cpu().numpy() + 1e-12,
                   f"bmshj_nll_grad C={Cc} n={n} off={off}")


# ====================================================================== H. the batch (*_files_u16) and window (*_window_f32) calls
# The case builders are those of the entry points' own modules; here their outputs get outer guards on both sides.
def _zeros(n, off):
    """A status array (OR-ed into) / a totals array (added to) that starts from zero, guarded."""
    return G((n,), torch.uint32, off).fill(np.zeros(n, np.uint32))


def test_batch_encode_of_segment_files(ops):
    """vbq_rans_encode_files_u16 and vbq_rans_sizes_files_u16 on the "rows-and-tables" / "rows-and-lambdas" cases of
    tests/test_gpu_encode_files.py and tests/test_gpu_budget_batch.py (tight layout: unaligned plane bases): words u16
    [M, seg + 2], sizes u32 [M], status u32 [F], totals u64 [L, F] (added to: a pattern first).  Inside: those modules'
    references (the C checker's words and sizes; words past a segment's size still canary)."""
    import test_gpu_budget_batch as BB
    import test_gpu_encode_files as EF
    rows, tables, n_tables, C_, seg, bits, _ = EF.KERNEL_CASES["rows-and-tables"]
    k = EF.Batch(rows, tables, n_tables, C_, seg, bits, seed=3, tight=True)
    assert EF.WORD == FP.canary(torch.uint16)                     # check_file wants the words past a size as they were
    p = k.plan
    for off in OFFSETS:
        gw, gs, st = G((p.M, seg + 2), torch.uint16, off), G((p.M,), torch.uint32, off), _zeros(len(rows), off)
        ops.rans_encode_files(k.d_idx, din(k.files), din(p.items), k.d_freq, p.M, seg=seg, N=bits, words=gw.view, sizes=gs.view,
                              status=st.view)
        torch.cuda.synchronize()
        for g in (gw, gs, st):
            g.assert_outside_intact(f"rans_encode_files off={off}")
        check(st, np.zeros(len(rows)), "rans_encode_files status")
        for f in range(len(rows)):
            k.check_file(f, gw.host(), gs.host())
    rows, L, C_, seg, bits, _ = BB.KERNEL_CASES["rows-and-lambdas"]
    k = BB.Batch(rows, L, C_, seg, bits, seed=4, tight=True)
    items = np.concatenate([k.plan.items, np.full((-k.plan.items.shape[0] % 64, 2), -1, np.int32)])
    for off in OFFSETS:
        gt, st = G((L, len(rows)), torch.uint64, off).fill(pattern((L, len(rows)), np.uint64)), _zeros(len(rows), off)
        ops.rans_sizes_files(k.d_idx, din(k.files), din(items), k.d_freq, lambda_stride=k.stride_l, seg=seg, N=bits,
                             totals=gt.view, status=st.view)
        torch.cuda.synchronize()
        check(gt, pattern((L, len(rows)), np.uint64) + k.want, f"rans_sizes_files off={off} totals")
        check(st, np.zeros(len(rows)), "rans_sizes_files status")


def test_batch_encode_of_mapped_files(ops):
    """vbq_rans_map_encode_files_u16, vbq_rans_map_sizes_files_u16 (the mixed palettes of tests/test_gpu_mapped_batch.py, tight
    layout) and vbq_rans_map_rates_files_u16 (six candidates of two classes, tests/test_gpu_mapped_budget.py): words, sizes,
    status, and totals u64 [K, F] added to a pattern.  Inside: those modules' references (tests/mapped_reference.py)."""
    import test_gpu_mapped_batch as MB
    import test_gpu_mapped_budget as MG
    k = MB.fitted_batch(**MB.MIXED, bits=10, seed=11, round_=1, tight=True)
    p, F = k.plan, len(k.rows)
    assert MB.WORD == FP.canary(torch.uint16)
    for off in OFFSETS:
        gw, gs, st = G((p.M, k.seg + 2), torch.uint16, off), G((p.M,), torch.uint32, off), _zeros(F, off)
        gs2, st2 = G((p.M,), torch.uint32, off), _zeros(F, off)
        args = (k.d_idx, k.d_cls, din(k.files), din(k.pal_rows), din(p.items), k.d_freq, p.M)
        kw = dict(seg=k.seg, max_classes=k.max_classes, N=k.bits)
        ops.rans_map_encode_files(*args, words=gw.view, sizes=gs.view, status=st.view, **kw)
        ops.rans_map_sizes_files(*args, sizes=gs2.view, status=st2.view, **kw)
        torch.cuda.synchronize()
        for g in (gw, gs, st, gs2, st2):
            g.assert_outside_intact(f"rans_map_encode / sizes_files off={off}")
        same(gs2.host(), gs.host(), "rans_map_sizes_files against the encode's sizes")
        check(st, np.zeros(F), "rans_map_encode_files status")
        check(st2, np.zeros(F), "rans_map_sizes_files status")
        for f in range(F):
            k.check_file(f, gw.host(), gs.host())
    r = MG.fitted(MG.SIX[2], 5, seed=21, tight=True)
    K, F = len(r.cands), len(r.rows)
    for off in OFFSETS:
        gt, st = G((K, F), torch.uint64, off).fill(pattern((K, F), np.uint64)), _zeros(F, off)
        ops.rans_map_rates_files(r.d_idx, r.d_cls, din(r.files), din(r.rows4()), din(r.plan.items), r.d_freq,
                                 lambda_stride=r.stride_l, seg=r.seg, max_classes=2, N=r.bits, totals=gt.view, status=st.view)
        torch.cuda.synchronize()
        check(gt, pattern((K, F), np.int64) + r.want, f"rans_map_rates_files off={off} totals")
        check(st, np.zeros(F), "rans_map_rates_files status")


def test_batch_of_compact_files(ops):
    """vbq_rans_il_sizes_files_u16 / _encode_files_u16 / _decode_files_u16 on the three files of tests/test_gpu_compact_files.py
    and vbq_rans_il_rates_files_u16 on the three planes of tests/test_gpu_compact_rates_files.py: sizes u32 [P_all] and
    [L, P_all], the payload of exactly the sum of the sizes, the index matrix of which only the files' columns may change (the
    sentinel columns around them are canary here), status.  Inside: tests/interleaved_reference.py through those builders."""
    import test_gpu_compact_files as CF
    import test_gpu_compact_rates_files as CR
    b = CF.Batch(*CF._three(10), 10)
    for off in OFFSETS:
        d_idx, d_files, d_items, d_freq = din(b.matrix.reshape(-1), off), din(b.files), din(b.items), din(b.freq, off)
        gs, st = G((b.P_all,), torch.uint32, off), _zeros(b.F, off)
        ops.rans_il_sizes_files(d_idx, d_files, d_items, d_freq, b.P_all, N=b.N, sizes=gs.view, status=st.view)
        torch.cuda.synchronize()
        check(gs, b.sizes, f"rans_il_sizes_files off={off}")
        check(st, np.zeros(b.F), "rans_il_sizes_files status")
        gp, st = G((b.payload.size,), torch.uint16, off), _zeros(b.F, off)
        ops.rans_il_encode_files(d_idx, d_files, d_items, d_freq, din(b.sizes, off), din(b.offsets, off), gp.view, N=b.N,
                                 status=st.view)
        torch.cuda.synchronize()
        check(gp, b.payload, f"rans_il_encode_files off={off}")
        check(st, np.zeros(b.F), "rans_il_encode_files status")
        gi, st = G((b.C * b.W,), torch.uint16, off), _zeros(b.F, off)
        ops.rans_il_decode_files(din(b.payload, off), din(b.sizes, off), din(b.offsets, off), d_files, d_items, d_freq, gi.view,
                                 N=b.N, status=st.view)
        torch.cuda.synchronize()
        check(gi, b.matrix.reshape(-1), f"rans_il_decode_files off={off}", b.matrix.reshape(-1) != CF.SENTINEL)
        check(st, np.zeros(b.F), "rans_il_decode_files status")
    r = CR.Planes(*CR._fitted(10), 10)
    for off in OFFSETS:
        gs, st = G((CR.L_, r.P_all), torch.uint32, off), _zeros(r.F, off)
        ops.rans_il_rates_files(din(r.array, off), din(r.files), din(r.items), din(r.freq, off), r.P_all, lambda_stride=r.stride,
                                N=r.N, sizes=gs.view, status=st.view)
        torch.cuda.synchronize()
        check(gs, r.sizes, f"rans_il_rates_files off={off}")
        check(st, np.zeros(r.F), "rans_il_rates_files status")


def test_window_decodes(ops):
    """vbq_rans_decode_window_f32 and vbq_rans_map_decode_window_f32 on the three-file batches of tests/test_gpu_window.py and
    tests/test_gpu_mapped_window.py: out f32 [F, w0, w1, w2, C_sel] and status u32 [F], all channels and a channel list with a
    repeat.  Every position of these boxes is covered by a listed segment, so the region is the whole output.  Inside: those
    modules' references (sorted[c][idx] of the symbols that were coded).  d_cls stays 8-byte aligned, as the header demands."""
    import test_gpu_mapped_window as MW
    import test_gpu_window as W
    from vbq_amd import bitstream as bs
    shapes = [(1, 17, 23), (1, 20, 30), (2, 9, 11)]
    k = W.Coded(shapes, [0, 1, 0], 2, 8, 64, 10, seed=5)
    boxes, _ = bs.region_boxes(shapes, MW.REGIONS3)
    lists = [bs.box_segments(d, lo, hi, k.seg) for d, lo, hi in boxes]
    segs = np.full((3, max(l.size for l in lists)), -1, np.int32)
    for f, l in enumerate(lists):
        segs[f, :l.size] = l
    files = np.array([[b, int(np.prod(s)), d[1], d[2], lo[0], lo[1], lo[2], t]
                      for b, s, (d, lo, hi), t in zip(k.seg_base, shapes, boxes, k.tables)], np.int64)
    box = tuple(h - l for l, h in zip(boxes[0][1], boxes[0][2]))
    rng = np.random.default_rng(17)
    m = MW.MappedCoded([(MW.SHAPES3[0], [2], None), (MW.SHAPES3[1], [0, 3], rng.integers(0, 2, 600).astype(np.uint8)),
                        (MW.SHAPES3[2], [1, 4, 0, 2], rng.integers(0, 4, 198).astype(np.uint8))], 5, 8, 64, 10, seed=11)
    m_files, m_segs, m_box, _, _ = m.stage(MW.REGIONS3)
    for channels in (None, [7, 0, 7]):
        n_sel = 8 if channels is None else len(channels)
        for off in OFFSETS:
            ch = None if channels is None else din(np.array(channels, np.int32), off)
            g, st = G((3,) + box + (n_sel,), torch.float32, off), _zeros(3, off)
            ops.rans_decode_window(k.payload, k.sizes, k.offsets, din(files), din(segs, off), k.d_freq, k.d_values, box, seg=k.seg,
                                   N=k.bits, channels=ch, status=st.view, out=g.view)
            torch.cuda.synchronize()
            check(g, k.want(MW.REGIONS3, channels).reshape(g.shape), f"rans_decode_window channels={channels} off={off}")
            check(st, np.zeros(3), "rans_decode_window status")
            g, st = G((3,) + m_box + (n_sel,), torch.float32, off), _zeros(3, off)
            ops.rans_map_decode_window(m.payload, m.sizes, m.offsets, din(m_files), din(m_segs, off), m.d_freq, m.d_values,
                                       din(m.area_host), m_box, seg=m.seg, max_classes=m.max_P, N=m.bits, channels=ch,
                                       status=st.view, out=g.view)
            torch.cuda.synchronize()
            check(g, m.want(MW.REGIONS3, channels).reshape(g.shape), f"rans_map_decode_window channels={channels} off={off}")
            check(st, np.zeros(3), "rans_map_decode_window status")


@pytest.mark.parametrize("n", [1, 3, 5, 1023])
def test_pixel_conversions(lib, n):
    """vbq_unit_to_u8_f32 (byte stores: with either byte canary around and, before the call, inside the output) and
    vbq_u8_to_f64 at n in {1, 3, 5, 1023}: a lone byte, odd counts on either side of a dword, one short of 1024.  Inside:
    NumPy's clip(round(x * 255)) and astype(float64)."""
    rng = np.random.default_rng(n)
    x = rng.uniform(-0.1, 1.1, n).astype(F32)
    want = np.clip(np.round(x * F32(255)), 0, 255).astype(np.uint8)
    u = rng.integers(0, 256, n).astype(np.uint8)
    for off in OFFSETS:
        for u8 in FP.U8_CANARIES:
            g = G((n,), torch.uint8, off, u8=u8)
            call(lib, "vbq_unit_to_u8_f32", ptr(din(x, off)), n, ptr(g), stream())
            check(g, want, f"unit_to_u8 n={n} off={off} canary {u8:#x}")
        g = G((n,), torch.float64, off)
        call(lib, "vbq_u8_to_f64", ptr(din(u, off)), n, ptr(g), stream())
        check(g, u.astype(np.float64), f"u8_to_f64 n={n} off={off}")


@pytest.mark.parametrize("u8", FP.U8_CANARIES)
def test_image_metrics(lib, u8):
    """vbq_downsample2_f64 at odd H and W (the clamped last row and column), vbq_image_sqerr_u8 (int64 [B]),
    vbq_ssim_scale_f64 (f64 [B] twice, the workspace at exactly vbq_ssim_scale_workspace_bytes) and vbq_analogy_ranks_f32
    (int64 [Q], the workspace at exactly vbq_analogy_ranks_workspace_bytes).  Inside: oracle.vbq_oracle.downsample2 and the
    integer sum bit for bit, oracle/metrics_f64.ssim_scale_ld within ssim_scale_error_bound, the C oracle's fma-chain ranks."""
    from oracle import metrics_f64 as MR
    from vbq_amd import metrics
    rng = np.random.default_rng(3)
    for off in OFFSETS:
        for shape in ((2, 5, 7, 3), (1, 1, 1, 1), (1, 3, 1, 2)):
            im = rng.random(shape)
            B, H, W, Cc = shape
            g = G((B, (H + 1) // 2, (W + 1) // 2, Cc), torch.float64, off)
            call(lib, "vbq_downsample2_f64", ptr(din(im, off)), B, H, W, Cc, ptr(g), stream())
            check(g, O.downsample2(im), f"downsample2 {shape} off={off}")
        B, n = 3, 1001
        a, b = rng.integers(0, 256, (B, n)).astype(np.uint8), rng.integers(0, 256, (B, n)).astype(np.uint8)
        g = G((B,), torch.int64, off)
        call(lib, "vbq_image_sqerr_u8", ptr(din(a, off)), ptr(din(b, off)), B, n, ptr(g), stream())
        d = a.astype(np.int64) - b
        check(g, (d * d).sum(1), f"image_sqerr off={off}")
        # one SSIM scale
        B, H, W, Cc, size = 2, 20, 23, 3, 11
        x = rng.integers(0, 256, (B, H, W, Cc)).astype(np.float64)
        y = np.clip(x + rng.integers(-30, 31, x.shape), 0, 255)
        win = metrics._gauss_1d(size, 1.5)
        nbytes = lib.vbq_ssim_scale_workspace_bytes(B, H, W, Cc, size)
        ws, gs, gc = WS(nbytes, u8), G((B,), torch.float64, off), G((B,), torch.float64, off)
        call(lib, "vbq_ssim_scale_f64", ptr(din(x, off)), ptr(din(y, off)), B, H, W, Cc, ptr(din(win, off)), size,
             C.c_double((0.01 * 255) ** 2), C.c_double((0.03 * 255) ** 2), ptr(gs), ptr(gc), ptr(ws), nbytes, stream())
        rs, rc = MR.ssim_scale_ld(x, y, max_val=255, filter_size=size)
        Ho, Wo = H - size + 1, W - size + 1
        bs, bc = MR.ssim_scale_error_bound(size, 255.0, 255, 0.01, 0.03, n_per_image=Ho * Wo * Cc,
                                           n_partials=Cc * -(-Ho // 16) * -(-Wo // 16))
        _close(gs, rs, bs, f"ssim_scale off={off} ssim")
        _close(gc, rc, bc, f"ssim_scale off={off} cs")
        ws.assert_outside_intact(f"ssim_scale off={off} workspace")
        # analogy ranks
        V, K, Q = 50, 7, 5
        emb = rng.standard_normal((V, K)).astype(F32)
        an = rng.integers(0, V, (Q, 4)).astype(np.int32)
        nbytes = lib.vbq_analogy_ranks_workspace_bytes(V, K, Q)
        ws, g = WS(nbytes, u8), G((Q,), torch.int64, off)
        call(lib, "vbq_analogy_ranks_f32", ptr(din(emb, off)), V, K, ptr(din(an, off)), Q, ptr(g), ptr(ws), nbytes, stream())
        check(g, CO.analogy_ranks(emb, an), f"analogy_ranks off={off}")
        ws.assert_outside_intact(f"analogy_ranks off={off} workspace")
