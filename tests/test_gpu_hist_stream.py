"""K2 (the rank histogram, vbq_hist.hip) at every seam of its load path, against np.bincount.

Counts are integers and models are table lookups of them: every comparison is exact equality.  The reference is
np.bincount per (lambda, channel) row; the fused models are compared with ops.code_lengths_from_counts on those counts.

The row lengths were laid out for `k_hist_stream`, a second load path through a per-wave LDS ring (512 threads, D = 4 slots of
one wave-stage = 64 octets = 512 indices; a workgroup-stage is 4096 indices).  It passed every case of this file and was
measured slower than k_hist_flat, so it is not in the library (EXPERIMENTS.md, "K2 through an LDS ring"); the cases stay
because they are seams of k_hist_flat too -- whole and partial 16-byte loads, the sub-octet tail, the head of rows that start
off a 16-byte boundary, waves with different numbers of stages -- and three lengths are added at k_hist_flat's own stage of
3 loads x 512 threads = 12288 indices.  Two grids:
  * L C >= 2048 rows of bins (L = 2, C = 1024): ONE workgroup per row.  Both the plain histogram (assign 0: atomics into
    zeroed counts) and the fused histogram_models (assign 2: the reverse channel walk, counts stored, with and without the
    model lookup) take this shape.
  * L = 2, C = 3: the plain histogram puts several workgroups on a row.
assign 1 is not reachable through the library (it needs more than 65535 channels, which the entry point refuses).
Odd row lengths shift every other row two bytes off a 16-byte boundary: the head path; the index tensor is exactly
L C n elements, so the last row ends where the allocation ends.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu]
N = 10
T = 2047
D = 4
STAGE = 4096                       # indices per workgroup-stage: 8 waves x 64 lanes x 8

FLAT_STAGE = 3 * 512 * 8           # indices per register stage of k_hist_flat with one workgroup on the row

LENGTHS = {
    "below_one_stage": STAGE - 8,              # seven wave-stages for eight waves
    "one_stage": STAGE,                        # fewer than D stages per wave
    "d_stages": D * STAGE,                     # exactly the ring, no steady iteration
    "d_stages_1_octet": D * STAGE + 8,         # + a partial wave-stage of one octet
    "wrap_tail7": (D + 1) * STAGE + 7,         # the ring wraps; 7 indices behind the last octet; odd: heads
    "ragged_odd": 2 * STAGE + 3 * 512 + 13,    # three waves have one stage more than the others; odd: heads
    "kodak_row": 36864,                        # the real row: 9 workgroup-stages, 3 register stages
    "flat_one_stage": FLAT_STAGE,              # k_hist_flat: one register stage, no refill
    "flat_two_stages_1_octet": 2 * FLAT_STAGE + 8,     # the odd stage behind a pair, one lane with one more load
    "flat_below_stage_odd": FLAT_STAGE - 3,    # no whole stage: single loads, partial wave, tail of 5, heads
}
CONTENTS = ["random", "equal", "ramp", "skew90"]
# every length once, the contents in turn; every content at the length that has all edges at once
CASES = [(k, CONTENTS[i % 4]) for i, k in enumerate(LENGTHS)] + [("wrap_tail7", c) for c in CONTENTS if c != "random"]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    from vbq_amd import ops as _ops
    return _ops


def make_indices(L, C, n, content, seed):
    rng = np.random.default_rng(seed)
    shape = (L, C, n)
    if content == "random":
        return rng.integers(0, T, shape, dtype=np.uint16)
    if content == "equal":                                      # one bin per row (the ballot-merge path), another per row
        return np.broadcast_to(rng.integers(0, T, (L, C, 1), dtype=np.uint16), shape).copy()
    if content == "ramp":                                       # all of 0..2046 in order, each row from its own start
        start = rng.integers(0, T, (L, C, 1), dtype=np.int32)
        return ((start + np.arange(n, dtype=np.int32)[None, None, :]) % T).astype(np.uint16)
    assert content == "skew90"                                  # 90 % one bin, the rest uniform
    idx = rng.integers(0, T, shape, dtype=np.uint16)
    keep = rng.random(shape, dtype=np.float32) < 0.9
    idx[keep] = 2046
    return idx


def reference_counts(idx):
    L, C, _ = idx.shape
    return np.stack([[np.bincount(idx[l, c], minlength=T) for c in range(C)] for l in range(L)])


def check_all_modes(ops, L, C, key, content, fused):
    n = LENGTHS[key]
    idx_h = make_indices(L, C, n, content, seed=n + 17 * C)
    want = reference_counts(idx_h)
    assert want.shape == (L, C, T) and int(want.sum()) == L * C * n
    idx = torch.from_numpy(idx_h).cuda()
    assert idx.numel() == L * C * n
    for dtype in (torch.int64, torch.int32):
        got = ops.histogram(idx, C, N=N, layout="cb", out=torch.zeros((L, C, T), dtype=dtype, device="cuda"))
        assert np.array_equal(got.cpu().numpy(), want), ("histogram", dtype, key, content)
    if not fused:
        return
    lut = torch.rand(n + 1, device="cuda")
    for dtype in (torch.int64, torch.int32):
        want_t = torch.from_numpy(want).to(dtype).cuda()
        want_m = ops.code_lengths_from_counts(want_t, lut, want_len=False, want_model=True)
        cnt = torch.full((L, C, T), -5, dtype=dtype, device="cuda")                  # assigned, not added
        ops.histogram_models(idx, C, cnt, N=N)
        assert torch.equal(cnt, want_t), ("histogram_models", dtype, key, content)
        cnt = torch.full((L, C, T), -5, dtype=dtype, device="cuda")
        mdl = torch.full((L, C, T), -1.0, dtype=torch.float32, device="cuda")
        ops.histogram_models(idx, C, cnt, N=N, lut=lut, models=mdl)
        assert torch.equal(cnt, want_t), ("histogram_models + lut", dtype, key, content)
        assert torch.equal(mdl, want_m), ("models", dtype, key, content)


@pytest.mark.parametrize("key,content", CASES)
def test_one_workgroup_per_row(ops, key, content):
    """L C = 2048: the plain histogram (assign 0) and the fused form (assign 2, with and without models), both counter widths."""
    check_all_modes(ops, 2, 1024, key, content, fused=True)


@pytest.mark.parametrize("key,content", CASES)
def test_several_workgroups_per_row(ops, key, content):
    """L = 2, C = 3: the plain histogram with its workgroups side by side on a row, both counter widths."""
    check_all_modes(ops, 2, 3, key, content, fused=False)
