"""The launch rules of the older kernels stated a second time, as pure functions of the shape and the CU count: which kernel a
call takes, how many workgroups it gets and how each workgroup walks its share.  tests/test_gpu_large_paths.py picks its shapes
with them and asserts, before every launch, that the shape reaches the path the test is named after;
tests/test_launch_plans_host.py reads the constants below out of the .hip sources, so that retuning one of them says which
shapes have to move.

    lookup_plan     lookup_lds_passes / k_lookup_lds                    vbq_amd/csrc/vbq_latents.hip
    rank_plan       vbq_analogy_ranks_f32 / k_rank_gemm                 vbq_amd/csrc/vbq_ranks.hip
    *_grid          vbq_moments_f32, vbq_rd_sums_u16, vbq_index_max_u16, vbq_check_inputs_f32
                                                                        vbq_amd/csrc/vbq_reduce.hip
                    launch_hist (k_hist_tiled)                          vbq_amd/csrc/vbq_hist.hip
    solve_kernel    launch_quantize: which solve kernel a lambda chunk takes     vbq_amd/csrc/vbq_quantize.hip, vbq_quantize_fast.hip
    notebook_kernel launch_notebook: which notebook kernel a beta chunk takes   vbq_amd/csrc/vbq_notebook.hip
    transpose_kernel, gather_kernel, np_sums_first_kernel               vbq_amd/csrc/vbq_transpose.hip, vbq_latents.hip, vbq_reduce.hip

and, for tests/test_gpu_wide_rows.py, the rules by which the kernels that size their dynamic LDS from their arguments accept a
shape, lay the LDS out and refuse one step further:

    record_words    record_check_words                                  vbq_amd/csrc/vbq_records_common.h
    bag_plan        vbq_bag_f32 / vbq_records_bag_f32 (k_bag)           vbq_amd/csrc/vbq_bag.hip
    scores_plan     scores_plan (k_scores)                              vbq_amd/ext/vbqx_scores.hip
    topk_plan       topk_plan (k_topk)                                  vbq_amd/csrc/vbq_topk.hip
    budget_plan     budget_plan / sweep_plan (k_budget_dp, k_budget_sweep)     vbq_amd/csrc/vbq_budget.hip, vbq_amd/budget/vbqb_sweep.hip
    widest          the last shape a rule accepts, by bisection
"""
from collections import namedtuple

# ---- vbq_latents.hip
LDS_MIN_LOOKUPS_Z = 9 << 14      # kLdsMinLookupsZ: lambdas x rows from which Z_hat comes out of the LDS
LDS_MIN_LOOKUPS_NB = 3 << 10     # kLdsMinLookupsNb: rows from which num_bits comes out of the LDS
LDS_ROWS = 256                   # kLdsRows: rows per block
LDS_AHEAD = 2                    # VBQ_LDS_AHEAD: blocks per iteration of the pipelined loop
LDS_CH = 16                      # kLdsCh: channel tables per workgroup
LDS_MAX_N = 10                   # `if constexpr (N > 10)`: larger tables do not fit
LDS_RENUMBER = 16                # `(gridDim.x & 15) == 0`: channel groups are renumbered in blocks of 16
# ---- vbq_ranks.hip
RANK_BM = 128                    # kBM: questions per tile
RANK_BN = 128                    # kBN: words per tile
RANK_BK = 32                     # VBQ_RANK_BK: k per LDS stage
RANK_WGS = 2                     # VBQ_RANK_WGS: workgroups per CU
RANK_MAX_SPLITS = 256            # `s <= 256` of the best_s loop
# ---- vbq_reduce.hip
MOMENTS_FLAT_WGS = 2048          # cap = 2048 / n_ch + 1 workgroups per channel
MOMENTS_FLAT_LOADS = 4           # 16-byte loads in flight per lane in the main loop
MOMENTS_BC_WGS = 2048            # `if (gx > 2048) gx = 2048`
MOMENTS_BC_PER_THREAD = 16       # gx = ceil(E / (256 * 16))
MOMENTS_MAX_CH = 4096            # n_ch <= 4096
SCAN_WGS = 4096                  # `if (gx > 4096) gx = 4096` of index_max and check_inputs
RD_WGS_PER_CU = 8                # cap = num_cus() * 8 / chunks + 1
RD_CHUNK = 8                     # kRdChunk: lambdas per workgroup
# ---- vbq_hist.hip
HIST_TILED_WGS = 512             # gx = 512 / (groups * L) + 1
HIST_TILED_ROWS = 64             # rows per pass of a k_hist_tiled workgroup (1024 threads / 16 channels)
HIST_TILE_CH = 16                # kTileChannels
THREADS = 256                    # workgroup size of the reductions and scans
# ---- vbq_common.h, vbq_quantize.hip, vbq_quantize_fast.hip: the solve
SOLVE_DEPTHS = (12, 11, 10, 9, 8, 7, 6, 5, 4)      # VBQ_FOR_EACH_N: the bit depths the solve kernels are built for
MAX_LAMBDA_CHUNK = 32            # kMaxLambdaChunk: lambdas per launch
PRUNED_MAX_L = 2                 # kPrunedMaxL: lambdas up to which the pruned descent K1p takes an indices-only call
PRUNED_BUILT_L = (1, 2)          # VBQ_PRUNED_CASE: the K1p instances that are compiled, all of them reached
HULL_IDX_MIN_L = 16              # `if (L < 16) return 1;` of launch_quant_hull_idx10: K1e from this many lambdas
FAST_LAMBDA_RANGE = (1.9e-12, 1.8e19)              # fast_ok: every lambda of the chunk inside, as doubles
SWEEP_KEY_SHIFT = 16             # build_sweep_table<16>: a bucket is one value of (f32 bits >> 16)
SWEEP_KEYS = 2048                # kHullKeys: buckets, 16 octaves of 128
TILED_MAX_N = 10                 # `else if constexpr (N > 10)`: channel-last with n_ch > 1 is refused above
# ---- vbq_notebook.hip, vbq_sweep_host.h: the notebook solve
NB_MAX_BETA_CHUNK = 64           # kMaxBetaChunk: betas per launch
NB_PRUNED_MAX_L = 2              # `nonneg && Lc <= 2`: the pruned descent
NB_HULL_MIN_L = 6                # `fast_ok && N == 10 && Lc >= 6`: K1nt from this many betas
NB_FAST_RANGE = (1e-12, 1e18)    # fast_ok: every beta of the chunk inside, as doubles
NB_SWEEP_RANGE = (2e-12, 2e18)   # build_sweep_table<kNbKeyShift>(b, Lc, 2e-12f, 2e18f, sw) on b = (float)(2 beta)
NB_KEY_SHIFT = 17                # kNbKeyShift
NB_KEYS = 1536                   # kNbKeys: 24 octaves of 64 buckets
# ---- vbq_reduce.hip: the NumPy-order sums
NP_BLOCK = 8192                  # kNpBlock: elements per k_np_block_sums workgroup
# ---- every launcher below: `lds > 64 * 1024` raises hipFuncAttributeMaxDynamicSharedMemorySize before the launch
LDS_OPT_IN = 64 * 1024
WAVE = 64                        # kWave (vbq_common.h)
# ---- vbq_records_common.h
RECORDS_MAX_N = 10               # kRecordsMaxN
RECORDS_MAX_WORDS = 8192         # kRecordsMaxWords: 32-bit words of one record
# ---- vbq_bag.hip
BAG_WG_PER_CU = 16               # kBagWgPerCu: single-wave workgroups per CU the grid is sized for
BAG_LDS_TABLE_REUSE = 4          # kBagLdsTableReuse: coordinates decoded per table entry loaded, from which the code book is staged
BAG_LDS_LIMIT = 160 * 1024       # kBagLdsLimit
BAG_ALWAYS_K = 16804             # kBagAlwaysK: every K up to here fits whatever N, total_bits and n_tables
# ---- vbqx_scores.hip
SCORES_MAX_GROUP = 64            # kScoresMaxGroup = kWave: pairs per wave, halved down to kScoresMinGroup
SCORES_MIN_GROUP = 8             # kScoresMinGroup (VBQX_SCORES_MIN_GROUP)
SCORES_LDS_TARGET = 8 * 1024     # kScoresLdsTarget (VBQX_SCORES_LDS_TARGET): what a group above the smallest may take
SCORES_LDS_LIMIT = 160 * 1024    # kScoresLdsLimit: what the smallest group may take
SCORES_ALWAYS_K = 3500           # kScoresAlwaysK
# ---- vbq_topk.hip
TOPK_Q = 32                      # kTopkQ: queries per workgroup
TOPK_MAX_E = 8                   # kTopkMaxE: exclusions per query
TOPK_MIN_ROWS, TOPK_MAX_ROWS = 32, 128       # kTopkMinRows, kTopkMaxRows: rows per tile, halved from the largest
TOPK_LDS_TWO_PER_CU = 80 * 1024  # kTopkLdsTwoPerCu: the plan first looks for a tile that leaves room for two workgroups per CU
TOPK_LDS_LIMIT = 160 * 1024      # kTopkLdsLimit
TOPK_ALWAYS_K = 512              # kTopkAlwaysK
# ---- vbq_budget.hip, vbqb_sweep.hip
BUDGET_LDS_BYTES = 160 * 1024    # kBudgetLdsBytes and kSweepLdsBytes
BUDGET_MAX_N = 52                # kBudgetMaxN and kSweepMaxN


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------- lookups
Walk = namedtuple("Walk", "pipelined rest last_rows")
"""How one workgroup walks `rows` rows of one lambda: iterations of the pipelined loop (LDS_AHEAD whole blocks each, FULL),
blocks of the ragged-rest loop, rows of the last of them (LDS_ROWS when it is whole)."""

LookupPlan = namedtuple("LookupPlan", "eligible z_lds nb_lds groups renumbered last_group_channels splits per last_split_rows")


def walk(rows, whole_group=True):
    it = rows // (LDS_AHEAD * LDS_ROWS) if whole_group else 0
    left = rows - it * LDS_AHEAD * LDS_ROWS
    rest = cdiv(left, LDS_ROWS)
    last = left - (rest - 1) * LDS_ROWS if rest else 0
    return Walk(it, rest, last)


def lookup_plan(L, C, B, N, cus, want_zhat=True, want_num_bits=True):
    """lookup_lds_passes: which of Z_hat / num_bits leave the generic kernel, and the grid of the sorted-table pass (channel
    groups x row splits of `per` rows, the last one shorter).  The num_bits pass is groups x L workgroups of all B rows."""
    groups = cdiv(C, LDS_CH)
    eligible = N <= LDS_MAX_N and B % 4 == 0 and C % 4 == 0
    z = eligible and want_zhat and L * B >= LDS_MIN_LOOKUPS_Z
    nb = eligible and want_num_bits and B >= LDS_MIN_LOOKUPS_NB
    blocks = cdiv(B, LDS_ROWS)
    splits = max(1, min(cdiv(2 * cus, groups), blocks))
    per = cdiv(blocks, splits) * LDS_ROWS
    splits = cdiv(B, per)
    return LookupPlan(eligible, z, nb, groups, groups % LDS_RENUMBER == 0, C - (groups - 1) * LDS_CH, splits, per,
                      B - (splits - 1) * per)


def renumbered(grp, groups):
    """The channel group workgroup `grp` of `groups` serves (k_lookup_lds, the XCD renumbering)."""
    if groups % LDS_RENUMBER:
        return grp
    return (grp & ~15) + ((grp & 7) << 1) + ((grp >> 3) & 1)


def find_lookup_shape(cus, C, N, blocks_per_split, last_rows, prefer=None, max_elements=44_000_000):
    """(L, B) at which the sorted-table pass gives every split `blocks_per_split` blocks and the last split `last_rows` rows
    (None: any), with Z_hat out of the LDS: B = `prefer` when it qualifies, else the smallest such multiple of 4, and L the
    fewest lambdas (two at least: the tables stay for the second) that take Z_hat to the LDS.  None if there is none."""
    def lambdas(B):
        return max(2, cdiv(LDS_MIN_LOOKUPS_Z, B))

    def ok(B):
        p = lookup_plan(lambdas(B), C, B, N, cus)
        return (p.z_lds and p.per == blocks_per_split * LDS_ROWS and last_rows in (None, p.last_split_rows) and p.splits >= 2
                and lambdas(B) * B * C <= max_elements)
    if prefer is not None and ok(prefer):
        return lambdas(prefer), prefer
    per = blocks_per_split * LDS_ROWS
    for k in range(1, 4 * cus * blocks_per_split + 2):
        B = k * LDS_ROWS + 4 if last_rows is None else k * per + last_rows
        if B % 4 == 0 and ok(B):
            return lambdas(B), B
    return None


# ---------------------------------------------------------------------------------------------------------------- rank GEMM
RankPlan = namedtuple("RankPlan", "qb nt best_s tiles_per_wg splits last_wg_tiles nk k2 kend_last")


def rank_plan(V, K, Q, cus):
    """vbq_analogy_ranks_f32: question blocks x word-tile ranges, and the k-chunks of a tile (nk stages, the last one multiplied
    up to kend_last)."""
    qb, nt = cdiv(Q, RANK_BM), cdiv(V, RANK_BN)
    slots = cus * RANK_WGS
    best_s, best_cost = 1, -1
    for s in range(1, min(nt, RANK_MAX_SPLITS) + 1):
        tpw = cdiv(nt, s)
        cost = cdiv(qb * s, slots) * tpw
        if best_cost < 0 or cost < best_cost or (cost == best_cost and tpw >= 8 and s > best_s):
            best_cost, best_s = cost, s
    tpw = cdiv(nt, best_s)
    splits = cdiv(nt, tpw)
    nk = cdiv(K, RANK_BK)
    k2 = (K + 1) & ~1
    return RankPlan(qb, nt, best_s, tpw, splits, nt - (splits - 1) * tpw, nk, k2, k2 - (nk - 1) * RANK_BK)


def find_rank_words(cus, Q, K, min_tiles_per_wg, shorter_last, prefer=None, max_work=1_000_000_000, partial=37):
    """V (its last tile holding `partial` words) at which a workgroup gets at least `min_tiles_per_wg` tiles, the last workgroup
    fewer when `shorter_last`; `prefer` when it qualifies, else the smallest such V with V * Q * K <= max_work.  None if none."""
    def ok(V):
        p = rank_plan(V, K, Q, cus)
        return (p.tiles_per_wg >= min_tiles_per_wg and p.splits >= 2 and V % RANK_BN != 0 and V * Q * K <= max_work
                and (not shorter_last or p.last_wg_tiles < p.tiles_per_wg))
    if prefer is not None and ok(prefer):
        return prefer
    for nt in range(2, max_work // (Q * K * RANK_BN) + 2):
        V = (nt - 1) * RANK_BN + partial
        if ok(V):
            return V
    return None


# ---------------------------------------------------------------------------------------------------------------- grid caps
def moments_flat_grid(n_per_ch, n_ch):
    """vbq_moments_f32, C = 1 or channel-major -> (workgroups per channel, float4 per channel that the main loop needs
    more than: with fewer no lane enters it)."""
    gx = max(1, min(cdiv(n_per_ch // 4, THREADS), MOMENTS_FLAT_WGS // n_ch + 1))
    return gx, (MOMENTS_FLAT_LOADS - 1) * gx * THREADS


def moments_bc_grid(rows, n_ch):
    """vbq_moments_f32, channel-last -> (workgroups, the element stride of a lane)."""
    gx = max(min(cdiv(rows * n_ch, THREADS * MOMENTS_BC_PER_THREAD), MOMENTS_BC_WGS), cdiv(n_ch, THREADS))
    return gx, (gx * THREADS // n_ch) * n_ch


def rd_sums_grid(E, L, cus):
    """vbq_rd_sums_u16 -> (workgroups per chunk of lambdas, chunks, grid passes over the E elements)."""
    chunks = cdiv(L, RD_CHUNK)
    gx = min(cdiv(E, THREADS), cus * RD_WGS_PER_CU // chunks + 1)
    return gx, chunks, cdiv(E, gx * THREADS)


def scan_grid(n):
    """vbq_index_max_u16 / vbq_check_inputs_f32 -> (workgroups, grid passes)."""
    gx = min(cdiv(n, THREADS), SCAN_WGS)
    return gx, cdiv(n, gx * THREADS)


def hist_tiled_grid(rows, n_ch, L):
    """launch_hist, channel-last with C > 1 -> (workgroups per channel group and lambda, channel groups, row passes of the
    busiest workgroup)."""
    groups = cdiv(n_ch, HIST_TILE_CH)
    iters = cdiv(rows, HIST_TILED_ROWS)
    gx = max(1, min(HIST_TILED_WGS // (groups * L) + 1, iters))
    return gx, groups, cdiv(iters, gx)


# ---------------------------------------------------------------------------------------------------------------- the solve
def sweep_eligible(lam):
    """build_sweep_table<16> on the chunk's lambdas as f32 (the threshold kernels K1t and K1e): at most 32 values inside the fast
    range, no two in one bucket of 7 mantissa bits (equal ones among them), no more octaves than there are buckets."""
    import struct
    if not 1 <= len(lam) <= MAX_LAMBDA_CHUNK:
        return False
    v = sorted(struct.unpack("f", struct.pack("f", x))[0] for x in lam)
    lo, hi = (struct.unpack("f", struct.pack("f", x))[0] for x in FAST_LAMBDA_RANGE)
    if not all(lo <= x <= hi for x in v):
        return False
    keys = [struct.unpack("I", struct.pack("f", x))[0] >> SWEEP_KEY_SHIFT for x in v]
    if any(b <= a for a, b in zip(keys, keys[1:])):
        return False
    return keys[-1] - keys[0] + 2 <= SWEEP_KEYS


def solve_kernel(N, lam, layout, n_ch, mode="f32", level_len=False, want_idx=True, want_zhat=False, want_bits=False,
                 counting=False, workgroups_per_cu=0, elements=0):
    """launch_quantize for ONE chunk of lambdas (`lam`, at most 32 doubles) -> the kernel it launches:
        "tiled"     k_quant_tiled         channel-last input with n_ch > 1 (the literal scan)
        "flat"      k_quant_flat          planes / one code book, the literal scan
        "K1t"       k_level_counts_hull   counting, raw lengths, N = 10, an eligible sweep
        "K1e"       k_quant_hull_idx      indices only, raw lengths, N = 10, 16 or more lambdas, an eligible sweep
        "K1p<LL>"   k_quant_pruned        indices only, LL <= kPrunedMaxL lambdas, workgroups_per_cu == 0; any lambda
        "K1<MODE>"  k_quant_fast          MODE 0 indices, 1 with Z_hat / lengths, 2 counting; every lambda in the fast range
        "refused"   VBQ_ERR_UNSUPPORTED
    layout: "bc", "cb" or "bc->cb"; level_len: a caller length table is given; elements: rows x n_ch (K1e's 4 GB plane limit).
    counting: vbq_level_counts_f32 (no per-element output, f32 mode)."""
    assert N in SOLVE_DEPTHS and 1 <= len(lam) <= MAX_LAMBDA_CHUNK and layout in ("bc", "cb", "bc->cb") and mode in ("f32", "f64")
    L = len(lam)
    if counting:
        want_idx = want_zhat = want_bits = False
        if n_ch > 1 and layout == "bc":
            return "refused"
    if mode == "f64" and level_len:
        return "refused"
    bc_to_cb = layout == "bc->cb" and n_ch > 1
    flat = n_ch == 1 or layout == "cb" or bc_to_cb
    if not flat:
        return "refused" if N > TILED_MAX_N else "tiled"
    f32 = mode == "f32"
    fast_ok = f32 and all(FAST_LAMBDA_RANGE[0] <= x <= FAST_LAMBDA_RANGE[1] for x in lam)
    idx_only = not counting and want_idx and not want_zhat and not want_bits
    if f32 and N == 10 and fast_ok and not level_len:
        if counting and sweep_eligible(lam):
            return "K1t"
        if idx_only and L >= HULL_IDX_MIN_L and 2 * elements <= 0xffffffff and sweep_eligible(lam):
            return "K1e"
    if f32 and idx_only and workgroups_per_cu == 0 and L <= PRUNED_MAX_L:
        return f"K1p<{L}>"
    if fast_ok:
        return "K1<2>" if counting else ("K1<1>" if want_zhat or want_bits else "K1<0>")
    if counting or bc_to_cb:
        return "refused"
    return "flat"


def solve_kernels(N, lam, layout, n_ch, **kw):
    """solve_kernel for every chunk of a sweep of any length (the l0 loop of launch_quantize); a per-lambda flag list
    level_len is not needed: the table is given for all chunks or for none."""
    return [solve_kernel(N, list(lam[l0:l0 + MAX_LAMBDA_CHUNK]), layout, n_ch, **kw) for l0 in range(0, len(lam), MAX_LAMBDA_CHUNK)]


# ---------------------------------------------------------------------------------------------------------------- other routes
def _f32(x):
    import struct
    return struct.unpack("f", struct.pack("f", x))[0]


def sweep_table_ok(values, max_l, shift, keys, lo, hi):
    """build_sweep_table<shift> (vbq_sweep_host.h) on f32 `values`: between 1 and max_l of them, each inside [lo, hi] (as f32),
    no two in one bucket of key = bits >> shift (equal ones among them), last key - first key + 2 <= keys."""
    import struct
    if not 1 <= len(values) <= max_l:
        return False
    v = sorted(_f32(x) for x in values)
    if not all(_f32(lo) <= x <= _f32(hi) for x in v):
        return False
    k = [struct.unpack("I", struct.pack("f", x))[0] >> shift for x in v]
    return all(b > a for a, b in zip(k, k[1:])) and k[-1] - k[0] + 2 <= keys


def notebook_kernel(N, betas):
    """launch_notebook for ONE chunk of betas (at most 64 doubles) -> the kernel it launches:
        "pruned<L>"  k_quant_notebook_pruned   one or two betas, none negative
        "hull"       k_quant_notebook_hull     N = 10, six or more betas in the fast range whose sweep table can be built
        "fast"       k_quant_notebook_fast     every beta in the fast range
        "literal"    k_quant_notebook          the rest: a negative beta, a beta outside the fast range"""
    L = len(betas)
    assert 1 <= L <= NB_MAX_BETA_CHUNK
    if all(b >= 0.0 for b in betas) and L <= NB_PRUNED_MAX_L:
        return f"pruned<{L}>"
    fast_ok = all(NB_FAST_RANGE[0] <= b <= NB_FAST_RANGE[1] for b in betas)
    if fast_ok and N == 10 and L >= NB_HULL_MIN_L and \
            sweep_table_ok([_f32(2.0 * b) for b in betas], NB_MAX_BETA_CHUNK, NB_KEY_SHIFT, NB_KEYS, *NB_SWEEP_RANGE):
        return "hull"
    return "fast" if fast_ok else "literal"


def transpose_kernel(rows, cols, elem_bytes, aligned=True):
    """launch_transpose_batched / vbq_transpose_f32 -> "vec" (k_transpose_batched_vec: rows and cols multiples of the 16-byte
    vector, 16-byte aligned bases; a whole number of vectors per plane follows) or "scalar" (k_transpose_batched)."""
    V = 16 // elem_bytes
    return "vec" if rows % V == 0 and cols % V == 0 and aligned else "scalar"


def gather_kernel(n_ch, layout, out_layout):
    """vbq_gather_f32 -> "k_gather_transpose" where the output's layout differs from the input's (C > 1), else "k_gather"."""
    return "k_gather_transpose" if n_ch > 1 and layout != out_layout else "k_gather"


def np_sums_first_kernel(n):
    """launch_np_sums: the first launch of vbq_numpy_sum_sq_f32 / vbq_numpy_row_sums_f32 on rows of n elements."""
    return "k_np_block_sums" if n // NP_BLOCK > 0 else "k_np_finish"


# ---------------------------------------------------------------------------------------------------------------- wide rows
def widest(pred, lo, hi):
    """The largest x in [lo, hi] with pred(x), for a pred that holds up to some x and fails from there on; pred(lo) must hold."""
    assert pred(lo), lo
    if pred(hi):
        return hi
    while hi - lo > 1:                                       # pred(lo) and not pred(hi)
        mid = (lo + hi) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return lo


def length_field_bits(N):
    """length_field_bits of vbq_records_common.h: N.bit_length() for N <= 15."""
    return 4 if N >= 8 else (3 if N >= 4 else (2 if N >= 2 else 1))


def table_size(N):
    return (2 << N) - 1


def record_words(K, N, total_bits):
    """record_words: K length fields, total_bits of codes, zero padding up to whole 32-bit words."""
    return (K * length_field_bits(N) + total_bits + 31) // 32


def record_fits(K, N, total_bits):
    """record_check_total_bits and record_check_words: what every entry point that takes records asks first."""
    return 1 <= N <= RECORDS_MAX_N and 0 <= total_bits <= K * N and record_words(K, N, total_bits) <= RECORDS_MAX_WORDS


BagPlan = namedtuple("BagPlan", "lds_bytes table_in_lds")


def bag_lds_bytes(K, n_words, table_entries):
    """bag_lds_bytes: the staged record, the accumulators twice, the one code book."""
    return 4 * (n_words + 2 * K + table_entries)


def bag_plan(K, N, total_bits, n_tables, n_ids, n_bags, cus, records):
    """vbq_records_bag_f32 (records) / vbq_bag_f32 for n_bags >= 1 bags -> BagPlan, or None where the call is refused."""
    if records and not record_fits(K, N, total_bits):
        return None
    n_words = record_words(K, N, total_bits) if records else 0
    if bag_lds_bytes(K, n_words, 0) > BAG_LDS_LIMIT:                       # bag_check_lds
        return None
    if not records:
        return BagPlan(bag_lds_bytes(K, 0, 0), False)
    grid = min(n_bags, cus * BAG_WG_PER_CU)                                # bag_grid
    per_wg = cdiv(n_ids, grid)
    T = table_size(N)
    in_lds = n_tables == 1 and per_wg * K >= BAG_LDS_TABLE_REUSE * T and bag_lds_bytes(K, n_words, T) <= BAG_LDS_LIMIT
    return BagPlan(bag_lds_bytes(K, n_words, T if in_lds else 0), in_lds)


ScoresPlan = namedtuple("ScoresPlan", "G RS lds_bytes")


def scores_lds_bytes(G, RS, n_words):
    """scores_lds_bytes: the ids of the group, the tile [G][RS], the staged records [G][n_words]."""
    return 8 * WAVE + 4 * (G * RS + G * n_words)


def scores_plan(K, N, total_bits, records):
    """scores_plan: the largest group within the target, else the smallest if it fits at all -> ScoresPlan, or None."""
    if records and not record_fits(K, N, total_bits):
        return None
    n_words = record_words(K, N, total_bits) if records else 0
    RS = K | 1
    G = SCORES_MAX_GROUP
    while G >= SCORES_MIN_GROUP:
        lds = scores_lds_bytes(G, RS, n_words)
        if lds <= (SCORES_LDS_TARGET if G > SCORES_MIN_GROUP else SCORES_LDS_LIMIT):
            return ScoresPlan(G, RS, lds)
        G >>= 1
    return None


TopkPlan = namedtuple("TopkPlan", "K2 R table_in_lds lds_bytes per_cu")


def topk_lds_bytes(K2, R, n_words, table_entries):
    """topk_lds_bytes: queries [K2][32], B tile [max(K2, 32)][R + 1], thresholds, exclusions, two flags (four words), the staged
    records, the one code book."""
    return 4 * (K2 * TOPK_Q + max(K2, TOPK_Q) * (R + 1) + TOPK_Q + TOPK_Q * TOPK_MAX_E + 4 + R * n_words + table_entries)


def topk_plan(K, N, total_bits, n_tables, records):
    """topk_plan: the largest tile that leaves room for two workgroups per CU, else the largest that fits at all; at each tile
    the one code book in LDS is tried before the code book through L2 -> TopkPlan, or None."""
    if records and not record_fits(K, N, total_bits):
        return None
    n_words = record_words(K, N, total_bits) if records else 0
    entries = table_size(N) if records and n_tables == 1 else 0
    K2 = (K + 1) & ~1
    for limit in (TOPK_LDS_TWO_PER_CU, TOPK_LDS_LIMIT):
        R = TOPK_MAX_ROWS
        while R >= TOPK_MIN_ROWS:
            for in_lds in ((True, False) if entries else (False,)):
                lds = topk_lds_bytes(K2, R, n_words, entries if in_lds else 0)
                if lds <= limit:
                    return TopkPlan(K2, R, in_lds, lds, 2 if lds <= TOPK_LDS_TWO_PER_CU else 1)      # topk_launch: the grid's cap
            R >>= 1
    return None


BudgetPlan = namedtuple("BudgetPlan", "threads lds_bytes bp_in_lds")


def budget_plan(K, N, width):
    """budget_plan of vbq_budget.hip (width = budget + 1) and sweep_plan of vbqb_sweep.hip with budgets to walk (a curve-only
    pass keeps no back-pointers and takes the value rows alone) -> BudgetPlan, or None when the two value rows do not fit."""
    threads = 64 if width <= 64 else (128 if width <= 128 else 256)
    values = (2 * width + 2 * (N + 1)) * 8 + 16
    if values > BUDGET_LDS_BYTES:
        return None
    bp_row = (K * width + 15) & ~15
    in_lds = values + bp_row <= BUDGET_LDS_BYTES
    return BudgetPlan(threads, values + (bp_row if in_lds else 0), in_lds)


def budget_bp_row_bytes(K, width):
    """bp_row_bytes: one row's back-pointers, the size of a workspace slice."""
    return (K * width + 15) & ~15
