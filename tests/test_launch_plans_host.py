"""tests/launch_plans.py against the sources it restates, without a GPU: every constant a plan depends on is read out of the
.hip files with a regular expression and compared with the Python copy, and the plan functions are checked on numbers worked
out by hand for 256 CUs -- the shapes tests/test_gpu_large_paths.py derives on an MI355X, and the widest rows
tests/test_gpu_wide_rows.py derives from the LDS rules.  A failure here after a retuning means: move the shapes of those modules
so that they still reach the paths they are named after."""
import os
import re

import pytest

import launch_plans as LP

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vbq_amd", "csrc")
PKG = os.path.dirname(CSRC)
CUS = 256


def _src(name):
    """A file of vbq_amd/csrc, or -- with a directory in the name -- of vbq_amd."""
    with open(os.path.join(PKG if "/" in name else CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, f"{what}: expected one match of {pattern!r}, found {len(found)} -- the source moved, restate it"
    return found[0]


def _int(expr):
    """'9 << 14', '160 * 1024' or '256' -> int."""
    m = re.fullmatch(r"\s*(\d+)\s*(?:(<<|\*)\s*(\d+))?\s*", expr)
    assert m, expr
    a, b = int(m.group(1)), int(m.group(3) or 0)
    return a * b if m.group(2) == "*" else a << b


def test_lookup_constants_match_the_source():
    s = _src("vbq_latents.hip")
    assert _int(_one(r"constexpr int64_t kLdsMinLookupsZ = ([^;]+);", s, "kLdsMinLookupsZ")) == LP.LDS_MIN_LOOKUPS_Z
    assert _int(_one(r"constexpr int64_t kLdsMinLookupsNb = ([^;]+);", s, "kLdsMinLookupsNb")) == LP.LDS_MIN_LOOKUPS_NB
    assert int(_one(r"#define VBQ_LDS_AHEAD (\d+)", s, "VBQ_LDS_AHEAD")) == LP.LDS_AHEAD
    ch, rows = _one(r"constexpr int kLdsCh = (\d+), kLdsRows = (\d+), kLdsPitch = kLdsRows, kLdsAhead = VBQ_LDS_AHEAD;", s, "kLdsCh")
    assert (int(ch), int(rows)) == (LP.LDS_CH, LP.LDS_ROWS)
    # the rule itself: the lines the plan restates are still there
    _one(r"if \(\(gridDim\.x & 15\) == 0\) grp = \(grp & ~15\) \+ \(\(grp & 7\) << 1\) \+ \(\(grp >> 3\) & 1\);", s, "renumbering")
    assert _one(r"if constexpr \(N > (\d+)\) \{\s*return VBQ_OK;", s, "largest N") == str(LP.LDS_MAX_N)
    _one(r"if \(B % 4 != 0 \|\| C % 4 != 0 \|\|", s, "preconditions")
    _one(r"\(int64_t\)L \* B >= kLdsMinLookupsZ;", s, "want_z")
    _one(r"&& B >= kLdsMinLookupsNb;", s, "want_nb")
    _one(r"int64_t splits = \(2 \* \(int64_t\)num_cus\(\) \+ groups - 1\) / groups;", s, "splits")
    _one(r"const int64_t per = \(\(blocks \+ splits - 1\) / splits\) \* kLdsRows;\s*splits = \(B \+ per - 1\) / per;", s, "per")
    _one(r"for \(; r0 \+ \(long\)kLdsAhead \* kLdsRows <= r_end; r0 \+= \(long\)kLdsAhead \* kLdsRows\)", s, "pipelined loop")


def test_rank_constants_match_the_source():
    s = _src("vbq_ranks.hip")
    assert int(_one(r"constexpr int kBM = (\d+);", s, "kBM")) == LP.RANK_BM
    assert int(_one(r"constexpr int kBN = (\d+);", s, "kBN")) == LP.RANK_BN
    assert int(_one(r"#define VBQ_RANK_BK (\d+)", s, "VBQ_RANK_BK")) == LP.RANK_BK
    assert int(_one(r"#define VBQ_RANK_WGS (\d+)", s, "VBQ_RANK_WGS")) == LP.RANK_WGS
    assert int(_one(r"for \(long s = 1; s <= nt && s <= (\d+); \+\+s\)", s, "best_s loop")) == LP.RANK_MAX_SPLITS
    _one(r"const long slots = \(long\)num_cus\(\) \* VBQ_RANK_WGS;", s, "slots")
    _one(r"const long cost = \(\(qb \* s \+ slots - 1\) / slots\) \* tpw;", s, "cost")
    _one(r"\(cost == best_cost && tpw >= 8 && s > best_s\)", s, "tie rule")
    _one(r"const int kend = last_k \? K2 - kc \* kBK : kBK;", s, "kend")
    _one(r"\(int\)\(\(K \+ 1\) & ~1\), tiles_per_wg, below\);", s, "K2")


def test_reduction_caps_match_the_source():
    s = _src("vbq_reduce.hip")
    assert int(_one(r"const int64_t cap = (\d+) / n_ch \+ 1;", s, "moments cap")) == LP.MOMENTS_FLAT_WGS
    assert int(_one(r"for \(; q \+ (\d+) \* stride < nq; q \+= \d+ \* stride\)", s, "moments main loop")) == LP.MOMENTS_FLAT_LOADS - 1
    per, cap = _one(r"int64_t gx = \(E \+ 256 \* (\d+) - 1\) / \(256 \* \d+\);\s*if \(gx > (\d+)\) gx = \d+;", s, "moments_bc grid")
    assert (int(per), int(cap)) == (LP.MOMENTS_BC_PER_THREAD, LP.MOMENTS_BC_WGS)
    assert int(_one(r"n_ch >= 1 && n_ch <= (\d+), VBQ_ERR_INVALID_ARGUMENT,\s*\"vbq_moments_f32", s, "moments limit")) == LP.MOMENTS_MAX_CH
    for who in ("check_inputs", "index_max"):
        body = s[s.index(f'extern "C" int vbq_{who}_'):]
        body = body[:body.index("\n}\n")]                                      # that entry point alone
        assert int(_one(r"int64_t gx = \(n \+ 255\) / 256;\s*if \(gx > (\d+)\) gx = \d+;", body, who)) == LP.SCAN_WGS
    assert int(_one(r"const int64_t cap = \(int64_t\)num_cus\(\) \* (\d+) / chunks \+ 1;", s, "rd_sums cap")) == LP.RD_WGS_PER_CU
    assert int(_one(r"constexpr int kRdChunk = (\d+);", s, "kRdChunk")) == LP.RD_CHUNK
    s = _src("vbq_hist.hip")
    assert int(_one(r"int64_t gx = (\d+) / \(\(int64_t\)groups \* L\) \+ 1;", s, "hist_tiled grid")) == LP.HIST_TILED_WGS
    rows, stride = _one(r"for \(long r = \(long\)blockIdx\.x \* (\d+) \+ slot; r < n_rows; r \+= \(long\)gridDim\.x \* (\d+)\)", s, "hist_tiled rows")
    assert int(rows) == int(stride) == LP.HIST_TILED_ROWS
    assert int(_one(r"constexpr int kHistTiledThreads = (\d+);", s, "kHistTiledThreads")) == LP.HIST_TILED_ROWS * LP.HIST_TILE_CH
    assert int(_one(r"constexpr int kTileChannels = (\d+);", _src("vbq_common.h") + s, "kTileChannels")) == LP.HIST_TILE_CH


def test_solve_constants_match_the_source():
    c, q, f = _src("vbq_common.h"), _src("vbq_quantize.hip"), _src("vbq_quantize_fast.hip")
    depths = _one(r"#else\s*#define VBQ_FOR_EACH_N\(X\) ((?:X\(\d+\) ?)+)\s*#endif", c, "VBQ_FOR_EACH_N")
    assert tuple(int(v) for v in re.findall(r"X\((\d+)\)", depths)) == LP.SOLVE_DEPTHS
    assert int(_one(r"constexpr int kMaxLambdaChunk = (\d+);", c, "kMaxLambdaChunk")) == LP.MAX_LAMBDA_CHUNK
    assert int(_one(r"constexpr int kPrunedMaxL = (\d+);", f, "kPrunedMaxL")) == LP.PRUNED_MAX_L
    built = _one(r"switch \(L\) \{\s*((?:VBQ_PRUNED_CASE\(\d+\) ?)+)\s*default: return 1;", f, "VBQ_PRUNED_CASE")
    assert tuple(int(v) for v in re.findall(r"\((\d+)\)", built)) == LP.PRUNED_BUILT_L and LP.PRUNED_MAX_L <= max(LP.PRUNED_BUILT_L)
    assert int(_one(r"if \(L < (\d+)\) return 1; +// below that the thresholds cost more", f, "K1e's shortest sweep")) == LP.HULL_IDX_MIN_L
    lo, hi = _one(r"fast_ok = fast_ok && \(lc\.lam\[i\] >= ([0-9.e+-]+) && lc\.lam\[i\] <= ([0-9.e+-]+)\);", q, "fast_ok")
    assert (float(lo), float(hi)) == LP.FAST_LAMBDA_RANGE
    shift, lo, hi = _one(r"return build_sweep_table<(\d+)>\(v, L, ([0-9.e+-]+)f, ([0-9.e+-]+)f, sw\);", f, "build_lambda_sweep")
    assert int(shift) == LP.SWEEP_KEY_SHIFT and (float(lo), float(hi)) == LP.FAST_LAMBDA_RANGE
    assert int(_one(r"constexpr int kHullKeys = (\d+);", f, "kHullKeys")) == LP.SWEEP_KEYS
    assert int(_one(r"\} else if constexpr \(N > (\d+)\) \{\s*set_error\(\"vbq_quantize_f32: N=%d is built for channel-major", q,
                    "tiled limit")) == LP.TILED_MAX_N
    # the order of the dispatch and its conditions: the lines solve_kernel restates are still there, in this order
    marks = [r"const bool flat = \(n_ch == 1\) \|\| \(layout == VBQ_LAYOUT_CB\) \|\| bc_to_cb;",
             r"if constexpr \(sizeof\(PenT\) == 4 && N == 10\) \{\s*// first entropy-model pass[^\n]*\s*if \(fast_ok && lc_out && !len_c\) \{",
             r"if \(fast_ok && !lc_out && !len_c && oi && !oz && !ob\) \{\s*const int r = launch_quant_hull_idx10",
             r"if \(!lc_out && oi && !oz && !ob && wg_per_cu == 0\) \{\s*const int r = launch_quant_pruned<N>",
             r"if \(fast_ok\) \{\s*const int r = launch_quant_fast<N>",
             r"hipLaunchKernelGGL\(\(k_quant_flat<N, PenT>\)"]
    at = [re.search(m, q) for m in marks]
    assert all(at), [m for m, a in zip(marks, at) if not a]
    assert [a.start() for a in at] == sorted(a.start() for a in at)
    _one(r"if \(L < 1 \|\| L > kPrunedMaxL\) return 1;", f, "K1p's limit")
    _one(r"if \(2 \* \(uint64_t\)E > 0xffffffffull\) return 1;", f, "K1e's plane limit")
    _one(r"if \(level_counts\)\s*hipLaunchKernelGGL\(\(k_quant_fast<N, 2>\)", f, "K1 mode 2")
    _one(r"else if \(out_zhat \|\| out_bits\)\s*hipLaunchKernelGGL\(\(k_quant_fast<N, 1>\)", f, "K1 mode 1")


def test_solve_kernel_routes():
    """The routes the docstring of tests/test_gpu_literal_solve.py states, and the ones tests/test_gpu_fast_solve_variants.py
    is built on."""
    K = LP.solve_kernel
    lam6 = [0.0, 2.0 ** -8 * 2 ** 0.5, 0.1, 1.0, 37.0, 300.0]
    inside = [0.01, 0.1, 1.0, 4.0, 37.0]
    for N in LP.SOLVE_DEPTHS:
        # test_gpu_literal_solve.py: "k_quant_tiled<N, double / float>  layout bc, n_ch > 1.  N <= 10."
        for mode in ("f32", "f64"):
            assert K(N, lam6, "bc", 3, mode=mode, want_bits=True) == ("tiled" if N <= 10 else "refused")
            # "k_quant_flat<N, double>  mode f64, layout cb or n_ch == 1"; f32 with lambda = 0 and L >= 5 likewise
            assert K(N, lam6, "cb", 3, mode=mode, want_zhat=True, want_bits=True) == "flat"
            assert K(N, lam6, "bc", 1, mode=mode) == "flat" and K(N, lam6, "cb", 3, mode=mode) == "flat"
        assert K(N, inside, "cb", 3, mode="f64") == "flat"
        # "... and not the pruned descent: L >= 5, Z_hat / bits wanted, or workgroups_per_cu != 0"
        for L in (1, 2, 3, 4):
            out = [0.0, 1e25, 1e-13, 0.2][:L]
            assert K(N, out, "cb", 2, want_zhat=True) == "flat" and K(N, out, "cb", 2, want_bits=True) == "flat"
            assert K(N, out, "cb", 2, workgroups_per_cu=4) == "flat" and K(N, out, "bc", 1, workgroups_per_cu=4) == "flat"
            assert K(N, out, "cb", 2) == (f"K1p<{L}>" if L <= LP.PRUNED_MAX_L else "flat")
            assert K(N, out, "bc->cb", 2) == (f"K1p<{L}>" if L <= LP.PRUNED_MAX_L else "refused")
            ins = inside[:L]
            assert K(N, ins, "cb", 2) == K(N, ins, "bc", 1) == K(N, ins, "cb", 2, level_len=True) == (f"K1p<{L}>" if L <= 2 else "K1<0>")
            assert K(N, ins, "cb", 2, workgroups_per_cu=4) == "K1<0>"
            assert K(N, ins, "cb", 2, want_bits=True) == K(N, ins, "bc->cb", 2, want_zhat=True, level_len=True) == "K1<1>"
        # the fast kernels
        assert K(N, inside, "cb", 2) == K(N, inside, "bc->cb", 2) == K(N, inside, "bc", 1) == "K1<0>"
        assert K(N, inside, "bc->cb", 1) == "K1<0>"                      # one channel: the layout does not matter
        assert K(N, inside, "cb", 2, counting=True, level_len=True) == "K1<2>"
        assert K(N, inside, "cb", 2, counting=True) == ("K1t" if N == 10 else "K1<2>")
        assert K(N, inside, "bc", 2, counting=True) == "refused" and K(N, lam6, "cb", 2, counting=True) == "refused"
        assert K(N, lam6, "bc->cb", 2) == "refused" and K(N, inside, "cb", 2, mode="f64", level_len=True) == "refused"
        sweep32 = [2.0 ** (-8 + 0.5 * i) for i in range(32)]
        for L in (15, 16, 32):
            assert K(N, sweep32[:L], "cb", 2, elements=4002) == ("K1e" if N == 10 and L >= 16 else "K1<0>")
            assert K(N, sweep32[:L], "cb", 2, level_len=True) == "K1<0>" and K(N, sweep32[:L], "cb", 2, want_zhat=True) == "K1<1>"
        assert K(N, sweep32[:16], "cb", 2, elements=1 << 31) == "K1<0>"
        assert LP.solve_kernels(N, sweep32 + [1.0], "cb", 2) == ["K1e" if N == 10 else "K1<0>", "K1p<1>"]
        assert LP.solve_kernels(N, sweep32 + [1.0], "cb", 2, level_len=True) == ["K1<0>", "K1p<1>"]
        assert LP.solve_kernels(N, sweep32 + [1.0], "cb", 2, want_zhat=True) == ["K1<1>", "K1<1>"]
        # per chunk: the four lambdas after the first 32 hold no zero and go fast
        assert LP.solve_kernels(N, lam6 * 6, "cb", 2, want_bits=True) == ["flat", "K1<1>"]
        assert LP.solve_kernels(N, lam6 * 6 + [0.0], "cb", 2, want_bits=True) == ["flat", "flat"]
    # sweeps the threshold kernels hand on (test_threshold_kernel_on_ties_and_odd_sweeps): repeated values, one bucket, octaves
    assert LP.sweep_eligible([0.37]) and LP.sweep_eligible([2.0 ** k for k in range(-7, 9)])      # 15 octaves: 1922 buckets
    assert not LP.sweep_eligible([2.0 ** k for k in range(-7, 10)])                              # 16 octaves: 2050
    assert not LP.sweep_eligible([1.0, 1.0, 2.0]) and not LP.sweep_eligible([1.0, 1.0 + 2.0 ** -9, 4.0])
    assert not LP.sweep_eligible([1e-9, 1.0, 1e9]) and LP.sweep_eligible([1.0, 1.0 + 2.0 ** -7, 4.0])
    assert K(10, [1.0, 1.0, 2.0], "bc", 1, counting=True) == "K1<2>"
    # the eight-lambda sweeps of solve_cases cycled to 33: repeats, so N = 10 stays on K1 for raw lengths as well
    assert LP.solve_kernels(10, [1.0, 8.0] * 16 + [1.0], "cb", 2, elements=4002) == ["K1<0>", "K1p<1>"]


# ------------------------------------------------------------------------------------------------ the LDS-planned kernels
def test_record_constants_match_the_source():
    s = _src("vbq_records_common.h")
    assert int(_one(r"constexpr int kRecordsMaxN = (\d+);", s, "kRecordsMaxN")) == LP.RECORDS_MAX_N
    assert int(_one(r"constexpr int64_t kRecordsMaxWords = (\d+);", s, "kRecordsMaxWords")) == LP.RECORDS_MAX_WORDS
    _one(r"int length_field_bits\(int N\) \{ return N >= 8 \? 4 : \(N >= 4 \? 3 : \(N >= 2 \? 2 : 1\)\); \}", s, "length_field_bits")
    _one(r"return \(\(int64_t\)K \* length_field_bits\(N\) \+ total_bits \+ 31\) / 32;", s, "record_words")
    _one(r"VBQ_REQUIRE\(\*n_words <= kRecordsMaxWords, VBQ_ERR_UNSUPPORTED,", s, "record_check_words")
    c = _src("vbq_common.h")
    assert int(_one(r"constexpr int kWave = (\d+);", c, "kWave")) == LP.WAVE
    _one(r"constexpr int table_size\(int N\) \{ return \(2 << N\) - 1; \}", c, "table_size")
    assert [LP.length_field_bits(N) for N in range(1, 11)] == [N.bit_length() for N in range(1, 11)]
    # the LDS of the two record kernels: the image, and the one code book behind it
    r = _src("vbq_records.hip")
    _one(r"dim3\(kWave\), \(size_t\)n_words \* 4,\s*reinterpret_cast<hipStream_t>\(stream\), d_idx,", r, "the pack's LDS")
    _one(r"const size_t lds = \(size_t\)n_words \* 4 \+ \(lds_table \? \(size_t\)T \* 4 : 0\);", r, "the unpack's LDS")


def _opt_ins(s):
    """How often a launcher of the file raises the dynamic LDS limit, each behind the same threshold."""
    n = len(re.findall(r"hipFuncAttributeMaxDynamicSharedMemorySize", s))
    assert len(re.findall(r"lds(?:_bytes)? > (\d+) \* 1024 &&\s*hipFuncSetAttribute", s)) == n
    assert {int(v) * 1024 for v in re.findall(r"lds(?:_bytes)? > (\d+) \* 1024 &&\s*hipFuncSetAttribute", s)} == {LP.LDS_OPT_IN}
    return n


def test_bag_constants_match_the_source():
    s = _src("vbq_bag.hip")
    assert int(_one(r"constexpr int kBagWgPerCu = (\d+);", s, "kBagWgPerCu")) == LP.BAG_WG_PER_CU
    assert int(_one(r"constexpr int64_t kBagLdsTableReuse = (\d+);", s, "kBagLdsTableReuse")) == LP.BAG_LDS_TABLE_REUSE
    assert _int(_one(r"constexpr size_t kBagLdsLimit = ([^;]+);", s, "kBagLdsLimit")) == LP.BAG_LDS_LIMIT
    assert int(_one(r"constexpr int kBagAlwaysK = (\d+);", s, "kBagAlwaysK")) == LP.BAG_ALWAYS_K
    _one(r"return 4 \* \(\(size_t\)n_words \+ 2 \* \(size_t\)K \+ \(size_t\)table_entries\);", s, "bag_lds_bytes")
    _one(r"const size_t need = bag_lds_bytes\(K, n_words, 0\);\s*VBQ_REQUIRE\(need <= kBagLdsLimit, VBQ_ERR_UNSUPPORTED,", s, "bag_check_lds")
    _one(r"const int64_t resident = \(int64_t\)num_cus\(\) \* kBagWgPerCu;\s*return \(unsigned\)\(n_bags < resident \? n_bags : resident\);", s,
         "bag_grid")
    _one(r"const int64_t per_wg = \(n_ids \+ grid - 1\) / grid;", s, "per_wg")
    _one(r"const bool lds_table = n_tables == 1 && per_wg \* K >= kBagLdsTableReuse \* T && bag_lds_bytes\(K, n_words, T\) <= kBagLdsLimit;", s,
         "lds_table")
    _one(r"bag_launch<false, false>\(who, a, bag_grid\(n_bags\), bag_lds_bytes\(K, 0, 0\),", s, "the dense launch")
    assert _opt_ins(s) == 1                                  # bag_launch, a template: every instance


def test_scores_constants_match_the_source():
    s = _src("ext/vbqx_scores.hip")
    assert _int(_one(r"#define VBQX_SCORES_LDS_TARGET \(([^)]+)\)", s, "VBQX_SCORES_LDS_TARGET")) == LP.SCORES_LDS_TARGET
    assert int(_one(r"#define VBQX_SCORES_MIN_GROUP (\d+)", s, "VBQX_SCORES_MIN_GROUP")) == LP.SCORES_MIN_GROUP
    _one(r"constexpr int kScoresMaxGroup = kWave, kScoresMinGroup = VBQX_SCORES_MIN_GROUP;", s, "kScoresMaxGroup")
    assert LP.SCORES_MAX_GROUP == LP.WAVE
    assert _int(_one(r"constexpr size_t kScoresLdsLimit = ([^;]+);", s, "kScoresLdsLimit")) == LP.SCORES_LDS_LIMIT
    _one(r"constexpr size_t kScoresLdsTarget = VBQX_SCORES_LDS_TARGET;", s, "kScoresLdsTarget")
    assert int(_one(r"constexpr int kScoresAlwaysK = (\d+);", s, "kScoresAlwaysK")) == LP.SCORES_ALWAYS_K
    _one(r"return 8 \* \(size_t\)kWave \+ 4 \* \(\(size_t\)G \* RS \+ \(size_t\)G \* \(size_t\)n_words\);", s, "scores_lds_bytes")
    _one(r"a\.RS = a\.K \| 1;", s, "RS")
    _one(r"for \(int G = kScoresMaxGroup; G >= kScoresMinGroup && !a\.G; G >>= 1\) \{", s, "the group loop")
    _one(r"if \(\*lds <= \(G > kScoresMinGroup \? kScoresLdsTarget : kScoresLdsLimit\)\) a\.G = G;", s, "the group rule")
    assert _opt_ins(s) == 1                                  # scores_launch_as, a template: every instance


def test_topk_constants_match_the_source():
    s = _src("vbq_topk.hip")
    assert int(_one(r"constexpr int kTopkQ = (\d+);", s, "kTopkQ")) == LP.TOPK_Q
    assert int(_one(r"constexpr int kTopkMaxE = (\d+);", s, "kTopkMaxE")) == LP.TOPK_MAX_E
    lo, hi = _one(r"constexpr int kTopkMinRows = (\d+), kTopkMaxRows = (\d+);", s, "kTopkMinRows")
    assert (int(lo), int(hi)) == (LP.TOPK_MIN_ROWS, LP.TOPK_MAX_ROWS)
    assert _int(_one(r"constexpr size_t kTopkLdsLimit = ([^;]+);", s, "kTopkLdsLimit")) == LP.TOPK_LDS_LIMIT
    assert _int(_one(r"constexpr size_t kTopkLdsTwoPerCu = ([^;]+);", s, "kTopkLdsTwoPerCu")) == LP.TOPK_LDS_TWO_PER_CU
    assert int(_one(r"constexpr int kTopkAlwaysK = (\d+);", s, "kTopkAlwaysK")) == LP.TOPK_ALWAYS_K
    _one(r"const size_t bt = \(size_t\)\(K2 > kTopkQ \? K2 : kTopkQ\) \* \(R \+ 1\);\s*return 4 \* \(\(size_t\)K2 \* kTopkQ \+ bt \+ kTopkQ \+ "
         r"kTopkQ \* kTopkMaxE \+ 4 \+ \(size_t\)R \* n_words \+ table_entries\);", s, "topk_lds_bytes")
    _one(r"a\.K2 = \(a\.K \+ 1\) & ~1;", s, "K2")
    _one(r"for \(size_t limit : \{kTopkLdsTwoPerCu, kTopkLdsLimit\}\) \{\s*for \(int R = kTopkMaxRows; R >= kTopkMinRows && !a\.R; R >>= 1\)\s*"
         r"for \(int in_lds = table_entries \? 1 : 0; in_lds >= 0 && !a\.R; --in_lds\) \{", s, "the plan's loops")
    _one(r"topk_plan\(who, a, n_words, n_tables == 1 \? table_size\(N\) : 0, &lds\)", s, "the record call's code book")
    _one(r"topk_lists_cap\(a\.Q, max_workgroups, lds <= kTopkLdsTwoPerCu \? 2 : 1\);", s, "the grid's cap")
    assert _opt_ins(s) == 1                                  # topk_launch, a template: both instances


def test_budget_constants_match_both_sources():
    """vbq_budget.hip and vbqb_sweep.hip state one rule; budget_plan restates it once."""
    for name, limit, max_n in (("vbq_budget.hip", "kBudgetLdsBytes", "kBudgetMaxN"), ("budget/vbqb_sweep.hip", "kSweepLdsBytes", "kSweepMaxN")):
        s = _src(name)
        assert _int(_one(rf"constexpr size_t {limit} = ([^;]+);", s, limit)) == LP.BUDGET_LDS_BYTES
        assert int(_one(rf"constexpr int {max_n} = (\d+);", s, max_n)) == LP.BUDGET_MAX_N
        _one(r"p\.threads = W <= 64 \? 64 : \(W <= 128 \? 128 : 256\);", s, name + ": threads")
        _one(r"const size_t values = \(2 \* W \+ 2 \* \(size_t\)\(N \+ 1\)\) \* sizeof\(double\) \+ 16;", s, name + ": values")
        _one(r"p\.bp_row_bytes = \(\(size_t\)K \* W \+ 15\) & ~\(size_t\)15;", s, name + ": bp_row_bytes")
        _one(rf"p\.ok = values <= {limit};\s*p\.bp_in_lds = p\.ok && values \+ p\.bp_row_bytes <= {limit};", s, name + ": bp_in_lds")
    b, w = _src("vbq_budget.hip"), _src("budget/vbqb_sweep.hip")
    _one(r"const size_t W = \(size_t\)budget \+ 1;", b, "the DP's width")
    _one(r"p\.lds_bytes = values \+ \(p\.bp_in_lds \? p\.bp_row_bytes : 0\);", b, "the DP's LDS")
    _one(r"const size_t W = \(size_t\)width;", w, "the sweep's width")
    _one(r"p\.lds_bytes = values \+ \(S > 0 && p\.bp_in_lds \? p\.bp_row_bytes : 0\);", w, "the sweep's LDS")
    _one(r"const int32_t top = S \? budgets\[S - 1\] \+ 1 : 0;\s*const int32_t width = top > curve_len \? top : curve_len;", w, "width")
    assert _opt_ins(w) == 1                                  # sweep_launch, a template: every instance
    assert _opt_ins(b) == 2                                  # k_budget_dp<true> and k_budget_dp<false>


def test_widest():
    assert LP.widest(lambda x: x <= 37, 1, 1000) == 37 and LP.widest(lambda x: x <= 37, 37, 38) == 37
    assert LP.widest(lambda x: True, 3, 9) == 9 and LP.widest(lambda x: x < 4, 3, 9) == 3
    with pytest.raises(AssertionError):
        LP.widest(lambda x: False, 3, 9)


def test_record_words_worked_numbers():
    assert LP.record_words(18724, 10, 187240) == 8192 and LP.record_fits(18724, 10, 187240)
    assert LP.record_words(18725, 10, 187250) == 8193 and not LP.record_fits(18725, 10, 187250)
    assert LP.widest(lambda K: LP.record_fits(K, 10, 10 * K), 1, 1 << 20) == 18724
    assert LP.record_words(12, 10, 41) == 3 and LP.record_words(7, 10, 10) == 2           # tests/test_gpu_records.py
    assert not LP.record_fits(12, 10, 121) and not LP.record_fits(12, 11, 0) and not LP.record_fits(12, 10, -1)


def test_bag_plan_worked_numbers():
    dense = lambda K: LP.bag_plan(K, 1, 0, 0, 11, 5, CUS, False)                           # noqa: E731
    assert dense(20480) == (163840, False) and dense(20481) is None
    assert dense(8192).lds_bytes == 65536 and dense(8193).lds_bytes == 65544               # the first launch that opts in
    assert LP.widest(lambda K: dense(K) is not None, 1, 1 << 20) == 20480
    assert dense(300).lds_bytes == 2400                                                    # the widest row tested before
    full = lambda K, C=1: LP.bag_plan(K, 10, 10 * K, C, 11, 5, CUS, True)                  # noqa: E731
    assert LP.record_words(16804, 10, 168040) == 7352
    assert full(16804) == (163840, False) == full(16804, 16804) and full(16805) is None
    assert LP.widest(lambda K: full(K) is not None, 1, 1 << 20) == 16804 == LP.BAG_ALWAYS_K
    # the exact fit of the one code book: 6913 + 2 * 16000 + 2047 = 40960 words
    assert LP.record_words(16000, 10, 157216) == 6913 and LP.record_words(16000, 10, 157217) == 6914
    assert LP.bag_plan(16000, 10, 157216, 1, 11, 5, CUS, True) == (163840, True)
    assert LP.bag_plan(16000, 10, 157217, 1, 11, 5, CUS, True) == (155656, False)
    assert LP.bag_plan(16000, 10, 157216, 16000, 11, 5, CUS, True) == (155652, False)      # per-column code books stay in L2
    # the reuse rule (tests/test_gpu_bag.py, test_both_sides_of_the_code_book_choice): 9 bags of 150 ids, 11 bags of 410
    assert not LP.bag_plan(300, 10, 1001, 1, 150, 9, CUS, True).table_in_lds
    assert LP.bag_plan(300, 10, 1001, 1, 410, 11, CUS, True).table_in_lds and LP.bag_plan(65, 3, 60, 1, 150, 9, CUS, True).table_in_lds
    for N in range(1, 11):                                                                 # what kBagAlwaysK promises
        assert all(LP.bag_plan(LP.BAG_ALWAYS_K, N, t, C, 11, 5, CUS, True) for t in (0, N * LP.BAG_ALWAYS_K) for C in (1, LP.BAG_ALWAYS_K))


def test_scores_plan_worked_numbers():
    dense = lambda K: LP.scores_plan(K, 1, 0, False)                                       # noqa: E731
    assert dense(5103) == (8, 5103, 163808) and dense(5104) is None
    assert dense(2031) == (8, 2031, 65504) and dense(2032) == (8, 2033, 65568)             # the first launch that opts in
    assert LP.widest(lambda K: dense(K) is not None, 1, 1 << 20) == 5103
    assert LP.widest(lambda K: dense(K).lds_bytes <= LP.LDS_OPT_IN, 1, 5103) == 2031
    full = lambda K: LP.scores_plan(K, 10, 10 * K, True)                                   # noqa: E731
    assert full(3549) == (8, 3549, 163776) and full(3550) is None
    assert LP.widest(lambda K: full(K) is not None, 1, 1 << 20) == 3549 >= LP.SCORES_ALWAYS_K
    # the groups tests/test_gpu_scores.py names: 64 (K = 1, 5), 32 (40), 16 (64, 65, 100), 8 (300, 512, 700)
    assert [LP.scores_plan(K, 3, K, True).G for K in (1, 5, 40, 64, 65, 100, 300, 512, 700)] == [64, 64, 32, 16, 16, 16, 8, 8, 8]
    assert LP.scores_plan(700, 3, 701, True).lds_bytes == 8 * 64 + 4 * 8 * (701 + 66)      # "about 32 KB"? 25 056
    for N in range(1, 11):                                                                 # what kScoresAlwaysK promises
        assert all(LP.scores_plan(LP.SCORES_ALWAYS_K, N, t, True) for t in (0, N * LP.SCORES_ALWAYS_K))


def test_topk_plan_worked_numbers():
    """The five regimes of the dense source.  K2 = (K + 1) & ~1 is even, so in K they are 1..124, 125..208, 209..310, 311..418
    and 419..624."""
    dense = lambda K: LP.topk_plan(K, 1, 0, 0, False)                                      # noqa: E731
    regime = lambda K: dense(K) and (dense(K).R, dense(K).per_cu)                          # noqa: E731
    assert [regime(K) for K in (1, 124)] == [(128, 2)] * 2 and dense(124).K2 == 124
    assert [regime(K) for K in (125, 208)] == [(64, 2)] * 2 and (dense(125).K2, dense(208).K2) == (126, 208)
    assert [regime(K) for K in (209, 310)] == [(32, 2)] * 2 and (dense(209).K2, dense(310).K2) == (210, 310)
    assert [regime(K) for K in (311, 418)] == [(64, 1)] * 2 and (dense(311).K2, dense(418).K2) == (312, 418)
    assert [regime(K) for K in (419, 624)] == [(32, 1)] * 2 and (dense(419).K2, dense(624).K2) == (420, 624)
    assert dense(624).lds_bytes == 163408 and dense(625) is None
    assert len({regime(K) for K in range(1, 625)}) == 5
    assert dense(300) == (300, 32, False, 79168, 2)                                        # the widest row tested before
    assert dense(310).lds_bytes <= LP.TOPK_LDS_TWO_PER_CU < dense(311).lds_bytes
    # records
    assert LP.record_words(512, 10, 5120) == 224
    assert LP.topk_plan(512, 10, 5120, 1, True) == (512, 32, False, 162960, 1) == LP.topk_plan(512, 10, 5120, 512, True)
    # kTopkAlwaysK = 512 is a guarantee, not the limit: at N = 10 and the full budget the last K that fits is 514 (225 words)
    full = lambda K, C=1: LP.topk_plan(K, 10, 10 * K, C, True)                             # noqa: E731
    assert LP.widest(lambda K: full(K) is not None, 1, 1 << 20) == 514 and full(514) == (514, 32, False, 163608, 1) == full(514, 514)
    assert full(515) is None
    # the one code book beside the smallest tile: up to 166 words per record
    assert LP.topk_plan(512, 10, 3264, 1, True) == (512, 32, True, 163724, 1)
    assert LP.topk_plan(512, 10, 3265, 1, True) == (512, 32, False, 155664, 1)
    for N in range(1, 11):                                                                 # what kTopkAlwaysK promises
        assert all(LP.topk_plan(LP.TOPK_ALWAYS_K, N, t, C, True) for t in (0, N * LP.TOPK_ALWAYS_K) for C in (1, LP.TOPK_ALWAYS_K))


def test_budget_plan_worked_numbers():
    assert LP.budget_plan(1023, 10, 10228) == (256, 163840, False) and LP.budget_plan(1023, 10, 10229) is None
    assert LP.widest(lambda w: LP.budget_plan(1023, 10, w) is not None, 1, 10231) == 10228
    assert LP.budget_plan(150, 10, 985) == (256, 163712, True) and LP.budget_plan(150, 10, 986) == (256, 15968, False)
    assert LP.widest(lambda w: LP.budget_plan(150, 10, w).bp_in_lds, 1, 1501) == 985
    assert LP.budget_bp_row_bytes(150, 986) == 147904 and LP.budget_bp_row_bytes(1023, 10228) == 10463248
    assert [LP.budget_plan(7, 10, w).threads for w in (1, 64, 65, 128, 129)] == [64, 64, 128, 128, 256]
    # tests/test_gpu_budget_dp.py: K = 300, N = 16 at budget 1600 is the workspace path, 4800 value rows above 64 KiB
    assert not LP.budget_plan(300, 16, 1601).bp_in_lds and LP.budget_plan(300, 16, 4801) == (256, 77104, False)


# ------------------------------------------------------------------------------------------------ worked numbers, 256 CUs
def test_lookup_plan_worked_numbers():
    p = LP.lookup_plan(8, 256, 20740, 10, CUS)
    assert p.z_lds and p.nb_lds and p.groups == 16 and p.renumbered
    assert (p.splits, p.per, p.last_split_rows) == (28, 768, 4)
    assert LP.walk(p.per) == LP.Walk(1, 1, 256) and LP.walk(p.last_split_rows) == LP.Walk(0, 1, 4)
    assert LP.walk(20740) == LP.Walk(40, 2, 4)                     # the num_bits pass: 81 whole blocks and four rows
    p = LP.lookup_plan(5, 256, 33028, 10, CUS)
    assert p.z_lds and (p.splits, p.per) == (26, 1280) and LP.walk(p.per) == LP.Walk(2, 1, 256)
    assert LP.walk(p.last_split_rows) == LP.Walk(2, 1, 4)
    p = LP.lookup_plan(8, 260, 20740, 10, CUS)
    assert p.z_lds and p.groups == 17 and not p.renumbered and p.last_group_channels == 4
    assert (p.splits, p.per, p.last_split_rows) == (28, 768, 4) and LP.walk(p.per, whole_group=False) == LP.Walk(0, 3, 256)
    p = LP.lookup_plan(3, 64, 65540, 10, CUS)
    assert p.z_lds and p.groups == 4 and (p.splits, p.per, p.last_split_rows) == (86, 768, 260)
    assert LP.walk(260) == LP.Walk(0, 2, 4)
    p = LP.lookup_plan(64, 16, 2308, 10, CUS)
    assert p.z_lds and not p.nb_lds and (p.groups, p.splits, p.per, p.last_split_rows) == (1, 10, 256, 4)
    p = LP.lookup_plan(2, 256, 3076, 10, CUS)
    assert not p.z_lds and p.nb_lds and LP.walk(3076) == LP.Walk(6, 1, 4)
    # the existing shapes of test_gather_latents_one_pass_against_numpy: one block per split, the pipelined loop never runs
    for L, C, B in ((16, 64, 4096), (3, 20, 16388), (2, 36, 3076)):
        p = LP.lookup_plan(L, C, B, 10, CUS)
        assert not p.renumbered and (not p.z_lds or p.per == LP.LDS_ROWS)
    # refusals of the LDS form
    assert not LP.lookup_plan(8, 256, 20742, 10, CUS).eligible and not LP.lookup_plan(8, 254, 20740, 10, CUS).eligible
    assert not LP.lookup_plan(8, 256, 20740, 11, CUS).eligible
    assert not LP.lookup_plan(8, 256, 18428, 10, CUS).z_lds and LP.lookup_plan(8, 256, 18432, 10, CUS).z_lds
    assert not LP.lookup_plan(1, 256, 3068, 10, CUS).nb_lds and LP.lookup_plan(1, 256, 3072, 10, CUS).nb_lds


def test_renumbering_is_a_permutation_inside_every_sixteen():
    for groups in (16, 32, 48):
        got = [LP.renumbered(g, groups) for g in range(groups)]
        assert sorted(got) == list(range(groups))
        assert all(a // 16 == g // 16 for g, a in enumerate(got))
        assert all(abs(got.index(2 * k) - got.index(2 * k + 1)) == 8 for k in range(groups // 2))   # one XCD of eight
    assert [LP.renumbered(g, 17) for g in range(17)] == list(range(17))


def test_find_lookup_shape_takes_the_worked_shape_or_an_equivalent_one():
    assert LP.find_lookup_shape(CUS, 256, 10, 3, 4, prefer=20740) == (8, 20740)
    assert LP.find_lookup_shape(CUS, 256, 10, 5, None, prefer=33028) == (5, 33028)
    assert LP.find_lookup_shape(CUS, 260, 10, 3, 4, prefer=20740) == (8, 20740)
    assert LP.find_lookup_shape(CUS, 64, 10, 3, 260, prefer=65540) == (3, 65540)
    for cus in (32, 64, 80, 104, 128, 228, 256, 304):              # other devices: the worked rows do not fit, others do
        for C, bps, last in ((256, 3, 4), (256, 5, None), (260, 3, 4), (64, 3, 260)):
            found = LP.find_lookup_shape(cus, C, 10, bps, last, prefer=20740)
            assert found is not None, (cus, C)
            L, B = found
            p = LP.lookup_plan(L, C, B, 10, cus)
            assert p.z_lds and p.per == bps * 256 and last in (None, p.last_split_rows) and L * B * C <= 44_000_000


def test_rank_plan_worked_numbers():
    p = LP.rank_plan(10277, 100, 1000, CUS)
    assert (p.qb, p.nt, p.tiles_per_wg, p.splits, p.last_wg_tiles) == (8, 81, 2, 41, 1)
    p = LP.rank_plan(33000, 1, 520, CUS)
    assert (p.qb, p.nt, p.tiles_per_wg, p.splits, p.last_wg_tiles) == (5, 258, 3, 86, 3)
    for K, nk, k2, kend in ((1, 1, 2, 2), (31, 1, 32, 32), (32, 1, 32, 32), (33, 2, 34, 2), (64, 2, 64, 32), (65, 3, 66, 2)):
        p = LP.rank_plan(10277, K, 1000, CUS)
        assert (p.nk, p.k2, p.kend_last) == (nk, k2, kend)
    # every shape the suite compared with a reference before: one tile per workgroup
    for V, K, Q in ((1, 3, 2), (127, 16, 1), (129, 17, 130), (1000, 300, 257), (5000, 33, 64)):
        assert LP.rank_plan(V, K, Q, CUS).tiles_per_wg == 1
    p = LP.rank_plan(100_000, 100, 19_544, CUS)                    # the notebook's size: several tiles, a clamped last range
    assert p.tiles_per_wg >= 2 and p.last_wg_tiles < p.tiles_per_wg


def test_find_rank_words_takes_the_worked_shape_or_an_equivalent_one():
    assert LP.find_rank_words(CUS, 1000, 65, 2, True, prefer=10277) == 10277
    assert LP.find_rank_words(CUS, 520, 1, 3, False, prefer=33000) == 33000
    for cus in (64, 80, 104, 128, 228, 256, 304):
        V = LP.find_rank_words(cus, 1000, 65, 2, True)
        p = LP.rank_plan(V, 65, 1000, cus)
        assert p.tiles_per_wg >= 2 and p.last_wg_tiles < p.tiles_per_wg and V * 1000 * 65 <= 1e9
        V = LP.find_rank_words(cus, 520, 1, 3, False)
        assert LP.rank_plan(V, 1, 520, cus).tiles_per_wg >= 3


def test_grid_caps_worked_numbers():
    assert LP.moments_flat_grid(6_300_000, 1) == (2049, 3 * 2049 * 256)        # "more than 6.29 M floats at C = 1"
    assert 4 * LP.moments_flat_grid(6_300_000, 1)[1] == 6_294_528
    assert LP.moments_flat_grid(101_380, 64) == (33, 25_344)                   # "more than 101 376 rows at C = 64"
    assert LP.moments_flat_grid(39_960, 1)[0] * 3 * 256 > 39_960 // 4          # the largest shape tested before: no main loop
    assert LP.moments_bc_grid(33, 4096) == (33, 8192)
    assert LP.rd_sums_grid(4995, 8, CUS) == (20, 1, 1)                         # the one shape tested before: one pass
    assert LP.rd_sums_grid(640_000, 9, CUS) == (1025, 2, 3)
    assert LP.rd_sums_grid(524_544, 8, CUS)[2] == 1 and LP.rd_sums_grid(524_545, 8, CUS)[2] == 2      # "needs E > 524 k"
    assert LP.scan_grid(1 << 20) == (4096, 1) and LP.scan_grid((1 << 20) + 1) == (4096, 2)
    assert LP.scan_grid((1 << 21) + 3) == (4096, 3) and LP.scan_grid(24_576) == (96, 1)
    assert LP.hist_tiled_grid(20_000, 40, 32) == (6, 3, 53)


@pytest.mark.parametrize("rows,want", [(0, (0, 0, 0)), (4, (0, 1, 4)), (256, (0, 1, 256)), (260, (0, 2, 4)), (512, (1, 0, 0)),
                                       (768, (1, 1, 256)), (1028, (2, 1, 4)), (1280, (2, 1, 256))])
def test_walk(rows, want):
    assert tuple(LP.walk(rows)) == want
    assert LP.walk(rows, whole_group=False).pipelined == 0
    assert LP.walk(rows, whole_group=False).rest == LP.cdiv(rows, 256)
