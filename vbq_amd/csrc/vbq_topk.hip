// Nearest rows of an embedding matrix to a few queries, without a decoded copy of the matrix: the rows come either from
// fixed-size records ("VBQr", vbq_records.hip) or from a dense [V, K] f32 matrix, are unpacked straight into the operand tile
// of the matrix cores, scored by the exact f32 MFMA chain and reduced to the k best per query on the chip.  The semantics
// (score chain, cosine denominator, total order, exclusion, padding, damaged records) are stated in include/vbq.h.
//   k_topk<records>  4 waves; blockIdx.y = a block of 32 queries kept in LDS as [k][32] for the whole workgroup, blockIdx.x
//                    strides over tiles of R = 128, 64 or 32 rows (the largest that fits the LDS).  Per tile: the records of the
//                    tile are staged with one coalesced copy; each wave decodes every fourth row with the unpack's scan
//                    (decode_record of vbq_records_common.h, rank -> value) into the B tile [k][R + 1] -- the odd row
//                    stride keeps both the decode's stores (lane -> k) and the operand fetch (lane & 31 -> row, lane >> 5 -> k)
//                    free of bank conflicts; after a barrier wave w runs the 32x32x2 chain over k for rows 32 w .. 32 w + 31 and
//                    adds up the rows' squared norms from the operands it fetches anyway.  A score enters a query's list only
//                    when it reaches the list's threshold, which is rare after the first tiles: then the 32 x R scores go
//                    through LDS (in place of the B tile) and each wave inserts for eight queries, one list entry per lane.
//                    The lists [grid.x][Q][k] live in the workspace; a lane only ever reads back what it wrote itself.
//   k_topk_merge     one wave per query: the same insertion over the grid.x lists, then the padded result.
// The order (score descending, id ascending) is total and every row is offered exactly once, so the result does not depend
// on the grid or on the order of the tiles.  Record words are untrusted exactly as in k_records_unpack: no read leaves the
// staged image, a record that fails a check counts as a row of zeros and sets the status bits.  gfx950 / ROCm only.
#include <limits.h>
#include <math.h>

#include "vbq_records_common.h"

namespace vbq {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTopkThreads = 256;
constexpr int kTopkWaves = kTopkThreads / kWave;
constexpr int kTopkQ = 32;                           // queries per workgroup: the M of one 32x32 MFMA tile
constexpr int kTopkMaxK = 64;                        // results per query: one list entry per lane
constexpr int kTopkMaxE = 8;
constexpr int kTopkMinRows = 32, kTopkMaxRows = 128; // rows per tile
constexpr size_t kTopkLdsLimit = 160 * 1024;         // per CU
constexpr size_t kTopkLdsTwoPerCu = 80 * 1024;
constexpr int kTopkAlwaysK = 512;                    // every K up to here fits at the smallest tile, whatever N and total_bits
constexpr long long kNoId = LLONG_MAX;               // the id of an empty list entry: after every row

// (score, id) a comes before b: score descending as IEEE values (-0 == 0), then id ascending.
__device__ __forceinline__ bool comes_before(float as, long long ai, float bs, long long bi) {
    return as > bs || (as == bs && ai < bi);
}

// A sorted list of k <= 64 entries, entry i in lane i: put the wave-uniform candidate (cs, ci) where it belongs and drop the
// last entry; a candidate that comes after all k changes nothing.
__device__ __forceinline__ void list_insert(float &es, long long &ei, float cs, long long ci, int k, int lane) {
    const int pos = __popcll(__ballot(lane < k && comes_before(es, ei, cs, ci)));
    const float us = __shfl_up(es, 1, kWave);
    const long long ui = __shfl_up(ei, 1, kWave);
    if (lane == pos) { es = cs; ei = ci; }
    else if (lane > pos) { es = us; ei = ui; }
}

struct TopkArgs {
    const float *emb;                 // the dense source [V][K]
    const unsigned int *words;        // the record source [V][n_words]
    const float *table;
    int N, total_bits, n_words, per_column, table_in_lds;
    unsigned int *status;
    const float *queries;
    long Q, V;
    int K, K2, k, metric;
    const long long *exclude;
    int E;
    int R;                            // rows per tile
    long tiles;
    long long *ws_ids;                // [grid.x][Q][k]
    float *ws_scores;
};

// LDS of k_topk in bytes: queries [K2][32], B tile [max(K2, 32)][R + 1] (the scores [32][R + 1] take its place on the slow
// path), thresholds, exclusions, two flags, the staged records, the one code book.
size_t topk_lds_bytes(int K2, int R, int64_t n_words, int table_entries) {
    const size_t bt = (size_t)(K2 > kTopkQ ? K2 : kTopkQ) * (R + 1);
    return 4 * ((size_t)K2 * kTopkQ + bt + kTopkQ + kTopkQ * kTopkMaxE + 4 + (size_t)R * n_words + table_entries);
}

template <bool kRecords>
__global__ void __launch_bounds__(kTopkThreads)
k_topk(const TopkArgs a) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lh = lane >> 5;
    const int R = a.R, RS = R + 1, K = a.K, K2 = a.K2, k = a.k;
    float *Qs = lds;
    float *Bs = Qs + K2 * kTopkQ;
    float *thr = Bs + (K2 > kTopkQ ? K2 : kTopkQ) * RS;
    int *excl = reinterpret_cast<int *>(thr + kTopkQ);
    int *flag = excl + kTopkQ * kTopkMaxE;
    unsigned int *stage = reinterpret_cast<unsigned int *>(flag + 4);
    const int n_words = a.n_words;
    const int T = table_size(a.N);
    const float *tab = a.table;
    if (kRecords && a.table_in_lds) {
        float *lt = reinterpret_cast<float *>(stage + R * n_words);
        for (int i = tid; i < T; i += kTopkThreads) lt[i] = a.table[i];
        tab = lt;
    }
    const long q0 = (long)blockIdx.y * kTopkQ;
    for (int i = tid; i < K2 * kTopkQ; i += kTopkThreads) {
        const int kk = i >> 5, q = i & 31;
        Qs[i] = (q0 + q < a.Q && kk < K) ? a.queries[(q0 + q) * K + kk] : 0.0f;
    }
    if (tid < kTopkQ) thr[tid] = q0 + tid < a.Q ? -INFINITY : INFINITY;     // nothing reaches the list of a query that is not there
    for (int i = tid; i < kTopkQ * kTopkMaxE; i += kTopkThreads) {
        const int q = i >> 3, e = i & 7;
        long long v = -1;
        if (q0 + q < a.Q && e < a.E) v = a.exclude[(q0 + q) * a.E + e];
        excl[i] = (v >= 0 && v < a.V) ? (int)v : -1;
    }
    if (tid < 2) flag[tid] = 0;
    for (int j = 0; j < kTopkQ / kTopkWaves; ++j) {                          // the wave's eight lists start empty
        const long q = q0 + wave + kTopkWaves * j;
        if (q < a.Q && lane < k) {
            const long at = ((long)blockIdx.x * a.Q + q) * k + lane;
            a.ws_scores[at] = -INFINITY;
            a.ws_ids[at] = kNoId;
        }
    }
    __syncthreads();

    int par = 0;
    for (long t = blockIdx.x; t < a.tiles; t += gridDim.x, par ^= 1) {
        const long v0 = t * R;
        const int valid = a.V - v0 < R ? (int)(a.V - v0) : R;
        if (kRecords) {
            const unsigned int *src = a.words + v0 * n_words;
            for (int i = tid; i < valid * n_words; i += kTopkThreads) stage[i] = src[i];
            __syncthreads();
        }
        for (int r = wave; r < R; r += kTopkWaves) {
            float *col = Bs + r;
            if (r >= valid) {
                for (int kk = lane; kk < K2; kk += kWave) col[kk * RS] = 0.0f;
            } else if (kRecords) {
                const unsigned int bad = decode_record(stage + r * n_words, n_words, K, a.N, a.total_bits, lane,
                                                       [&](int kk, unsigned int q) {
                    col[kk * RS] = tab[(a.per_column ? (long)kk * T : 0L) + q];
                });
                if (bad) {                                                   // wave-uniform: a rejected row counts as zeros
                    for (int kk = lane; kk < K; kk += kWave) col[kk * RS] = 0.0f;
                    if (lane == 0 && a.status) atomicOr(a.status, bad);
                }
                if ((K & 1) && lane == 0) col[K * RS] = 0.0f;
            } else {
                const float *row = a.emb + (v0 + r) * K;
                for (int kk = lane; kk < K2; kk += kWave) col[kk * RS] = kk < K ? row[kk] : 0.0f;
            }
        }
        __syncthreads();                                                     // the B tile is whole

        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
        const bool mine = kTopkQ * wave < R;                                 // wave-uniform: rows 32 w .. 32 w + 31 exist
        const long my_row = v0 + kTopkQ * wave + lr;
        if (mine) {
            const float *qa = Qs + lh * kTopkQ + lr;
            const float *bb = Bs + lh * RS + kTopkQ * wave + lr;
            float sum = 0.0f;                                                // of row lr's squares, the same in every lane
            for (int kk = 0; kk < K2; kk += 2) {
                const float av = qa[kk * kTopkQ], bv = bb[kk * RS];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
                if (a.metric) {
                    const float b0 = __shfl(bv, lr, kWave), b1 = __shfl(bv, lr + 32, kWave);
                    sum = __fadd_rn(sum, __fmul_rn(b0, b0));                 // a padded k adds +0: no change
                    sum = __fadd_rn(sum, __fmul_rn(b1, b1));
                }
            }
            const float den = __fadd_rn(1e-8f, sqrtf(sum));
            bool pass = false;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float s = a.metric ? __fdiv_rn(acc[i], den) : acc[i];
                acc[i] = s;
                pass |= s >= thr[8 * (i >> 2) + 4 * lh + (i & 3)];
            }
            if (pass && my_row < a.V) flag[par] = 1;
        }
        __syncthreads();                                                     // the B tile is free, the flag is final
        const bool slow = flag[par] != 0;
        if (tid == 0) flag[par ^ 1] = 0;                                     // the next tile's
        if (slow) {
            float *S = Bs;                                                   // [32][R + 1]
            if (mine) {
#pragma unroll
                for (int i = 0; i < 16; ++i) S[(8 * (i >> 2) + 4 * lh + (i & 3)) * RS + kTopkQ * wave + lr] = acc[i];
            }
            __syncthreads();
            for (int j = 0; j < kTopkQ / kTopkWaves; ++j) {
                const int qi = wave + kTopkWaves * j;
                const long q = q0 + qi;
                if (q >= a.Q) continue;                                      // wave-uniform
                const long at = ((long)blockIdx.x * a.Q + q) * k + lane;
                float es = lane < k ? a.ws_scores[at] : -INFINITY;
                long long ei = lane < k ? a.ws_ids[at] : kNoId;
                bool changed = false;
                for (int c0 = 0; c0 < R; c0 += kWave) {
                    const int c = c0 + lane;
                    const long row = v0 + c;
                    const float s = c < R ? S[qi * RS + c] : 0.0f;
                    const float ls = __shfl(es, k - 1, kWave);
                    const long long li = __shfl(ei, k - 1, kWave);
                    bool pass = c < R && row < a.V && comes_before(s, row, ls, li);
                    if (pass)
                        for (int e = 0; e < a.E; ++e) pass = pass && excl[qi * kTopkMaxE + e] != (int)row;
                    unsigned long long mask = __ballot(pass);
                    while (mask) {
                        const int b = __builtin_ctzll(mask);
                        mask &= mask - 1;
                        list_insert(es, ei, __shfl(s, b, kWave), v0 + c0 + b, k, lane);
                        changed = true;
                    }
                }
                if (changed) {
                    const float ls = __shfl(es, k - 1, kWave);
                    if (lane < k) {
                        a.ws_scores[at] = es;
                        a.ws_ids[at] = ei;
                    }
                    if (lane == 0) thr[qi] = ls;
                }
            }
        }
        __syncthreads();                                                     // the scores are read, the thresholds written
    }
}

__global__ void __launch_bounds__(kWave)
k_topk_merge(const long long *__restrict__ ws_ids, const float *__restrict__ ws_scores, int n_lists, long Q, int k,
             long long *__restrict__ out_ids, float *__restrict__ out_scores) {
    const int lane = threadIdx.x;
    const long q = blockIdx.x;
    float es = -INFINITY;
    long long ei = kNoId;
    const long total = (long)n_lists * k;
    for (long c0 = 0; c0 < total; c0 += kWave) {
        const long c = c0 + lane;
        const bool have = c < total;
        const long at = have ? ((c / k) * Q + q) * k + c % k : 0;
        const float s = have ? ws_scores[at] : -INFINITY;
        const long long id = have ? ws_ids[at] : kNoId;
        const float ls = __shfl(es, k - 1, kWave);
        const long long li = __shfl(ei, k - 1, kWave);
        unsigned long long mask = __ballot(have && comes_before(s, id, ls, li));
        while (mask) {
            const int b = __builtin_ctzll(mask);
            mask &= mask - 1;
            list_insert(es, ei, __shfl(s, b, kWave), __shfl(id, b, kWave), k, lane);
        }
    }
    if (lane < k) {
        out_ids[q * k + lane] = ei == kNoId ? -1 : ei;
        out_scores[q * k + lane] = es;
    }
}

// What both calls take alike.
int topk_check(const char *who, int64_t V, int32_t K, int64_t Q, int32_t k, int32_t metric, int32_t E) {
    VBQ_REQUIRE(V >= 1 && V < (1ll << 31) && K >= 1 && Q >= 0 && Q <= 65535ll * kTopkQ, VBQ_ERR_INVALID_ARGUMENT,
                "%s: bad sizes V=%lld K=%d Q=%lld (need 1 <= V < 2^31, K >= 1, 0 <= Q <= %lld)", who, (long long)V, K,
                (long long)Q, 65535ll * kTopkQ);
    VBQ_REQUIRE(k >= 1 && k <= kTopkMaxK, VBQ_ERR_INVALID_ARGUMENT, "%s: k = %d outside 1..%d", who, k, kTopkMaxK);
    VBQ_REQUIRE(metric == 0 || metric == 1, VBQ_ERR_INVALID_ARGUMENT, "%s: metric %d is neither 0 (dot) nor 1 (cosine)", who,
                metric);
    VBQ_REQUIRE(E >= 0 && E <= kTopkMaxE, VBQ_ERR_INVALID_ARGUMENT, "%s: E = %d exclusions per query outside 0..%d", who, E,
                kTopkMaxE);
    return VBQ_OK;
}

// The most lists per query a call can write: what the workspace is sized by.  max_workgroups > 0 caps the row split;
// otherwise two workgroups per CU, shared among the query blocks.
int64_t topk_lists_cap(int64_t Q, int32_t max_workgroups, int per_cu) {
    if (max_workgroups > 0) return max_workgroups;
    const int64_t qb = (Q + kTopkQ - 1) / kTopkQ;
    const int64_t cap = (int64_t)num_cus() * per_cu / (qb > 0 ? qb : 1);
    return cap > 0 ? cap : 1;
}

size_t topk_workspace(int64_t V, int64_t Q, int32_t k, int32_t max_workgroups) {
    const int64_t tiles = (V + kTopkMinRows - 1) / kTopkMinRows, cap = topk_lists_cap(Q, max_workgroups, 2);
    return (size_t)(tiles < cap ? tiles : cap) * (size_t)Q * (size_t)k * 12;
}

// The tile of a call: the largest that leaves room for two workgroups per CU, else the largest that fits at all; the one code
// book goes to LDS where it fits beside the tile.  Sets K2, R and table_in_lds; *lds gets the bytes.
int topk_plan(const char *who, TopkArgs &a, int64_t n_words, int table_entries, size_t *lds) {
    a.K2 = (a.K + 1) & ~1;
    a.R = 0;
    for (size_t limit : {kTopkLdsTwoPerCu, kTopkLdsLimit}) {
        for (int R = kTopkMaxRows; R >= kTopkMinRows && !a.R; R >>= 1)
            for (int in_lds = table_entries ? 1 : 0; in_lds >= 0 && !a.R; --in_lds) {
                *lds = topk_lds_bytes(a.K2, R, n_words, in_lds ? table_entries : 0);
                if (*lds <= limit) {
                    a.R = R;
                    a.table_in_lds = in_lds;
                }
            }
        if (a.R) break;
    }
    VBQ_REQUIRE(a.R, VBQ_ERR_UNSUPPORTED,
                "%s: K = %d (%lld words per record) needs %zu bytes of LDS at the smallest tile, the limit is %zu (every "
                "K <= %d fits); decode the matrix instead", who, a.K, (long long)n_words, *lds, kTopkLdsLimit, kTopkAlwaysK);
    return VBQ_OK;
}

template <bool kRecords>
int topk_launch(const char *who, TopkArgs a, size_t lds, long long *d_out_ids, float *d_out_scores, int32_t max_workgroups,
                void *d_workspace, size_t workspace_bytes, hipStream_t st) {
    a.tiles = (long)((a.V + a.R - 1) / a.R);
    const int64_t cap = topk_lists_cap(a.Q, max_workgroups, lds <= kTopkLdsTwoPerCu ? 2 : 1);
    const unsigned gx = (unsigned)(a.tiles < cap ? a.tiles : cap), gy = (unsigned)((a.Q + kTopkQ - 1) / kTopkQ);
    const size_t entries = (size_t)gx * (size_t)a.Q * (size_t)a.k;
    VBQ_REQUIRE(workspace_bytes >= entries * 12, VBQ_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes,
                entries * 12);
    a.ws_ids = reinterpret_cast<long long *>(d_workspace);
    a.ws_scores = reinterpret_cast<float *>(a.ws_ids + entries);
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(k_topk<kRecords>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
        (void)hipGetLastError();                                     // the launch below reports what is wrong, if anything
    hipLaunchKernelGGL(k_topk<kRecords>, dim3(gx, gy), dim3(kTopkThreads), lds, st, a);
    VBQ_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)a.Q), dim3(kWave), 0, st, a.ws_ids, a.ws_scores, (int)gx, a.Q, a.k, d_out_ids,
                       d_out_scores);
    VBQ_CHECK_LAUNCH(who);
    return VBQ_OK;
}

}  // namespace
}  // namespace vbq

extern "C" size_t vbq_topk_workspace_bytes(int64_t V, int32_t K, int64_t Q, int32_t k, int32_t max_workgroups) {
    using namespace vbq;
    if (V < 1 || V >= (1ll << 31) || K < 1 || Q < 1 || Q > 65535ll * kTopkQ || k < 1 || k > kTopkMaxK || max_workgroups < 0)
        return 0;
    return topk_workspace(V, Q, k, max_workgroups);
}

extern "C" int vbq_records_topk_f32(const uint32_t *d_words, int64_t n_rows, int32_t K, int32_t N, int32_t total_bits,
                                    const float *d_table_sorted, int32_t n_tables, const float *d_queries, int64_t Q, int32_t k,
                                    int32_t metric, const int64_t *d_exclude, int32_t E, int64_t *d_out_ids, float *d_out_scores,
                                    uint32_t *d_status, int32_t max_workgroups, void *d_workspace, size_t workspace_bytes,
                                    void *stream) {
    using namespace vbq;
    const char *who = "vbq_records_topk_f32";
    VBQ_REQUIRE(K >= 1 && N >= 1 && N <= kRecordsMaxN, VBQ_ERR_INVALID_ARGUMENT, "%s: bad sizes K=%d N=%d (need K >= 1, 1 <= N <= 10)",
                who, K, N);
    if (int rc = record_check_total_bits(who, K, N, total_bits)) return rc;
    VBQ_REQUIRE(n_tables == 1 || n_tables == K, VBQ_ERR_INVALID_ARGUMENT, "%s: n_tables = %d is neither 1 nor K = %d", who,
                n_tables, K);
    if (int rc = topk_check(who, n_rows, K, Q, k, metric, E)) return rc;
    VBQ_REQUIRE(max_workgroups >= 0, VBQ_ERR_INVALID_ARGUMENT, "%s: negative max_workgroups %d", who, max_workgroups);
    int64_t n_words = 0;
    if (int rc = record_check_words(who, K, N, total_bits, &n_words)) return rc;
    TopkArgs a = {};
    a.K = K;
    size_t lds = 0;
    if (int rc = topk_plan(who, a, n_words, n_tables == 1 ? table_size(N) : 0, &lds)) return rc;
    if (Q == 0) return VBQ_OK;
    VBQ_REQUIRE(d_words && d_table_sorted && d_queries && d_out_ids && d_out_scores && d_workspace && (d_exclude || E == 0),
                VBQ_ERR_INVALID_ARGUMENT, "%s: null pointer argument", who);
    a.words = d_words;
    a.table = d_table_sorted;
    a.N = N;
    a.total_bits = total_bits;
    a.n_words = (int)n_words;
    a.per_column = n_tables > 1;
    a.status = d_status;
    a.queries = d_queries;
    a.Q = (long)Q;
    a.V = (long)n_rows;
    a.k = k;
    a.metric = metric;
    a.exclude = reinterpret_cast<const long long *>(d_exclude);
    a.E = E;
    return topk_launch<true>(who, a, lds, reinterpret_cast<long long *>(d_out_ids), d_out_scores, max_workgroups, d_workspace,
                             workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int vbq_topk_f32(const float *d_emb, int64_t V, int32_t K, const float *d_queries, int64_t Q, int32_t k, int32_t metric,
                            const int64_t *d_exclude, int32_t E, int64_t *d_out_ids, float *d_out_scores, int32_t max_workgroups,
                            void *d_workspace, size_t workspace_bytes, void *stream) {
    using namespace vbq;
    const char *who = "vbq_topk_f32";
    if (int rc = topk_check(who, V, K, Q, k, metric, E)) return rc;
    VBQ_REQUIRE(max_workgroups >= 0, VBQ_ERR_INVALID_ARGUMENT, "%s: negative max_workgroups %d", who, max_workgroups);
    TopkArgs a = {};
    a.K = K;
    size_t lds = 0;
    if (int rc = topk_plan(who, a, 0, 0, &lds)) return rc;
    if (Q == 0) return VBQ_OK;
    VBQ_REQUIRE(d_emb && d_queries && d_out_ids && d_out_scores && d_workspace && (d_exclude || E == 0), VBQ_ERR_INVALID_ARGUMENT,
                "%s: null pointer argument", who);
    a.emb = d_emb;
    a.N = 1;
    a.queries = d_queries;
    a.Q = (long)Q;
    a.V = (long)V;
    a.k = k;
    a.metric = metric;
    a.exclude = reinterpret_cast<const long long *>(d_exclude);
    a.E = E;
    return topk_launch<false>(who, a, lds, reinterpret_cast<long long *>(d_out_ids), d_out_scores, max_workgroups, d_workspace,
                              workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}
