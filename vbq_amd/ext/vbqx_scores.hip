// Listed rows: the score of each query against the rows the caller names for it, without the [Q M, K] matrix of the listed
// rows in between.  The rows come either from fixed-size records ("VBQr", vbq_records.hip) or from a dense [V, K] f32 matrix.
// The semantics (pairs, padding, status bits, damaged records) are stated in include/vbq_ext.h, "Listed rows"; the score is
// the one of include/vbq.h, "Nearest rows".
//   k_scores<records, cosine>  one wave per group of G consecutive flat pairs p = q M + m, one workgroup per group.  The ids of
//                    the group go to LDS; the records they name are staged with one coalesced copy (every load in flight at
//                    once) and decoded one after the other by the unpack's scan (decode_record of vbq_records_common.h) into
//                    the tile [G][RS], RS = K | 1: the odd row stride keeps both the decode's stores (lane -> k) and the
//                    chains' loads (lane -> pair) free of bank conflicts.  The tile holds RANKS: the decode touches LDS only.
//                    Lane j then walks pair j's chain over ascending k -- __fmaf_rn for the score, __fmul_rn / __fadd_rn for
//                    the squared norm -- with v_k = table[rank] (the loads do not depend on the chain and run ahead of it)
//                    and q_k from its query through L2 (the lanes of one query read one address).  The dense loader fills
//                    the same tile with the values themselves: the two sources agree bit for bit.
// Group size.  A record's scan is a chain of dependent LDS reads and wave shuffles that one wave walks alone, record after
// record: what hides it is other waves, not more pairs per wave.  Measured on an MI355X (100 000 x 100 file, 3 bits per
// coordinate, 1 024 000 pairs, cosine): G = 64 1.27 ms, 32 0.77, 16 0.44, 8 0.44, 4 0.70, 2 1.02, 1 1.59 -- below 8 the idle
// lanes of the chains cost more than the extra waves give.  So G is the largest of 64, 32, 16 that keeps the workgroup's LDS
// within 8 KiB, and 8 otherwise (K = 100: 16; K >= 128 or so: 8).
// The chain over k is the definition, so a pair is serial in k and owned by one lane from its first step to its last: the
// result does not depend on G or on where a pair falls in its group.  Record words are untrusted exactly as in
// k_records_unpack: no read leaves the staged record, a record that fails a check counts as a row of zeros and sets the status
// bits.  gfx950 / ROCm only.
#include <limits.h>
#include <math.h>

#include "vbq_records_common.h"
#include "vbq_ext.h"

namespace vbq {
namespace {

#ifndef VBQX_SCORES_LDS_TARGET          // -DVBQX_SCORES_LDS_TARGET=<bytes> -DVBQX_SCORES_MIN_GROUP=<pairs> build other group sizes, for A/B timing
#define VBQX_SCORES_LDS_TARGET (8 * 1024)
#endif
#ifndef VBQX_SCORES_MIN_GROUP
#define VBQX_SCORES_MIN_GROUP 8
#endif
constexpr int kScoresMaxGroup = kWave, kScoresMinGroup = VBQX_SCORES_MIN_GROUP;     // pairs per wave
constexpr size_t kScoresLdsLimit = 160 * 1024;                  // per CU
constexpr size_t kScoresLdsTarget = VBQX_SCORES_LDS_TARGET;
// Every K up to here fits at the smallest group whatever N, total_bits and n_tables: 8 ((K | 1) + ceil(14 K / 32)) + 128 words
// <= 40960 (N = 10, total_bits = 10 K).
constexpr int kScoresAlwaysK = 3500;
constexpr int64_t kScoresMaxGroups = INT_MAX;                   // grid.x

struct ScoresArgs {
    const float *emb;                 // the dense source [V][K]
    const unsigned int *words;        // the record source [V][n_words]
    const float *table;
    long V;
    int K, N, total_bits, n_words, per_column;
    const float *queries;
    const long long *ids;
    long P, M;                        // pairs in all, pairs per query
    int G, RS;                        // pairs per group, floats per tile row
    float *out;
    unsigned int *status;
};

// LDS of k_scores in bytes: the ids of the group, the tile [G][RS], the staged records [G][n_words].
size_t scores_lds_bytes(int G, int RS, int64_t n_words) {
    return 8 * (size_t)kWave + 4 * ((size_t)G * RS + (size_t)G * (size_t)n_words);
}

// A value every lane holds alike, in scalar registers: the branches on it are uniform for the compiler too.
__device__ __forceinline__ long wave_uniform(long long v) {
    const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)v);
    const unsigned int hi = __builtin_amdgcn_readfirstlane((unsigned int)((unsigned long long)v >> 32));
    return (long)(((unsigned long long)hi << 32) | lo);
}

template <bool kRecords, bool kCosine>
__global__ void __launch_bounds__(kWave)
k_scores(const ScoresArgs a) {
    extern __shared__ long long group_ids[];
    const int lane = threadIdx.x;
    const int K = a.K, RS = a.RS, n_words = a.n_words;
    float *tile = reinterpret_cast<float *>(group_ids + kWave);
    unsigned int *stage = reinterpret_cast<unsigned int *>(tile + a.G * RS);
    const long p0 = (long)blockIdx.x * a.G;
    const int n = a.P - p0 < a.G ? (int)(a.P - p0) : a.G;            // pairs of this group, >= 1
    long long my_id = -1;
    if (lane < n) my_id = a.ids[p0 + lane];
    const bool listed = my_id >= 0 && my_id < a.V;                   // neither padding nor out of range
    group_ids[lane] = listed ? my_id : -1;
    unsigned int st = __any(my_id >= a.V) ? (unsigned int)kUnpackBadRow : 0u;    // wave-uniform
    unsigned int *ranks = reinterpret_cast<unsigned int *>(tile);    // the record source's tile: every entry < T
    bool zero_row = false;                                           // this lane's pair names a record that failed a check
    __syncthreads();

    if (kRecords) {
        for (int i = lane; i < n * n_words; i += kWave) {
            const int j = i / n_words;
            const long long id = group_ids[j];
            if (id >= 0) stage[i] = a.words[id * n_words + (i - j * n_words)];
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const long id = wave_uniform(group_ids[j]);
            if (id < 0) continue;
            unsigned int *row = ranks + j * RS;
            const unsigned int bad = decode_record(stage + j * n_words, n_words, K, a.N, a.total_bits, lane,
                                                   [&](int k, unsigned int q) { row[k] = q; });
            if (bad) {                                               // wave-uniform: a rejected record is a row of zeros
                st |= bad;
                zero_row |= lane == j;
            }
        }
    } else {
        for (int i = lane; i < n * K; i += kWave) {
            const int j = i / K, k = i - j * K;
            const long long id = group_ids[j];
            if (id >= 0) tile[j * RS + k] = a.emb[id * K + k];
        }
    }
    __syncthreads();                                                 // the tile is whole

    if (lane < n) {
        float s = -INFINITY;
        if (listed) {
            const float *q = a.queries + (p0 + lane) / a.M * K;
            const float *v = tile + lane * RS;
            const unsigned int *r = ranks + lane * RS;
            const long T = a.per_column ? table_size(a.N) : 0;       // column k reads code book k
            float acc = 0.0f, sum = 0.0f;
#pragma unroll 8
            for (int k = 0; k < K; ++k) {
                const float vk = !kRecords ? v[k] : (zero_row ? 0.0f : a.table[k * T + r[k]]);
                acc = __fmaf_rn(q[k], vk, acc);
                if (kCosine) sum = __fadd_rn(sum, __fmul_rn(vk, vk));
            }
            s = kCosine ? __fdiv_rn(acc, __fadd_rn(1e-8f, sqrtf(sum))) : acc;
        }
        a.out[p0 + lane] = s;
    }
    if (st && lane == 0 && a.status) atomicOr(a.status, st);
}

// What both calls take alike, before any device work.
int scores_check(const char *who, int64_t V, int32_t K, int64_t Q, int64_t M, int32_t metric) {
    VBQ_REQUIRE(V >= 1 && K >= 1 && Q >= 0 && M >= 0, VBQ_ERR_INVALID_ARGUMENT,
                "%s: bad sizes V=%lld K=%d Q=%lld M=%lld (need V >= 1, K >= 1, Q >= 0, M >= 0)", who, (long long)V, K, (long long)Q,
                (long long)M);
    VBQ_REQUIRE(metric == 0 || metric == 1, VBQ_ERR_INVALID_ARGUMENT, "%s: metric %d is neither 0 (dot) nor 1 (cosine)", who,
                metric);
    return VBQ_OK;
}

// The group of a call: the largest whose LDS stays within the target, else the smallest if it fits at all.  Sets G and RS;
// *lds gets the bytes.  Then the grid: one workgroup per group.
int scores_plan(const char *who, ScoresArgs &a, int64_t n_words, int64_t Q, int64_t M, size_t *lds) {
    a.RS = a.K | 1;
    a.G = 0;
    for (int G = kScoresMaxGroup; G >= kScoresMinGroup && !a.G; G >>= 1) {
        *lds = scores_lds_bytes(G, a.RS, n_words);
        if (*lds <= (G > kScoresMinGroup ? kScoresLdsTarget : kScoresLdsLimit)) a.G = G;
    }
    VBQ_REQUIRE(a.G, VBQ_ERR_UNSUPPORTED,
                "%s: K = %d (%lld words per record) needs %zu bytes of LDS at the smallest group of %d pairs, the limit is %zu "
                "(every K <= %d fits); decode the rows and reduce them instead", who, a.K, (long long)n_words, *lds, kScoresMinGroup,
                kScoresLdsLimit, kScoresAlwaysK);
    VBQ_REQUIRE(M == 0 || Q <= kScoresMaxGroups * a.G / M, VBQ_ERR_INVALID_ARGUMENT,
                "%s: Q * M = %lld * %lld pairs exceed the grid limit of %lld groups of %d pairs", who, (long long)Q, (long long)M,
                (long long)kScoresMaxGroups, a.G);
    return VBQ_OK;
}

template <bool kRecords, bool kCosine>
int scores_launch_as(const char *who, const ScoresArgs &a, size_t lds, hipStream_t st) {
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(k_scores<kRecords, kCosine>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
        (void)hipGetLastError();                                     // the launch below reports what is wrong, if anything
    const unsigned grid = (unsigned)((a.P + a.G - 1) / a.G);
    hipLaunchKernelGGL((k_scores<kRecords, kCosine>), dim3(grid), dim3(kWave), lds, st, a);
    VBQ_CHECK_LAUNCH(who);
    return VBQ_OK;
}

template <bool kRecords>
int scores_launch(const char *who, const ScoresArgs &a, int32_t metric, size_t lds, hipStream_t st) {
    return metric ? scores_launch_as<kRecords, true>(who, a, lds, st) : scores_launch_as<kRecords, false>(who, a, lds, st);
}

}  // namespace
}  // namespace vbq

#pragma GCC visibility push(default)
extern "C" int vbqx_records_scores_f32(const uint32_t *d_words, int64_t n_rows, int32_t K, int32_t N, int32_t total_bits,
                                       const float *d_table_sorted, int32_t n_tables, const float *d_queries, int64_t Q,
                                       const int64_t *d_ids, int64_t M, int32_t metric, float *d_out, uint32_t *d_status,
                                       void *stream) {
    using namespace vbq;
    const char *who = "vbqx_records_scores_f32";
    VBQ_REQUIRE(K >= 1 && N >= 1 && N <= kRecordsMaxN, VBQ_ERR_INVALID_ARGUMENT, "%s: bad sizes K=%d N=%d (need K >= 1, 1 <= N <= 10)",
                who, K, N);
    if (int rc = record_check_total_bits(who, K, N, total_bits)) return rc;
    VBQ_REQUIRE(n_tables == 1 || n_tables == K, VBQ_ERR_INVALID_ARGUMENT, "%s: n_tables = %d is neither 1 nor K = %d", who,
                n_tables, K);
    if (int rc = scores_check(who, n_rows, K, Q, M, metric)) return rc;
    int64_t n_words = 0;
    if (int rc = record_check_words(who, K, N, total_bits, &n_words)) return rc;
    ScoresArgs a = {};
    a.K = K;
    size_t lds = 0;
    if (int rc = scores_plan(who, a, n_words, Q, M, &lds)) return rc;
    if (Q == 0 || M == 0) return VBQ_OK;
    VBQ_REQUIRE(d_words && d_table_sorted && d_queries && d_ids && d_out, VBQ_ERR_INVALID_ARGUMENT, "%s: null pointer argument",
                who);
    a.words = d_words;
    a.table = d_table_sorted;
    a.V = (long)n_rows;
    a.N = N;
    a.total_bits = total_bits;
    a.n_words = (int)n_words;
    a.per_column = n_tables > 1;
    a.queries = d_queries;
    a.ids = reinterpret_cast<const long long *>(d_ids);
    a.P = (long)(Q * M);
    a.M = (long)M;
    a.out = d_out;
    a.status = d_status;
    return scores_launch<true>(who, a, metric, lds, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int vbqx_scores_f32(const float *d_emb, int64_t V, int32_t K, const float *d_queries, int64_t Q, const int64_t *d_ids,
                               int64_t M, int32_t metric, float *d_out, uint32_t *d_status, void *stream) {
    using namespace vbq;
    const char *who = "vbqx_scores_f32";
    if (int rc = scores_check(who, V, K, Q, M, metric)) return rc;
    ScoresArgs a = {};
    a.K = K;
    size_t lds = 0;
    if (int rc = scores_plan(who, a, 0, Q, M, &lds)) return rc;
    if (Q == 0 || M == 0) return VBQ_OK;
    VBQ_REQUIRE(d_emb && d_queries && d_ids && d_out, VBQ_ERR_INVALID_ARGUMENT, "%s: null pointer argument", who);
    a.emb = d_emb;
    a.V = (long)V;
    a.N = 1;
    a.queries = d_queries;
    a.ids = reinterpret_cast<const long long *>(d_ids);
    a.P = (long)(Q * M);
    a.M = (long)M;
    a.out = d_out;
    a.status = d_status;
    return scores_launch<false>(who, a, metric, lds, reinterpret_cast<hipStream_t>(stream));
}
#pragma GCC visibility pop
