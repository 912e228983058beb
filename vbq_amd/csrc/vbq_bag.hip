// Pooled rows ("embedding bags"): the sum, mean or max of a short list of rows per output row, without the [n_ids, K] matrix
// of the rows in between.  The rows come either from fixed-size records ("VBQr", vbq_records.hip) or from a dense [V, K] f32
// matrix.  The semantics (entry kinds, the order of the additions, the max's tie rule, damaged records, damaged offsets) are
// stated in include/vbq.h, "Pooled rows".
//   k_bag<records, table in LDS>  one wave per bag, the grid strides over the bags.  The ids of a bag are read 64 at a time
//                    (one coalesced load) and handed out wave-uniformly; per counted entry the record is staged in LDS with one
//                    coalesced copy and decoded by the unpack's scan (decode_record of vbq_records_common.h), whose emit looks
//                    the code point up and folds it into the accumulator of coordinate k.  decode_record gives lane l the
//                    coordinates l, l + 64, ...: every accumulator has one owner, so the fold needs no atomics and no barrier
//                    beyond the two that guard the image.  The accumulators live in LDS (K is not bounded by registers), twice:
//                    an entry folds `cur` into `nxt` and the two swap when the record passed its checks -- what a record is
//                    worth is known only after its scan, and a rejected one folds a row of zeros into `cur` instead.  The
//                    dense loader is the same fold with row[k] in place of the decoded value: the two sources agree bit for bit.
// Every operation of the fold is a separately rounded f32 operation (__fadd_rn, __fmul_rn, __fdiv_rn): NumPy float32
// reproduces it.  Record words are untrusted exactly as in k_records_unpack; the offsets are clamped into [0, n_ids] before
// anything is read through them.  gfx950 / ROCm only.
#include "vbq_records_common.h"

namespace vbq {
namespace {

constexpr int kBagWgPerCu = 16;                  // single-wave workgroups the bag loop's grid is sized for (the unpack's)
constexpr int64_t kBagLdsTableReuse = 4;         // the unpack's rule: coordinates decoded per table entry loaded
constexpr size_t kBagLdsLimit = 160 * 1024;      // per CU
// Every K up to here fits whatever N, total_bits and n_tables: ceil(14 K / 32) + 2 K <= 40960 words (N = 10, total_bits = 10 K;
// the code book goes to LDS only where it fits beside them).  The dense source fits up to K = 20480.
constexpr int kBagAlwaysK = 16804;

enum : unsigned int { kBagBadOffsets = 16u };    // next to kUnpackBad*: a bag's range left [0, n_ids] or ran backwards

enum { kBagSum = 0, kBagMean = 1, kBagMax = 2 };

struct BagArgs {
    const float *emb;                 // the dense source [V][K]
    const unsigned int *words;        // the record source [V][n_words]
    const float *table;
    long V;
    int K, N, total_bits, n_words, per_column;
    const long long *ids;
    long n_ids;
    const long long *offsets;
    long n_bags;
    const float *weights;
    int mode;
    float *out;
    unsigned int *status;
};

// LDS of k_bag in bytes: the staged record, the accumulators twice, the one code book.
size_t bag_lds_bytes(int K, int64_t n_words, int table_entries) {
    return 4 * ((size_t)n_words + 2 * (size_t)K + (size_t)table_entries);
}

// A value every lane holds alike, in scalar registers: the branches on it are uniform for the compiler too.
__device__ __forceinline__ long wave_uniform(long long v) {
    const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)v);
    const unsigned int hi = __builtin_amdgcn_readfirstlane((unsigned int)((unsigned long long)v >> 32));
    return (long)(((unsigned long long)hi << 32) | lo);
}

// One entry's coordinate folded into the accumulator: include/vbq.h, "Pooled rows".
__device__ __forceinline__ float bag_fold(float acc, float v, float w, bool weighted, bool first, int mode) {
    if (mode == kBagMax) return (first || v > acc) ? v : acc;
    return __fadd_rn(acc, weighted ? __fmul_rn(w, v) : v);
}

template <bool kRecords, bool kTableInLds>
__global__ void __launch_bounds__(kWave)
k_bag(const BagArgs a) {
    extern __shared__ unsigned int img[];
    const int lane = threadIdx.x;
    const int K = a.K, n_words = a.n_words, mode = a.mode;
    const int T = table_size(a.N);
    const bool weighted = a.weights != nullptr;
    float *cur = reinterpret_cast<float *>(img + n_words);
    float *nxt = cur + K;
    const float *tab = a.table;
    if (kRecords && kTableInLds) {
        float *lt = nxt + K;
        for (int i = lane; i < T; i += kWave) lt[i] = a.table[i];
        tab = lt;
    }
    unsigned int st = 0u;                                            // wave-uniform
    for (long b = blockIdx.x; b < a.n_bags; b += gridDim.x) {
        long begin = wave_uniform(a.offsets[b]), end = wave_uniform(a.offsets[b + 1]);
        if (begin < 0 || begin > a.n_ids || end < 0 || end > a.n_ids || begin > end) {
            st |= kBagBadOffsets;
            begin = begin < 0 ? 0 : (begin > a.n_ids ? a.n_ids : begin);
            end = end < 0 ? 0 : (end > a.n_ids ? a.n_ids : end);
            if (begin > end) end = begin;
        }
        for (int k = lane; k < K; k += kWave) cur[k] = 0.0f;
        long count = 0;
        for (long c0 = begin; c0 < end; c0 += kWave) {
            const long rest = end - c0;
            const int chunk = rest < kWave ? (int)rest : kWave;
            long long my_id = -1;
            float my_w = 0.0f;
            if (lane < chunk) {
                my_id = a.ids[c0 + lane];
                if (weighted) my_w = a.weights[c0 + lane];
            }
            for (int j = 0; j < chunk; ++j) {
                const long id = wave_uniform(__shfl(my_id, j, kWave));
                if (id < 0) continue;                                // padding
                if (id >= a.V) {
                    st |= kUnpackBadRow;
                    continue;
                }
                const float w = __shfl(my_w, j, kWave);
                const bool first = count == 0;
                ++count;
                if (kRecords) {
                    __syncthreads();                                 // the previous entry's reads of the image are done
                    const unsigned int *rec = a.words + id * n_words;
                    for (int i = lane; i < n_words; i += kWave) img[i] = rec[i];
                    __syncthreads();
                    const unsigned int bad = decode_record(img, n_words, K, a.N, a.total_bits, lane, [&](int k, unsigned int q) {
                        nxt[k] = bag_fold(cur[k], tab[(a.per_column ? (long)k * T : 0L) + q], w, weighted, first, mode);
                    });
                    if (bad) {                                       // wave-uniform: a rejected record is a row of zeros
                        st |= bad;
                        for (int k = lane; k < K; k += kWave) cur[k] = bag_fold(cur[k], 0.0f, w, weighted, first, mode);
                    } else {
                        float *t = cur;
                        cur = nxt;
                        nxt = t;
                    }
                } else {
                    const float *row = a.emb + id * K;
                    for (int k = lane; k < K; k += kWave) cur[k] = bag_fold(cur[k], row[k], w, weighted, first, mode);
                }
            }
        }
        const float n = (float)count;
        float *row_out = a.out + b * K;
        for (int k = lane; k < K; k += kWave) {
            const float s = cur[k];
            row_out[k] = (mode == kBagMean && count > 0) ? __fdiv_rn(s, n) : s;
        }
    }
    if (st && lane == 0 && a.status) atomicOr(a.status, st);
}

// What both calls take alike, before any device work.
int bag_check(const char *who, int64_t V, int32_t K, int64_t n_ids, int64_t n_bags, const float *d_weights, int32_t mode) {
    VBQ_REQUIRE(V >= 1 && K >= 1 && n_ids >= 0 && n_bags >= 0, VBQ_ERR_INVALID_ARGUMENT,
                "%s: bad sizes V=%lld K=%d n_ids=%lld n_bags=%lld (need V >= 1, K >= 1, n_ids >= 0, n_bags >= 0)", who, (long long)V,
                K, (long long)n_ids, (long long)n_bags);
    VBQ_REQUIRE(mode >= kBagSum && mode <= kBagMax, VBQ_ERR_INVALID_ARGUMENT, "%s: mode %d is none of 0 (sum), 1 (mean), 2 (max)", who,
                mode);
    VBQ_REQUIRE(!d_weights || mode == kBagSum, VBQ_ERR_INVALID_ARGUMENT, "%s: weights go with mode 0 (sum) only, not mode %d", who,
                mode);
    return VBQ_OK;
}

int bag_check_lds(const char *who, int32_t K, int64_t n_words) {
    const size_t need = bag_lds_bytes(K, n_words, 0);
    VBQ_REQUIRE(need <= kBagLdsLimit, VBQ_ERR_UNSUPPORTED,
                "%s: K = %d (%lld words per record) needs %zu bytes of LDS for one bag, the limit is %zu (every K <= %d fits); "
                "decode the rows and reduce them instead", who, K, (long long)n_words, need, kBagLdsLimit, kBagAlwaysK);
    return VBQ_OK;
}

template <bool kRecords, bool kTableInLds>
int bag_launch(const char *who, const BagArgs &a, unsigned grid, size_t lds, hipStream_t st) {
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(k_bag<kRecords, kTableInLds>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
        (void)hipGetLastError();                                     // the launch below reports what is wrong, if anything
    hipLaunchKernelGGL((k_bag<kRecords, kTableInLds>), dim3(grid), dim3(kWave), lds, st, a);
    VBQ_CHECK_LAUNCH(who);
    return VBQ_OK;
}

unsigned bag_grid(int64_t n_bags) {
    const int64_t resident = (int64_t)num_cus() * kBagWgPerCu;
    return (unsigned)(n_bags < resident ? n_bags : resident);
}

}  // namespace
}  // namespace vbq

extern "C" int vbq_records_bag_f32(const uint32_t *d_words, int64_t n_rows, int32_t K, int32_t N, int32_t total_bits,
                                   const float *d_table_sorted, int32_t n_tables, const int64_t *d_ids, int64_t n_ids,
                                   const int64_t *d_offsets, int64_t n_bags, const float *d_weights, int32_t mode, float *d_out,
                                   uint32_t *d_status, void *stream) {
    using namespace vbq;
    const char *who = "vbq_records_bag_f32";
    VBQ_REQUIRE(K >= 1 && N >= 1 && N <= kRecordsMaxN, VBQ_ERR_INVALID_ARGUMENT, "%s: bad sizes K=%d N=%d (need K >= 1, 1 <= N <= 10)",
                who, K, N);
    if (int rc = record_check_total_bits(who, K, N, total_bits)) return rc;
    VBQ_REQUIRE(n_tables == 1 || n_tables == K, VBQ_ERR_INVALID_ARGUMENT, "%s: n_tables = %d is neither 1 nor K = %d", who,
                n_tables, K);
    if (int rc = bag_check(who, n_rows, K, n_ids, n_bags, d_weights, mode)) return rc;
    int64_t n_words = 0;
    if (int rc = record_check_words(who, K, N, total_bits, &n_words)) return rc;
    if (int rc = bag_check_lds(who, K, n_words)) return rc;
    if (n_bags == 0) return VBQ_OK;
    VBQ_REQUIRE(d_words && d_table_sorted && d_offsets && d_out && (d_ids || n_ids == 0), VBQ_ERR_INVALID_ARGUMENT,
                "%s: null pointer argument", who);
    BagArgs a = {};
    a.words = d_words;
    a.table = d_table_sorted;
    a.V = (long)n_rows;
    a.K = K;
    a.N = N;
    a.total_bits = total_bits;
    a.n_words = (int)n_words;
    a.per_column = n_tables > 1;
    a.ids = reinterpret_cast<const long long *>(d_ids);
    a.n_ids = (long)n_ids;
    a.offsets = reinterpret_cast<const long long *>(d_offsets);
    a.n_bags = (long)n_bags;
    a.weights = d_weights;
    a.mode = mode;
    a.out = d_out;
    a.status = d_status;
    const unsigned grid = bag_grid(n_bags);
    const int T = table_size(N);
    const int64_t per_wg = (n_ids + grid - 1) / grid;                // entries a workgroup decodes, on average
    const bool lds_table = n_tables == 1 && per_wg * K >= kBagLdsTableReuse * T && bag_lds_bytes(K, n_words, T) <= kBagLdsLimit;
    const size_t lds = bag_lds_bytes(K, n_words, lds_table ? T : 0);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return lds_table ? bag_launch<true, true>(who, a, grid, lds, st) : bag_launch<true, false>(who, a, grid, lds, st);
}

extern "C" int vbq_bag_f32(const float *d_emb, int64_t V, int32_t K, const int64_t *d_ids, int64_t n_ids, const int64_t *d_offsets,
                           int64_t n_bags, const float *d_weights, int32_t mode, float *d_out, uint32_t *d_status, void *stream) {
    using namespace vbq;
    const char *who = "vbq_bag_f32";
    if (int rc = bag_check(who, V, K, n_ids, n_bags, d_weights, mode)) return rc;
    if (int rc = bag_check_lds(who, K, 0)) return rc;
    if (n_bags == 0) return VBQ_OK;
    VBQ_REQUIRE(d_emb && d_offsets && d_out && (d_ids || n_ids == 0), VBQ_ERR_INVALID_ARGUMENT, "%s: null pointer argument", who);
    BagArgs a = {};
    a.emb = d_emb;
    a.V = (long)V;
    a.K = K;
    a.N = 1;
    a.ids = reinterpret_cast<const long long *>(d_ids);
    a.n_ids = (long)n_ids;
    a.offsets = reinterpret_cast<const long long *>(d_offsets);
    a.n_bags = (long)n_bags;
    a.weights = d_weights;
    a.mode = mode;
    a.out = d_out;
    a.status = d_status;
    return bag_launch<false, false>(who, a, bag_grid(n_bags), bag_lds_bytes(K, 0, 0), reinterpret_cast<hipStream_t>(stream));
}
