// What the readers of fixed-size records share -- vbq_records.hip (pack, unpack) and vbq_topk.hip (the search that scores rows
// straight from their records): the limits, the unpack's status bits, the record length with its size checks, and the decode
// of ONE record by one wave.  Format ("VBQr"): include/vbq.h.  The decode is the format's untrusted-input boundary: no read
// leaves the staged image, and a record that fails a check is reported in the returned bits.  What a kernel does with a
// decoded rank, how it zeroes a rejected row and where it reports the bits is each kernel's own business; so are staging the
// image and the code book, and the packer's put_bits and status bits.
#pragma once
#include "vbq_common.h"

namespace vbq {

constexpr int kRecordsMaxN = 10;
constexpr int64_t kRecordsMaxWords = 8192;       // 32 KiB: the LDS image of one record

enum : unsigned int {
    kUnpackBadLength = 1u,     // a length field > N
    kUnpackBadSum = 2u,        // the lengths of a record do not add up to total_bits
    kUnpackBadPadding = 4u,    // non-zero padding
    kUnpackBadRow = 8u         // a row id outside [0, n_rows)
};

__host__ __device__ constexpr int length_field_bits(int N) { return N >= 8 ? 4 : (N >= 4 ? 3 : (N >= 2 ? 2 : 1)); }

// Inclusive prefix sum over the 64 lanes of the wave.
__device__ __forceinline__ int wave_inclusive_sum(int v, int lane) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int u = __shfl_up(v, d, kWave);
        if (lane >= d) v += u;
    }
    return v;
}

// `nbits` (0..31) bits of the image at bit `pos`, through a window of two words; words outside [0, n_words) read as zero.
__device__ __forceinline__ unsigned int get_bits(const unsigned int *img, int n_words, int pos, int nbits) {
    const int w = pos >> 5, sh = pos & 31;
    const unsigned long long lo = w < n_words ? img[w] : 0u;
    const unsigned long long hi = w + 1 < n_words ? img[w + 1] : 0u;
    return (unsigned int)(((hi << 32) | lo) >> sh) & ((1u << nbits) - 1u);
}

// One record, staged in `img[n_words]`, decoded by the 64 lanes of a wave: the K length fields at W bits, their prefix sum
// carried over the chunks of 64 coordinates, every code through the two-word window, emit(k, rank) for every k < K (lane ->
// k within a chunk).  Returns the wave-uniform kUnpackBad* bits of the record; when they are not 0 the ranks emitted are
// in [0, T) but mean nothing, and the caller zeroes its row.
template <typename Emit>
__device__ __forceinline__ unsigned int decode_record(const unsigned int *img, int n_words, int K, int N, int total_bits, int lane,
                                                      Emit emit) {
    const int W = length_field_bits(N);
    const int code0 = K * W, end = code0 + total_bits;
    unsigned int bad = 0u;
    int carry = 0;
    for (int base = 0; base < K; base += kWave) {
        const int k = base + lane;
        int n = 0;
        if (k < K) {
            n = (int)get_bits(img, n_words, k * W, W);
            if (n > N) { bad |= kUnpackBadLength; n = 0; }
        }
        const int incl = wave_inclusive_sum(n, lane);
        const int off = carry + incl - n;
        carry += __shfl(incl, kWave - 1, kWave);
        if (k < K) {
            if (off + n > total_bits) n = 0;                         // over the budget: rejected below; read no code
            const unsigned int j = get_bits(img, n_words, code0 + off, n);
            emit(k, ((2u * j + 1u) << (N - n)) - 1u);                // < T for every n <= N and j < 2^n
        }
    }
    if (carry != total_bits) bad |= kUnpackBadSum;
    if ((end & 31) && (img[n_words - 1] >> (end & 31))) bad |= kUnpackBadPadding;
    return bad | (__any(bad & kUnpackBadLength) ? kUnpackBadLength : 0u);
}

// 32-bit words of one record: K length fields, total_bits of codes, zero padding.
static inline int64_t record_words(int32_t K, int32_t N, int32_t total_bits) {
    return ((int64_t)K * length_field_bits(N) + total_bits + 31) / 32;
}

static inline bool record_total_bits_ok(int32_t K, int32_t N, int32_t total_bits) {
    return total_bits >= 0 && (int64_t)total_bits <= (int64_t)K * N;
}

// The size checks of an entry point that takes records, after its own check of K and N (whose message names the entry
// point's other sizes too): total_bits, then the record length into *n_words and its limit.  The search raises its other
// argument errors between the two, so they are two calls.
static inline int record_check_total_bits(const char *who, int32_t K, int32_t N, int32_t total_bits) {
    VBQ_REQUIRE(record_total_bits_ok(K, N, total_bits), VBQ_ERR_INVALID_ARGUMENT, "%s: total_bits %d outside [0, K*N = %lld]", who,
                total_bits, (long long)K * N);
    return VBQ_OK;
}

static inline int record_check_words(const char *who, int32_t K, int32_t N, int32_t total_bits, int64_t *n_words) {
    *n_words = record_words(K, N, total_bits);
    VBQ_REQUIRE(*n_words <= kRecordsMaxWords, VBQ_ERR_UNSUPPORTED, "%s: a record of %lld words exceeds the limit of %lld", who,
                (long long)*n_words, (long long)kRecordsMaxWords);
    return VBQ_OK;
}

}  // namespace vbq
