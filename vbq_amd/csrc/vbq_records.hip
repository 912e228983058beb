// Fixed-size records of rows quantized to one bit budget (vbq_amd/bitstream.py, magic "VBQr"; the format is stated in
// include/vbq.h).  A record holds the K bit lengths of a row at W = bit_length(N) bits each, then the codes back to back, then
// zero padding up to a whole number of 32-bit words; every row of a file costs the same, so row r starts at word
// r * record_words and a lookup is one address computation and one short unpack.
//   k_records_pack    one wave per row: (n, j) from the rank index alone, a wave prefix sum of the lengths carried over the
//                     chunks of 64 coordinates, the fields OR-ed into an LDS image of the record, the image written with
//                     coalesced 4-byte stores.  A row whose lengths do not add up to total_bits, or with an index >= T, gets an
//                     all-zero record and a status bit.
//   k_records_unpack  one wave per requested row: the record staged in LDS, the same scan, every field read through a two-word
//                     window, (n, j) -> rank -> value (decode_record of vbq_records_common.h, which the search shares).  The record bytes are untrusted: no read leaves the LDS image, a row
//                     that fails a check decodes to zeros and sets a status bit.
// Workgroups are single waves, so the barriers between the phases of a row are wave-local and the row loop needs no
// agreement between waves.  gfx950 / ROCm only.
#include "vbq_records_common.h"

namespace vbq {
namespace {

constexpr int kRecordsWgPerCu = 16;              // single-wave workgroups the row loop's grid is sized for
// The one code book in LDS pays once a workgroup decodes this many coordinates per table entry it loads; below that (short
// lookups) the table is read through L2, where every workgroup shares it.
constexpr int64_t kRecordsLdsTableReuse = 4;

enum : unsigned int {
    kPackBadIndex = 1u,        // an index >= T
    kPackBadSum = 2u           // the lengths of a row do not add up to total_bits
};

// OR the low `nbits` (0..32 - 1) bits of `val` into the image at bit `pos`; the caller keeps pos + nbits inside the image.
__device__ __forceinline__ void put_bits(unsigned int *img, int pos, int nbits, unsigned int val) {
    if (nbits == 0) return;
    const int w = pos >> 5, sh = pos & 31;
    atomicOr(img + w, val << sh);
    if (sh + nbits > 32) atomicOr(img + w + 1, val >> (32 - sh));
}

__global__ void __launch_bounds__(kWave)
k_records_pack(const uint16_t *__restrict__ idx, long n_rows, int K, int N, int total_bits, int n_words,
               unsigned int *__restrict__ words, unsigned int *__restrict__ status) {
    extern __shared__ unsigned int img[];
    const int lane = threadIdx.x;
    const int W = length_field_bits(N), T = table_size(N);
    const int code0 = K * W;
    for (int i = lane; i < n_words; i += kWave) img[i] = 0u;
    __syncthreads();
    for (long r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const uint16_t *row = idx + r * K;
        unsigned int bad = 0u;
        int carry = 0;
        for (int base = 0; base < K; base += kWave) {
            const int k = base + lane;
            int n = 0;
            unsigned int j = 0u;
            if (k < K) {
                const unsigned int kk = (unsigned int)row[k] + 1u;
                if (kk > (unsigned int)T) bad |= kPackBadIndex;
                else {
                    n = N - __builtin_ctz(kk);
                    j = kk >> (N - n + 1);
                }
            }
            const int incl = wave_inclusive_sum(n, lane);
            const int off = carry + incl - n;
            carry += __shfl(incl, kWave - 1, kWave);
            if (k < K && off + n <= total_bits) {                    // a row over the budget is rejected below: write nothing
                put_bits(img, k * W, W, (unsigned int)n);            // outside the image
                put_bits(img, code0 + off, n, j);
            }
        }
        if (carry != total_bits) bad |= kPackBadSum;
        bad = __any(bad & kPackBadIndex) ? (bad | kPackBadIndex) : bad;
        __syncthreads();
        unsigned int *out = words + r * n_words;
        for (int i = lane; i < n_words; i += kWave) {
            out[i] = bad ? 0u : img[i];
            img[i] = 0u;                                             // the next row's image
        }
        if (bad && lane == 0 && status) atomicOr(status, bad);
        __syncthreads();
    }
}

template <bool kTableInLds>
__global__ void __launch_bounds__(kWave)
k_records_unpack(const unsigned int *__restrict__ words, long n_rows, int K, int N, int total_bits, int n_words,
                 const float *__restrict__ table, int per_column, const long long *__restrict__ row_ids, long n_out,
                 float *__restrict__ out_val, uint16_t *__restrict__ out_idx, unsigned int *__restrict__ status) {
    extern __shared__ unsigned int img[];
    const int lane = threadIdx.x;
    const int T = table_size(N);
    const float *tab = table;
    if (kTableInLds) {
        float *lt = reinterpret_cast<float *>(img + n_words);
        for (int i = lane; i < T; i += kWave) lt[i] = table[i];
        tab = lt;
    }
    for (long o = blockIdx.x; o < n_out; o += gridDim.x) {
        const long r = row_ids ? (long)row_ids[o] : o;
        const bool in_range = r >= 0 && r < n_rows;
        __syncthreads();                                             // the previous row's reads of the image are done
        if (in_range) {
            const unsigned int *rec = words + r * n_words;
            for (int i = lane; i < n_words; i += kWave) img[i] = rec[i];
        }
        __syncthreads();
        uint16_t *row_idx = out_idx + o * K;                         // used only where the output was asked for
        float *row_val = out_val + o * K;
        unsigned int bad = kUnpackBadRow;
        if (in_range)
            bad = decode_record(img, n_words, K, N, total_bits, lane, [&](int k, unsigned int q) {
                if (out_idx) row_idx[k] = (uint16_t)q;
                if (out_val) row_val[k] = tab[(per_column ? (long)k * T : 0L) + q];
            });
        if (bad) {                                                   // wave-uniform: a rejected row decodes to zeros
            for (int k = lane; k < K; k += kWave) {
                if (out_idx) row_idx[k] = 0;
                if (out_val) row_val[k] = 0.0f;
            }
            if (lane == 0 && status) atomicOr(status, bad);
        }
    }
}

// The sizes every entry point takes; *n_words gets the record length.
int records_check(const char *who, int64_t n_rows, int32_t K, int32_t N, int32_t total_bits, int64_t *n_words) {
    VBQ_REQUIRE(n_rows >= 0 && K >= 1 && N >= 1 && N <= kRecordsMaxN, VBQ_ERR_INVALID_ARGUMENT,
                "%s: bad sizes n_rows=%lld K=%d N=%d (need K >= 1, 1 <= N <= 10)", who, (long long)n_rows, K, N);
    if (int rc = record_check_total_bits(who, K, N, total_bits)) return rc;
    return record_check_words(who, K, N, total_bits, n_words);
}

unsigned records_grid(int64_t rows) {
    const int64_t resident = (int64_t)num_cus() * kRecordsWgPerCu;
    return (unsigned)(rows < resident ? rows : resident);
}

}  // namespace
}  // namespace vbq

extern "C" size_t vbq_records_words(int32_t K, int32_t N, int32_t total_bits) {
    using namespace vbq;
    if (K < 1 || N < 1 || N > kRecordsMaxN || !record_total_bits_ok(K, N, total_bits)) return 0;
    return (size_t)record_words(K, N, total_bits);
}

extern "C" int vbq_records_pack_u16(const uint16_t *d_idx, int64_t n_rows, int32_t K, int32_t N, int32_t total_bits,
                                    uint32_t *d_words, uint32_t *d_status, void *stream) {
    using namespace vbq;
    int64_t n_words = 0;
    if (int rc = records_check("vbq_records_pack_u16", n_rows, K, N, total_bits, &n_words)) return rc;
    if (n_rows == 0) return VBQ_OK;
    VBQ_REQUIRE(d_idx && d_words, VBQ_ERR_INVALID_ARGUMENT, "vbq_records_pack_u16: null pointer argument");
    hipLaunchKernelGGL(k_records_pack, dim3(records_grid(n_rows)), dim3(kWave), (size_t)n_words * 4,
                       reinterpret_cast<hipStream_t>(stream), d_idx, (long)n_rows, (int)K, (int)N, (int)total_bits, (int)n_words,
                       d_words, d_status);
    VBQ_CHECK_LAUNCH("records_pack");
    return VBQ_OK;
}

extern "C" int vbq_records_unpack_f32(const uint32_t *d_words, int64_t n_rows, int32_t K, int32_t N, int32_t total_bits,
                                      const float *d_table_sorted, int32_t n_tables, const int64_t *d_row_ids, int64_t n_sel,
                                      float *d_out_values, uint16_t *d_out_idx, uint32_t *d_status, void *stream) {
    using namespace vbq;
    int64_t n_words = 0;
    if (int rc = records_check("vbq_records_unpack_f32", n_rows, K, N, total_bits, &n_words)) return rc;
    VBQ_REQUIRE(n_tables == 1 || n_tables == K, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_records_unpack_f32: n_tables = %d is neither 1 nor K = %d", n_tables, K);
    VBQ_REQUIRE(n_sel >= 0, VBQ_ERR_INVALID_ARGUMENT, "vbq_records_unpack_f32: negative n_sel %lld", (long long)n_sel);
    const int64_t n_out = d_row_ids ? n_sel : n_rows;
    if (n_out == 0) return VBQ_OK;
    VBQ_REQUIRE(d_words && (d_table_sorted || !d_out_values), VBQ_ERR_INVALID_ARGUMENT,
                "vbq_records_unpack_f32: null pointer argument");
    const unsigned grid = records_grid(n_out);
    const int T = table_size(N);
    const int64_t per_wg = (n_out + grid - 1) / grid;
    const bool lds_table = d_out_values && n_tables == 1 && per_wg * K >= kRecordsLdsTableReuse * T;
    const size_t lds = (size_t)n_words * 4 + (lds_table ? (size_t)T * 4 : 0);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long *ids = reinterpret_cast<const long long *>(d_row_ids);
    if (lds_table)
        hipLaunchKernelGGL(k_records_unpack<true>, dim3(grid), dim3(kWave), lds, st, d_words, (long)n_rows, (int)K, (int)N,
                           (int)total_bits, (int)n_words, d_table_sorted, 0, ids, (long)n_out, d_out_values, d_out_idx, d_status);
    else
        hipLaunchKernelGGL(k_records_unpack<false>, dim3(grid), dim3(kWave), lds, st, d_words, (long)n_rows, (int)K, (int)N,
                           (int)total_bits, (int)n_words, d_table_sorted, (int)(n_tables > 1), ids, (long)n_out, d_out_values,
                           d_out_idx, d_status);
    VBQ_CHECK_LAUNCH("records_unpack");
    return VBQ_OK;
}
