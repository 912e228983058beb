// Wave-interleaved rANS: the coder of the compact latent file (vbq_amd/bitstream.py, magic "VBQc"; format: include/vbq.h,
// vbq_rans_il_encode_u16).  Same coder constants as vbq_rans.hip (32-bit state, start state 2^16, 16-bit renormalisation
// words, 15 probability bits), another layout: the S * n symbols of all streams in stream-major order are cut into parts of
// `part` symbols, and the 64 lanes of ONE wave code a part together -- in every step lane l owns the l-th of 64 consecutive
// symbols, and the words the lanes emit / take in a step lie next to each other in ascending lane order.  A part costs 128
// state words however long it is, where a segment of vbq_rans.hip costs 2 state words and a 2-byte size per 1024 symbols.
//
// A part may start and end inside a stream.  A run is a stretch of the part inside one stream: the tables of that stream
// are staged into LDS at the start of every run, and the lane states carry on from run to run.
//
// The coder over one part is vbq_rans_il_common.h's; the kernels here give it the parts of ONE tensor.
//
//   k_il_encode<false>  the encoder's state machine counting words only -> sizes u32 [P]
//   k_il_encode<true>   the same, writing the words backwards from off + size so that the part ends exactly at off
//   k_il_decode         untrusted words / sizes / offsets -> indices; what is wrong is reported in *status
#include "vbq_rans_il_common.h"

namespace vbq {
namespace {

// One wave per part of the one tensor: part p is the symbols [p * part, (p + 1) * part) of the `total`, the streams lie back
// to back (stride n) and stream s has row s of freq.  The coder itself is il_encode_part (vbq_rans_il_common.h).
template <bool kWrite>
__global__ void __launch_bounds__(kLanes)
k_il_encode(const uint16_t *__restrict__ idx, long n, long total, int T, int part, const uint16_t *__restrict__ freq,
            const uint32_t *__restrict__ sizes_in, const int64_t *__restrict__ offs, long n_words,
            uint16_t *__restrict__ payload, uint32_t *__restrict__ sizes_out) {
    __shared__ uint32_t fc_l[2048];
    const long p = blockIdx.x;
    const long a = p * (long)part;
    const long b = a + part < total ? a + part : total;
    long k0 = 0, off = 0;
    if (kWrite) {
        k0 = sizes_in[p], off = offs[p];
        // (sizes and offsets are the caller's own, from k_il_encode<false> and a scan; checked for memory safety only)
        if (k0 < kStateWords || off < 0 || off > n_words - k0) return;
    }
    il_encode_part<kWrite>(idx, n, n, a, b, T, freq, nullptr, payload, off, k0, kWrite ? nullptr : sizes_out + p, fc_l);
}

// Untrusted input: sizes, offsets and words may come from a damaged or foreign file.  Every read stays inside the part's
// [off, off + size), which is checked against [0, n_words) first; every symbol written is below T.  *status: bit 0 a part
// size outside [128, m + 128]; bit 1 a part ran out of words; bit 2 words left over or a final state other than 2^16; bit 3
// an invalid frequency row; bit 4 a part outside the payload, or the last part not ending at n_words (the sizes do not add
// up to n_words).  A part with any bit set decodes to zeros.  The decoder itself is il_decode_part (vbq_rans_il_common.h).
__global__ void __launch_bounds__(kLanes)
k_il_decode(const uint16_t *__restrict__ payload, long n_words, const uint32_t *__restrict__ sizes,
            const int64_t *__restrict__ offs, long P, long n, long total, int T, int part, const uint16_t *__restrict__ freq,
            uint16_t *__restrict__ idx, uint32_t *__restrict__ status) {
    __shared__ uint32_t fc_l[2048];
    __shared__ uint16_t c_l[2048 + 2];
    __shared__ uint16_t start[(1 << kPB) / 16];
    const long p = blockIdx.x;
    const long a = p * (long)part;
    const long b = a + part < total ? a + part : total;
    const long k0 = sizes[p], off = offs[p];
    unsigned bad = 0;
    if (k0 < kStateWords || k0 > (b - a) + kStateWords) bad |= 1u;
    if (off < 0 || off > n_words - k0 || (p == P - 1 && off + k0 != n_words)) bad |= 16u;
    if (!bad) bad = il_decode_part(payload + off, k0, idx, n, n, a, b, T, freq, fc_l, c_l, start);
    if (bad) {
        il_zero_part(idx, n, n, a, b);
        if (status && threadIdx.x == 0) atomicOr(status, bad);
    }
}

int check_il(const char *who, int64_t n_streams, int64_t n, int32_t N, int32_t part, int64_t *P) {
    VBQ_REQUIRE(n_streams >= 0 && n >= 0 && N >= 1 && N <= 10 && part >= 1 && part <= (1 << 24), VBQ_ERR_INVALID_ARGUMENT,
                "%s: bad sizes n_streams=%lld n=%lld N=%d part=%d", who, (long long)n_streams, (long long)n, N, part);
    VBQ_REQUIRE(n == 0 || n_streams <= (INT64_MAX >> 2) / n, VBQ_ERR_INVALID_ARGUMENT, "%s: %lld streams of %lld symbols are too many",
                who, (long long)n_streams, (long long)n);
    *P = (n_streams * n + part - 1) / part;
    VBQ_REQUIRE(*P <= INT32_MAX, VBQ_ERR_INVALID_ARGUMENT, "%s: %lld parts are too many", who, (long long)*P);
    return VBQ_OK;
}

}  // namespace
}  // namespace vbq

extern "C" int vbq_rans_il_sizes_u16(const uint16_t *d_idx, int64_t n_streams, int64_t n, int32_t N, int32_t part,
                                     const uint16_t *d_freq, uint32_t *d_sizes, void *stream) {
    using namespace vbq;
    int64_t P = 0;
    if (int r = check_il("vbq_rans_il_sizes_u16", n_streams, n, N, part, &P)) return r;
    if (P == 0) return VBQ_OK;
    VBQ_REQUIRE(d_idx && d_freq && d_sizes, VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_il_sizes_u16: null pointer argument");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_il_encode<false>), dim3((unsigned)P), dim3(kLanes), 0,
                       reinterpret_cast<hipStream_t>(stream), d_idx, (long)n, (long)(n_streams * n), table_size(N), (int)part,
                       d_freq, nullptr, nullptr, 0L, nullptr, d_sizes);
    VBQ_CHECK_LAUNCH("rans_il_sizes");
    return VBQ_OK;
}

extern "C" int vbq_rans_il_encode_u16(const uint16_t *d_idx, int64_t n_streams, int64_t n, int32_t N, int32_t part,
                                      const uint16_t *d_freq, const uint32_t *d_sizes, const int64_t *d_offsets,
                                      uint16_t *d_payload, int64_t n_words, void *stream) {
    using namespace vbq;
    int64_t P = 0;
    if (int r = check_il("vbq_rans_il_encode_u16", n_streams, n, N, part, &P)) return r;
    VBQ_REQUIRE(n_words >= 0, VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_il_encode_u16: bad sizes n_words=%lld", (long long)n_words);
    if (P == 0) return VBQ_OK;
    VBQ_REQUIRE(d_idx && d_freq && d_sizes && d_offsets && d_payload, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_il_encode_u16: null pointer argument");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_il_encode<true>), dim3((unsigned)P), dim3(kLanes), 0,
                       reinterpret_cast<hipStream_t>(stream), d_idx, (long)n, (long)(n_streams * n), table_size(N), (int)part,
                       d_freq, d_sizes, d_offsets, (long)n_words, d_payload, nullptr);
    VBQ_CHECK_LAUNCH("rans_il_encode");
    return VBQ_OK;
}

extern "C" int vbq_rans_il_decode_u16(const uint16_t *d_payload, int64_t n_words, const uint32_t *d_sizes,
                                      const int64_t *d_offsets, int64_t n_streams, int64_t n, int32_t N, int32_t part,
                                      const uint16_t *d_freq, uint16_t *d_idx, uint32_t *d_status, void *stream) {
    using namespace vbq;
    int64_t P = 0;
    if (int r = check_il("vbq_rans_il_decode_u16", n_streams, n, N, part, &P)) return r;
    VBQ_REQUIRE(n_words >= 0, VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_il_decode_u16: bad sizes n_words=%lld", (long long)n_words);
    if (P == 0) return VBQ_OK;
    VBQ_REQUIRE(d_sizes && d_offsets && d_freq && d_idx, VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_il_decode_u16: null pointer argument");
    VBQ_REQUIRE(n_words == 0 || d_payload, VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_il_decode_u16: null d_payload");
    hipLaunchKernelGGL(k_il_decode, dim3((unsigned)P), dim3(kLanes), 0, reinterpret_cast<hipStream_t>(stream), d_payload,
                       (long)n_words, d_sizes, d_offsets, (long)P, (long)n, (long)(n_streams * n), table_size(N), (int)part,
                       d_freq, d_idx, d_status);
    VBQ_CHECK_LAUNCH("rans_il_decode");
    return VBQ_OK;
}
