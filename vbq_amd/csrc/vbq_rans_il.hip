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
//   k_il_encode<false>  the encoder's state machine counting words only -> sizes u32 [P]
//   k_il_encode<true>   the same, writing the words backwards from off + size so that the part ends exactly at off
//   k_il_decode         untrusted words / sizes / offsets -> indices; what is wrong is reported in *status
#include "vbq_rans_common.h"

namespace vbq {
namespace {

constexpr int kLanes = 64;                                       // the lane count of the FORMAT (and of the workgroup)
constexpr int kStateWords = 2 * kLanes;

// Inclusive prefix sum over the 64 lanes in six DPP adds, no LDS: row_shr 1, 2, 4, 8 scan the rows of 16 lanes (a lane without
// a source adds 0), row_bcast:15 adds the total of row 0 / 2 to row 1 / 3, row_bcast:31 the total of the first 32 lanes to the
// last 32.  (A scan by __shfl_up is six LDS-permute round trips per 64 symbols, and the staging runs once per run.)
__device__ __forceinline__ unsigned wave_incl_scan(unsigned v) {
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 into rows 1 and 3
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 into rows 2 and 3
    return v;
}

// The tables of one stream into LDS, 64 symbols per round (coalesced reads, conflict-free LDS writes; the prefix sum of a round
// is one wave scan plus the carry of the rounds before):
//   fc_l[sym] = f | c << 16       c = exclusive cumulative frequency
// and for the decoder (kDecode)
//   c_l[sym]  = c, c_l[T] = 2^15
//   start[b]  = the symbol whose slot range [c, c + f) holds slot 16 b, by a direct fill of the ranges: a lane fills the range
//               of its own symbol when that is short (f <= 64: at most 5 buckets); a long range -- the one symbol of a near-dead
//               channel that holds nearly all the mass -- is filled by the 64 lanes together.
// Returns whether the row is valid (it sums to 2^15 and no entry is above 2^15 - 1).  For an invalid row the tables are
// garbage but every write stayed inside them; the caller does not decode with them.
template <bool kDecode>
__device__ __forceinline__ bool stage_tables_il(const uint16_t *__restrict__ freq, int T, uint32_t *fc_l, uint16_t *c_l,
                                                uint16_t *start) {
    const int lane = threadIdx.x;
    __syncthreads();                                             // the previous run's reads of the tables are done
    unsigned carry = 0;
    bool big = false;
    for (int base = 0; base < T; base += kLanes) {
        const int i = base + lane;
        const unsigned f = i < T ? (unsigned)freq[i] : 0u;
        const unsigned incl = wave_incl_scan(f);
        const unsigned run = carry + incl - f;
        if (i < T) {
            fc_l[i] = f | (run << 16);
            if (kDecode) c_l[i] = (uint16_t)run;
        }
        if (kDecode) {
            big |= f >= (1u << kPB);
            const unsigned lim = 1u << kPB;                      // an invalid row may run past 2^15: no bucket beyond the table
            const bool wide = f > 64u;
            if (!wide) {
                const unsigned end = run + f < lim ? run + f : lim;
                for (unsigned b = (run + 15u) >> 4; 16u * b < end; ++b) start[b] = (uint16_t)i;
            }
            unsigned long long m = __ballot(wide);
            while (m) {                                          // wave-uniform
                const int src = __ffsll((long long)m) - 1;
                m &= m - 1;
                const unsigned r0 = __shfl(run, src, 64), f0 = __shfl(f, src, 64);
                const unsigned end = r0 + f0 < lim ? r0 + f0 : lim;
                for (unsigned b = ((r0 + 15u) >> 4) + lane; 16u * b < end; b += kLanes) start[b] = (uint16_t)(base + src);
            }
        }
        carry += __shfl(incl, 63, 64);
    }
    const bool ok = carry == (1u << kPB) && !__any(big);
    if (kDecode && lane == 0) c_l[T] = (uint16_t)(1u << kPB);    // > every slot: ends the decoder's walk below T
    __syncthreads();
    return ok;
}

// One wave per part.  Runs last to first, steps last to first; in a step every active lane renormalises (emitting at most
// one word) and encodes its symbol.  The words of a step go to [wp - cnt, wp) in ascending lane order: a lane's place is
// the number of emitting lanes below it (a wave ballot).  kWrite = false counts only.
template <bool kWrite>
__global__ void __launch_bounds__(kLanes)
k_il_encode(const uint16_t *__restrict__ idx, long n, long total, int T, int part, const uint16_t *__restrict__ freq,
            const uint32_t *__restrict__ sizes_in, const int64_t *__restrict__ offs, long n_words,
            uint16_t *__restrict__ payload, uint32_t *__restrict__ sizes_out) {
    __shared__ uint32_t fc_l[2048];
    const int lane = threadIdx.x;
    const long p = blockIdx.x;
    const long a = p * (long)part;
    const long b = a + part < total ? a + part : total;
    long lo = 0, wp = 0;                                         // the renormalisation words of the part: [lo, wp), written downwards
    if (kWrite) {
        const long k0 = sizes_in[p], off = offs[p];
        // (sizes and offsets are the caller's own, from k_il_encode<false> and a scan; checked for memory safety only)
        if (k0 < kStateWords || off < 0 || off > n_words - k0) return;
        lo = off + kStateWords;
        wp = off + k0;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned x = kRansL;
    unsigned count = 0;
    for (long s = (b - 1) / n; s >= a / n; --s) {                // stream of the run (wave-uniform)
        const long rs = s * n > a ? s * n : a;
        const long re = (s + 1) * n < b ? (s + 1) * n : b;
        const int len = (int)(re - rs);
        stage_tables_il<false>(freq + s * T, T, fc_l, nullptr, nullptr);
        const uint16_t *src = idx + rs;
        int t = (len - 1) / kLanes;
        unsigned nxt = t * kLanes + lane < len ? (unsigned)src[t * kLanes + lane] : 0u;
        for (; t >= 0; --t) {
            const bool active = t * kLanes + lane < len;
            const unsigned sym = nxt;
            if (t > 0) nxt = src[(t - 1) * kLanes + lane];       // a full step: the next symbol is on its way while this one is coded
            const unsigned fc = fc_l[sym < (unsigned)T ? sym : 0u];   // (an index outside the table: memory-safe)
            const unsigned f = fc & 0xffffu, c = fc >> 16;
            const bool emit = active && x >= (f << (32 - kPB));
            const unsigned long long m = __ballot(emit);
            const int cnt = __popcll(m);
            if (kWrite) {
                wp -= cnt;
                const long at = wp + __popcll(m & below);
                if (emit && at >= lo) payload[at] = (uint16_t)(x & 0xffffu);
            }
            count += (unsigned)cnt;
            if (emit) x >>= 16;
            if (active) x = rans_push(x, f, c);
        }
    }
    if (kWrite) {
        uint16_t *st = payload + (lo - kStateWords);
        st[2 * lane] = (uint16_t)(x & 0xffffu);
        st[2 * lane + 1] = (uint16_t)(x >> 16);
    } else if (lane == 0) {
        sizes_out[p] = count + (unsigned)kStateWords;
    }
}

// Untrusted input: sizes, offsets and words may come from a damaged or foreign file.  Every read stays inside the part's
// [off, off + size), which is checked against [0, n_words) first; every symbol written is below T.  *status: bit 0 a part
// size outside [128, m + 128]; bit 1 a part ran out of words; bit 2 words left over or a final state other than 2^16; bit 3
// an invalid frequency row; bit 4 a part outside the payload, or the last part not ending at n_words (the sizes do not add
// up to n_words).  A part with any bit set decodes to zeros.
//
// The words come through a two-register window: lane j holds words base + j (`cur`) and base + 64 + j (`nxt`) of the part, a
// lane takes its word from them by a shuffle, and the window moves on by 64 when `cur` is used up: one coalesced load per 64
// words instead of a dependent 2-byte load per lane and step.
__global__ void __launch_bounds__(kLanes)
k_il_decode(const uint16_t *__restrict__ payload, long n_words, const uint32_t *__restrict__ sizes,
            const int64_t *__restrict__ offs, long P, long n, long total, int T, int part, const uint16_t *__restrict__ freq,
            uint16_t *__restrict__ idx, uint32_t *__restrict__ status) {
    __shared__ uint32_t fc_l[2048];
    __shared__ uint16_t c_l[2048 + 2];
    __shared__ uint16_t start[(1 << kPB) / 16];
    const int lane = threadIdx.x;
    const long p = blockIdx.x;
    const long a = p * (long)part;
    const long b = a + part < total ? a + part : total;
    const long k0 = sizes[p], off = offs[p];
    unsigned bad = 0;
    if (k0 < kStateWords || k0 > (b - a) + kStateWords) bad |= 1u;
    if (off < 0 || off > n_words - k0 || (p == P - 1 && off + k0 != n_words)) bad |= 16u;
    if (!bad) {
        const uint16_t *in = payload + off;                      // reads: in[j] with 0 <= j < k0 only
        unsigned x = (unsigned)in[2 * lane] | ((unsigned)in[2 * lane + 1] << 16);
        long base = kStateWords, rp = kStateWords;               // window start and next unread word, relative to `in`
        unsigned cur = base + lane < k0 ? (unsigned)in[base + lane] : 0u;
        unsigned nxt = base + kLanes + lane < k0 ? (unsigned)in[base + kLanes + lane] : 0u;
        const unsigned long long below = (1ull << lane) - 1ull;
        for (long s = a / n; s <= (b - 1) / n && !bad; ++s) {    // stream of the run (wave-uniform)
            const long rs = s * n > a ? s * n : a;
            const long re = (s + 1) * n < b ? (s + 1) * n : b;
            const int len = (int)(re - rs);
            if (!stage_tables_il<true>(freq + s * T, T, fc_l, c_l, start)) { bad |= 8u; break; }
            uint16_t *dst = idx + rs;
            for (int t = 0; t * kLanes < len; ++t) {
                const bool active = t * kLanes + lane < len;
                unsigned sym = 0;
                if (active) sym = rans_pop(x, start, c_l, fc_l);
                const bool need = active && x < kRansL;
                const unsigned long long m = __ballot(need);
                const int cnt = __popcll(m);
                if (rp + cnt > k0) { bad |= 2u; break; }         // wave-uniform: a valid part holds every word its steps take
                const int j = (int)(rp - base) + __popcll(m & below);   // 0 .. 127
                const unsigned w0 = __shfl(cur, j & 63, 64), w1 = __shfl(nxt, j & 63, 64);
                if (need) x = (x << 16) | (j < kLanes ? w0 : w1);
                rp += cnt;
                if (rp - base >= kLanes) {
                    base += kLanes;
                    cur = nxt;
                    nxt = base + kLanes + lane < k0 ? (unsigned)in[base + kLanes + lane] : 0u;
                }
                if (active) dst[t * kLanes + lane] = (uint16_t)sym;
            }
        }
        if (!bad && (rp != k0 || __any(x != kRansL))) bad |= 4u;
    }
    if (bad) {
        for (long i = a + lane; i < b; i += kLanes) idx[i] = 0;
        if (status && lane == 0) atomicOr(status, bad);
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
