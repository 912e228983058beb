// What the rANS coders share -- vbq_rans.hip (segments, one lane per segment), vbq_rans_map.hip (the same with a table per
// symbol) and vbq_rans_il.hip (parts, the 64 lanes of a wave together): the coder's constants and the per-symbol state updates
// of the encoder and of the decoder.  32-bit state, start state 2^16, 16-bit renormalisation words, 15 probability bits;
// format: include/vbq.h.  The two segment coders also share, further down, how a frequency row reaches LDS, the bucket table
// of the slot search, the rules for reading an untrusted segment and the host-side argument check; the interleaved coder maps
// lanes to symbols differently and keeps its own staging and its own two-register word window (vbq_rans_il_common.h, for
// vbq_rans_il.hip and vbq_rans_il_files.hip).
#pragma once
#include "vbq_common.h"

namespace vbq {

constexpr int kPB = 15;
constexpr unsigned kRansL = 1u << 16;

// x / f and x % f for 1 <= f < 2^15 and x < f 2^17 (the encoder's invariant after renormalisation) without the ~35-instruction
// expansion of a 32-bit division: the quotient is below 2^17, a float estimate of it is off by at most one, and the remainder says
// which way (exact by construction: the result is verified, not trusted).
__device__ __forceinline__ void divmod_small(unsigned x, unsigned f, unsigned &q, unsigned &r) {
    q = (unsigned)(__uint2float_rn(x) * __builtin_amdgcn_rcpf(__uint2float_rn(f)));
    int rr = (int)(x - q * f);
    if (rr < 0) { rr += (int)f; --q; }
    if (rr >= (int)f) { rr -= (int)f; ++q; }
    r = (unsigned)rr;
}

// The encoder's step: the renormalised state x takes the symbol of frequency f and exclusive cumulative frequency c.
__device__ __forceinline__ unsigned rans_push(unsigned x, unsigned f, unsigned c) {
    unsigned q, r;
    divmod_small(x, f, q, r);
    return (q << kPB) + r + c;
}

// The decoder's step, before its renormalisation: the symbol whose slot range [c, c + f) holds the state's slot, and the state
// without it.  Tables in LDS: fc_l[sym] = f | c << 16, c_l[sym] = c with c_l[T] = 2^15, start[b] = the symbol whose range holds
// slot 16 b -- the search begins there and walks up (a bucket of 16 slots holds one symbol on average; empty ranges are skipped).
__device__ __forceinline__ unsigned rans_pop(unsigned &x, const uint16_t *start, const uint16_t *c_l, const uint32_t *fc_l) {
    const unsigned slot = x & ((1u << kPB) - 1u);
    unsigned sym = start[slot >> 4];                             // last symbol with c <= slot
    while (c_l[sym + 1] <= slot) ++sym;                          // c_l[T] = 2^15 > slot ends the walk below T
    const unsigned fc = fc_l[sym];
    x = (fc & 0xffffu) * (x >> kPB) + slot - (fc >> 16);
    return sym;
}

// The same step without the fc table: f = c[sym + 1] - c[sym], for a decoder that keeps several tables in LDS at once
// (vbq_rans_map.hip) and has no room for a third array per table.
__device__ __forceinline__ unsigned rans_pop(unsigned &x, const uint16_t *start, const uint16_t *c_l) {
    const unsigned slot = x & ((1u << kPB) - 1u);
    unsigned sym = start[slot >> 4];
    unsigned c1 = c_l[sym + 1];
    while (c1 <= slot) c1 = c_l[++sym + 1];
    const unsigned c0 = c_l[sym];
    x = (c1 - c0) * (x >> kPB) + slot - c0;
    return sym;
}

// ---- the segment layout (vbq_rans.hip, vbq_rans_map.hip): one lane per segment, the 64 segments of a workgroup share a stream ----

// One frequency row into LDS by ONE wave, each lane a contiguous chunk of the exclusive prefix sum: fc_l[i] = f | c << 16 with
// kFc (f >= 1, c < 2^15: one LDS read per symbol in an encoder), c_l[i] = c where c_l is given, with c_l[T] = 2^15 for a row that
// sums to 2^15 and 0 for one that does not (it may overflow the 16 bits: a decoder rejects it through c_l[T] before it uses
// any entry).  The barrier is the caller's, after its last row.  (kFc is a template flag and the loop bounds are spelled as
// they are because k_rans_encode's instruction stream is pinned: a run-time test of fc_l, or bounds hoisted into i0 / i1,
// change it.)
template <bool kFc>
__device__ __forceinline__ void stage_segment_table(const uint16_t *__restrict__ freq, int T, uint32_t *fc_l, uint16_t *c_l) {
    const int lane = threadIdx.x;
    const int per = (T + 63) / 64;
    unsigned sum = 0;
    for (int i = lane * per; i < min(T, (lane + 1) * per); ++i) sum += freq[i];
    unsigned incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    unsigned run = incl - sum;
    for (int i = lane * per; i < min(T, (lane + 1) * per); ++i) {
        const unsigned f = freq[i];
        if (kFc) fc_l[i] = f | (run << 16);
        if (c_l) c_l[i] = (uint16_t)run;
        run += f;
    }
    if (lane == 63 && c_l) c_l[T] = (uint16_t)(incl == (1u << kPB) ? incl : 0u);
}

// fc_l[t] = fc_l[canon[t]] for every t, by the one wave that staged fc_l: the whole table through registers (T <= 2047: at
// most 32 entries per lane) between two barriers, so that no entry is overwritten before it was read.  An encoder that reads
// fc_l[sym] then codes symbol canon[sym] at no cost per symbol.  (An entry of canon outside the table counts as 0.)  For the
// batch kernels (vbq_rans_files.hip, vbq_rans_sizes_files.hip, and per run vbq_rans_il_common.h's encoder).
__device__ __forceinline__ void map_segment_table(const uint16_t *__restrict__ canon, int T, uint32_t *fc_l) {
    const int lane = threadIdx.x;
    uint32_t v[32];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const int t = j * 64 + lane;
        v[j] = 0u;
        if (t < T) {
            const unsigned s = canon[t];
            v[j] = fc_l[s < (unsigned)T ? s : 0u];
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const int t = j * 64 + lane;
        if (t < T) fc_l[t] = v[j];
    }
}

// start[b] of rans_pop for slot = 16 b: the last symbol with c <= slot, by bisection over a valid row's c_l[0..T).
__device__ __forceinline__ uint16_t bucket_start(const uint16_t *c_l, int T, unsigned slot) {
    int lo = 0, hi = T;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (c_l[mid] <= slot) lo = mid; else hi = mid;
    }
    return (uint16_t)lo;
}

// A decoder with a table per class (vbq_rans_map.hip, vbq_rans_map_window.hip) keeps, per class in use, c[0..T] and start[] in LDS.
constexpr int kMapMaxClasses = 4;
constexpr int kMapT = 2048;                                      // table stride in LDS (T <= 2047)
constexpr int kMapCStride = kMapT + 2;                           // c[0..T], an even count of u16
constexpr int kMapBuckets = (1 << kPB) / 16;

// Reading one segment, whose words are UNTRUSTED: words[0 .. k - 3] renormalisation words in emission order, words[k - 2],
// words[k - 1] the final state (low, high half).  The decoder starts from that state and consumes the words backwards.  What a
// kernel decodes after a starved segment, and which flag it keeps, is the kernel's own business.
struct SegmentReader {
    const uint16_t *in;
    int k;                                                       // words not yet consumed
    unsigned x;                                                  // the state

    // The caller has checked 2 <= k0 <= seg + 2 (status bit 0 otherwise) and that words[0 .. k0) may be read.
    __device__ __forceinline__ void open(const uint16_t *words, unsigned k0) {
        in = words;
        k = (int)k0;
        x = ((unsigned)in[k - 1] << 16) | in[k - 2];
        k -= 2;
    }
    // After every rans_pop(x, ...).  false: the segment starved (status bit 1) -- a valid one never renormalises past its
    // first word; x is then not to be decoded from again.
    __device__ __forceinline__ bool refill() {
        if (x < kRansL) {
            if (k == 0) return false;
            x = (x << 16) | in[--k];
        }
        return true;
    }
    // After the last symbol: the encoder started from kRansL with no word written (status bit 2 otherwise).
    __device__ __forceinline__ bool clean() const { return k == 0 && x == kRansL; }
};

// ---- host side: what every entry point over (n_streams, n, N, seg) checks before any device work ----

// The sizes the segment coders accept, and nseg = ceil(n / seg), which the kernels take as an int.  (pack / unpack / the value
// decoder take other arguments and word their own messages.)
inline int check_segments(const char *who, int64_t n_streams, int64_t n, int32_t N, int32_t seg, int64_t &nseg) {
    VBQ_REQUIRE(n_streams >= 0 && n >= 0 && N >= 1 && N <= 10 && seg >= 1 && seg <= 65533 && n_streams <= 65535,
                VBQ_ERR_INVALID_ARGUMENT, "%s: bad sizes n_streams=%lld n=%lld N=%d seg=%d", who, (long long)n_streams,
                (long long)n, N, seg);
    nseg = (n + seg - 1) / seg;
    VBQ_REQUIRE(nseg <= INT32_MAX, VBQ_ERR_INVALID_ARGUMENT, "%s: %lld segments per stream are too many", who, (long long)nseg);
    return VBQ_OK;
}

// One 64-lane workgroup per 64 segments of a stream.
inline dim3 segment_grid(int64_t nseg, int64_t n_streams) { return dim3((unsigned)((nseg + 63) / 64), (unsigned)n_streams); }

}  // namespace vbq
