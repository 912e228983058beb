// f2: a static-model rANS coder for the rank indices, so that the rates the
// reference only ESTIMATES as sum(-log2 freq) (quantizer.py:144,226-228) become real bits.
//
// Format (ours; the reference has no coder): every (lambda, channel) stream of n indices is cut
// into segments of `seg` symbols; each segment is an independent rANS stream (32-bit state,
// 16-bit renormalisation, PB = 15 probability bits, frequencies >= 1 summing to 2^15):
//     words[0..k-3] = renormalisation words in emission order, words[k-2], words[k-1] = final state
//     (low, high half), k = size of the segment in 16-bit words (<= seg + 2).
// Symbols are encoded last-to-first, so the decoder -- starting from the state at the END of the
// segment and consuming words backwards -- reproduces them first-to-last.  One thread per
// segment; the 64 segments of a workgroup belong to one stream and share its frequency /
// cumulative tables in LDS.  oracle/vbq_oracle.c (rans_* functions) is the bit-exact checker.
// Table staging, the bucket table, the segment reader (the rules for untrusted words) and the
// argument check of the entry points are vbq_rans_common.h's, shared with vbq_rans_map.hip.
#include "vbq_rans_common.h"

namespace vbq {
namespace {

constexpr int kRansThreads = 64;

// One thread per segment; a lane walks its segment from the last symbol to the first.  Symbols come in 16-byte groups of eight
// where the layout allows it (segment length and stream length multiples of eight: one load per eight symbols instead of eight
// dependent 2-byte loads from a line other lanes do not share).
__global__ void __launch_bounds__(kRansThreads)
k_rans_encode(const uint16_t *__restrict__ idx, long n, int T, int seg, int nseg, const uint16_t *__restrict__ freq,
              uint16_t *__restrict__ words, uint32_t *__restrict__ sizes) {
    __shared__ uint32_t fc_l[2048];
    const long s = blockIdx.y;                                   // stream
    stage_segment_table<true>(freq + s * T, T, fc_l, nullptr);
    __syncthreads();
    const int g = blockIdx.x * kRansThreads + threadIdx.x;       // segment within the stream
    if (g >= nseg) return;
    const long a = (long)g * seg;
    const long b = a + seg < n ? a + seg : n;
    const uint16_t *src = idx + s * n;
    uint16_t *out = words + (s * nseg + g) * (long)(seg + 2);
    unsigned x = kRansL;
    int k = 0;
    auto put = [&](unsigned sym) {
        const unsigned fc = fc_l[sym < (unsigned)T ? sym : 0u];  // (an index outside the table: memory-safe; vbq_index_max_u16 tells beforehand)
        const unsigned f = fc & 0xffffu, c = fc >> 16;
        if (x >= (f << (32 - kPB))) { out[k++] = (uint16_t)(x & 0xffffu); x >>= 16; }
        x = rans_push(x, f, c);
    };
    long i = b;
    const bool vec = ((seg | n) % 8 == 0) && (reinterpret_cast<uintptr_t>(src) % 16 == 0);
    if (vec) {
        for (; i - 8 >= a; i -= 8) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + i - 8);
            put(v.w >> 16); put(v.w & 0xffffu); put(v.z >> 16); put(v.z & 0xffffu);
            put(v.y >> 16); put(v.y & 0xffffu); put(v.x >> 16); put(v.x & 0xffffu);
        }
    }
    for (--i; i >= a; --i) put(src[i]);
    out[k++] = (uint16_t)(x & 0xffffu);
    out[k++] = (uint16_t)(x >> 16);
    sizes[s * nseg + g] = (uint32_t)k;
}

// The sizes k_rans_encode writes, without the words: the same state machine, renormalisation and final-state flush over the same
// symbols in the same order (the same 16-byte loads where the layout allows them), storing only the count k of every segment --
// the exact coded length without a (seg + 2)-word buffer per segment.  (The encoder keeps its own copy of these lines: moving its
// body into a helper shared by both kernels, templated on the word stores, changed the register allocation of k_rans_encode --
// one more v_mov on every renormalisation -- and its ISA is pinned; tests/test_gpu_budget.py pins the two kernels' sizes to each
// other and to the C checker element by element.)
__global__ void __launch_bounds__(kRansThreads)
k_rans_sizes(const uint16_t *__restrict__ idx, long n, int T, int seg, int nseg, const uint16_t *__restrict__ freq,
             uint32_t *__restrict__ sizes) {
    __shared__ uint32_t fc_l[2048];
    const long s = blockIdx.y;                                   // stream
    stage_segment_table<true>(freq + s * T, T, fc_l, nullptr);
    __syncthreads();
    const int g = blockIdx.x * kRansThreads + threadIdx.x;       // segment within the stream
    if (g >= nseg) return;
    const long a = (long)g * seg;
    const long b = a + seg < n ? a + seg : n;
    const uint16_t *src = idx + s * n;
    unsigned x = kRansL;
    int k = 0;
    auto put = [&](unsigned sym) {
        const unsigned fc = fc_l[sym < (unsigned)T ? sym : 0u];  // (an index outside the table: memory-safe, as in the encoder)
        const unsigned f = fc & 0xffffu, c = fc >> 16;
        if (x >= (f << (32 - kPB))) { ++k; x >>= 16; }
        x = rans_push(x, f, c);
    };
    long i = b;
    const bool vec = ((seg | n) % 8 == 0) && (reinterpret_cast<uintptr_t>(src) % 16 == 0);
    if (vec) {
        for (; i - 8 >= a; i -= 8) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + i - 8);
            put(v.w >> 16); put(v.w & 0xffffu); put(v.z >> 16); put(v.z & 0xffffu);
            put(v.y >> 16); put(v.y & 0xffffu); put(v.x >> 16); put(v.x & 0xffffu);
        }
    }
    for (--i; i >= a; --i) put(src[i]);
    sizes[s * nseg + g] = (uint32_t)(k + 2);                     // + the final state's two words
}

// Untrusted input: the segment sizes and words may come from a damaged or foreign file.  Every read is kept
// inside the segment's (seg + 2)-word buffer and every decoded symbol below T; what is wrong is reported in
// *status (bit 0: a segment size outside [2, seg + 2]; bit 1: a segment ran out of words; bit 2: words left
// over or a final state other than the encoder's start state -- SegmentReader; bit 3: a frequency row that does
// not sum to 2^15 -- stage_segment_table).
__global__ void __launch_bounds__(kRansThreads)
k_rans_decode(const uint16_t *__restrict__ words, const uint32_t *__restrict__ sizes, long n, int T, int seg, int nseg,
              const uint16_t *__restrict__ freq, uint16_t *__restrict__ idx, uint32_t *__restrict__ status) {
    __shared__ uint32_t fc_l[2048];
    __shared__ uint16_t c_l[2049 + 1];
    // start[b] = the symbol whose slot range contains slot 16 b: the search for a slot begins there and walks
    // up (a bucket of 16 slots holds 1 symbol on average), instead of 11 dependent LDS reads of a bisection
    __shared__ uint16_t start[(1 << kPB) / 16];
    const long s = blockIdx.y;
    stage_segment_table<true>(freq + s * T, T, fc_l, c_l);
    __syncthreads();
    const bool table_ok = c_l[T] == (uint16_t)(1u << kPB);
    if (table_ok) {
        for (int bkt = threadIdx.x; bkt < (1 << kPB) / 16; bkt += kRansThreads) {
            start[bkt] = bucket_start(c_l, T, 16u * bkt);
        }
    }
    __syncthreads();
    const int g = blockIdx.x * kRansThreads + threadIdx.x;
    if (g >= nseg) return;
    const long a = (long)g * seg;
    const long b = a + seg < n ? a + seg : n;
    const uint16_t *in = words + (s * nseg + g) * (long)(seg + 2);
    uint16_t *dst = idx + s * n;
    unsigned bad = table_ok ? 0u : 8u;
    const unsigned k0 = sizes[s * nseg + g];
    if (k0 < 2u || k0 > (unsigned)seg + 2u) bad |= 1u;
    if (bad) {
        for (long i = a; i < b; ++i) dst[i] = 0;
        if (status) atomicOr(status, bad);
        return;
    }
    SegmentReader rd;
    rd.open(in, k0);
    bool starved = false;
    auto get = [&]() -> unsigned {                               // one symbol; after a starved stream: zeros
        if (starved) return 0u;
        const unsigned lo = rans_pop(rd.x, start, c_l, fc_l);
        if (!rd.refill()) { bad |= 2u; starved = true; }
        return lo;
    };
    long i = a;
    // eight symbols per 16-byte store where the layout allows it (instead of eight 2-byte stores into a line of its own)
    if (((seg | n) % 8 == 0) && (reinterpret_cast<uintptr_t>(dst) % 16 == 0)) {
        for (; i + 8 <= b; i += 8) {
            uint4 v;
            v.x = get(); v.x |= get() << 16;
            v.y = get(); v.y |= get() << 16;
            v.z = get(); v.z |= get() << 16;
            v.w = get(); v.w |= get() << 16;
            *reinterpret_cast<uint4 *>(dst + i) = v;
        }
    }
    for (; i < b; ++i) dst[i] = (uint16_t)get();
    if (!bad && !rd.clean()) bad |= 4u;
    if (bad && status) atomicOr(status, bad);
}

// ---- the byte-string container (vbq_amd/bitstream.py): padded segments [M][seg+2] <-> contiguous payload ----
// Segment g (M = n_streams * nseg of them, stream-major) occupies payload words [off[g], off[g] + size[g]), off = exclusive
// prefix sum of the sizes.  Two launches either way:
//   k_scan_groups   ONE workgroup: thread t sums the sizes of group t (kGroup consecutive segments), the workgroup scans those
//                   totals (wave64 shuffles + LDS) into exclusive group offsets -> offs[first segment of the group], and writes
//                   the grand total.  Any number of groups: chunks of kScanThreads groups with a running carry.  (A separate
//                   multi-workgroup pass for the group totals was one more launch: ~5 us more on an image's 512 - 9216
//                   segments, where the single workgroup needs one chunk.)
//   k_copy_segments one wave per segment: its offset = the group's offset + the sizes before it in the group (a 16-lane
//                   shuffle sum, no LDS), then the 64 lanes copy its words (coalesced on both sides)
// Unpacking reads UNTRUSTED sizes: one outside [2, seg + 2] counts as 0 (status bit 0), a segment that would read past n_words
// is left zero-sized (the decoder then rejects it), and a total other than n_words sets status bit 4.
constexpr int kGroup = 16;
constexpr int kScanThreads = 1024;
constexpr int kCopyThreads = 256;                                // 4 waves = 4 segments per workgroup

template <bool kUntrusted, typename SizeT>
__device__ __forceinline__ unsigned segment_size(const SizeT *sizes, long i, int seg, unsigned &bad) {
    const unsigned k = sizes[i];
    if (kUntrusted) {
        if (k < 2u || k > (unsigned)seg + 2u) { bad = 1u; return 0u; }
        return k;
    }
    return k < (unsigned)seg + 2u ? k : (unsigned)seg + 2u;     // (the encoder never writes more; clamped for memory safety)
}

template <bool kUntrusted, typename SizeT>
__global__ void __launch_bounds__(kScanThreads)
k_scan_groups(const SizeT *__restrict__ sizes, long M, int seg, long expect, int64_t *__restrict__ offs,
              uint64_t *__restrict__ total, uint32_t *__restrict__ status) {
    __shared__ long wsum[kScanThreads / 64];
    const long G = (M + kGroup - 1) / kGroup;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned bad = 0;
    long carry = 0;                                              // the same in every thread (it only reads wsum)
    for (long base = 0; base < G; base += kScanThreads) {
        const long gi = base + threadIdx.x;
        long v = 0;
        if (gi < G) {
            const long a = gi * kGroup, b = a + kGroup < M ? a + kGroup : M;
            for (long i = a; i < b; ++i) v += segment_size<kUntrusted>(sizes, i, seg, bad);
        }
        long incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long u = __shfl_up(incl, o, 64);
            if (lane >= o) incl += u;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        long before = carry, chunk = 0;
        for (int w = 0; w < kScanThreads / 64; ++w) {
            if (w < wave) before += wsum[w];
            chunk += wsum[w];
        }
        if (gi < G) offs[gi * kGroup] = before + incl - v;
        carry += chunk;
        __syncthreads();                                         // wsum is rewritten by the next chunk
    }
    if (bad && status) atomicOr(status, 1u);
    if (threadIdx.x == 0) {
        if (total) *total = (uint64_t)carry;
        if (expect >= 0 && carry != expect && status) atomicOr(status, 16u);
    }
}

template <bool kUnpack, typename SizeT>
__global__ void __launch_bounds__(kCopyThreads)
k_copy_segments(const uint16_t *__restrict__ src, const SizeT *__restrict__ sizes, long M, int seg, long n_words,
                int64_t *__restrict__ offs, uint16_t *__restrict__ dst, uint32_t *__restrict__ sizes_out) {
    const int lane = threadIdx.x & 63;
    const long g = (long)blockIdx.x * (kCopyThreads / 64) + (threadIdx.x >> 6);
    if (g >= M) return;                                          // wave-uniform
    const long g0 = g - g % kGroup;
    const int r = (int)(g - g0);
    unsigned bad = 0, kl = 0;
    if (lane < kGroup && g0 + lane < M) kl = segment_size<kUnpack>(sizes, g0 + lane, seg, bad);
    unsigned before = lane < r ? kl : 0u;
#pragma unroll
    for (int o = kGroup / 2; o >= 1; o >>= 1) before += __shfl_xor(before, o, 64);   // lanes 0..15: sum of the group's first r
    before = __shfl(before, 0, 64);
    const unsigned k = __shfl(kl, r, 64);
    const long off = (long)offs[g0] + before;                    // offs[g0] = the group's offset (k_scan_groups)
    if (lane == 0 && r != 0) offs[g] = off;                      // (segment g0's own entry already holds it)
    const uint16_t *s;
    uint16_t *d;
    if (kUnpack) {
        const bool fits = k != 0u && off + (long)k <= n_words;   // off >= 0: every read stays in [0, n_words)
        if (lane == 0) sizes_out[g] = fits ? k : 0u;
        if (!fits) return;
        s = src + off;
        d = dst + g * (long)(seg + 2);                           // k <= seg + 2: every write stays in segment g's buffer
    } else {
        s = src + g * (long)(seg + 2);
        d = dst + off;
    }
    int j = lane;
    for (; j + 192 < (int)k; j += 256) {                         // four loads in flight before the stores
        const uint16_t a = s[j], b = s[j + 64], c = s[j + 128], e = s[j + 192];
        d[j] = a; d[j + 64] = b; d[j + 128] = c; d[j + 192] = e;
    }
    for (; j < (int)k; j += 64) d[j] = s[j];
}

}  // namespace
}  // namespace vbq

extern "C" int vbq_rans_encode_u16(const uint16_t *d_idx, int64_t n_streams, int64_t n, int32_t N, int32_t seg,
                                   const uint16_t *d_freq, uint16_t *d_words, uint32_t *d_sizes, void *stream) {
    using namespace vbq;
    int64_t nseg;
    if (int r = check_segments("vbq_rans_encode_u16", n_streams, n, N, seg, nseg)) return r;
    if (n_streams == 0 || n == 0) return VBQ_OK;
    VBQ_REQUIRE(d_idx && d_freq && d_words && d_sizes, VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_encode_u16: null pointer argument");
    hipLaunchKernelGGL(k_rans_encode, segment_grid(nseg, n_streams), dim3(kRansThreads), 0, reinterpret_cast<hipStream_t>(stream),
                       d_idx, (long)n, table_size(N), (int)seg, (int)nseg, d_freq, d_words, d_sizes);
    VBQ_CHECK_LAUNCH("rans_encode");
    return VBQ_OK;
}

extern "C" int vbq_rans_sizes_u16(const uint16_t *d_idx, int64_t n_streams, int64_t n, int32_t N, int32_t seg,
                                  const uint16_t *d_freq, uint32_t *d_sizes, void *stream) {
    using namespace vbq;
    int64_t nseg;
    if (int r = check_segments("vbq_rans_sizes_u16", n_streams, n, N, seg, nseg)) return r;
    if (n_streams == 0 || n == 0) return VBQ_OK;
    VBQ_REQUIRE(d_idx && d_freq && d_sizes, VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_sizes_u16: null pointer argument");
    hipLaunchKernelGGL(k_rans_sizes, segment_grid(nseg, n_streams), dim3(kRansThreads), 0, reinterpret_cast<hipStream_t>(stream),
                       d_idx, (long)n, table_size(N), (int)seg, (int)nseg, d_freq, d_sizes);
    VBQ_CHECK_LAUNCH("rans_sizes");
    return VBQ_OK;
}

extern "C" int vbq_rans_decode_u16(const uint16_t *d_words, const uint32_t *d_sizes, int64_t n_streams, int64_t n,
                                   int32_t N, int32_t seg, const uint16_t *d_freq, uint16_t *d_idx, uint32_t *d_status,
                                   void *stream) {
    using namespace vbq;
    int64_t nseg;
    if (int r = check_segments("vbq_rans_decode_u16", n_streams, n, N, seg, nseg)) return r;
    if (n_streams == 0 || n == 0) return VBQ_OK;
    VBQ_REQUIRE(d_idx && d_freq && d_words && d_sizes, VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_decode_u16: null pointer argument");
    hipLaunchKernelGGL(k_rans_decode, segment_grid(nseg, n_streams), dim3(kRansThreads), 0, reinterpret_cast<hipStream_t>(stream),
                       d_words, d_sizes, (long)n, table_size(N), (int)seg, (int)nseg, d_freq, d_idx, d_status);
    VBQ_CHECK_LAUNCH("rans_decode");
    return VBQ_OK;
}

extern "C" int vbq_rans_pack_u16(const uint16_t *d_words, const uint32_t *d_sizes, int64_t n_streams, int64_t n, int32_t seg,
                                 uint16_t *d_payload, int64_t *d_offsets, uint64_t *d_total, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n_streams >= 0 && n >= 0 && seg >= 1 && seg <= 65533 && n_streams <= 65535, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_pack_u16: bad sizes n_streams=%lld n=%lld seg=%d", (long long)n_streams, (long long)n, seg);
    VBQ_REQUIRE(d_total, VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_pack_u16: null d_total");
    const int64_t M = n_streams * ((n + seg - 1) / seg);
    VBQ_REQUIRE(M == 0 || (d_words && d_sizes && d_payload && d_offsets), VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_pack_u16: null pointer argument");
    VBQ_REQUIRE((M + kCopyThreads / 64 - 1) / (kCopyThreads / 64) <= INT32_MAX, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_pack_u16: %lld segments are too many", (long long)M);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_groups<false, uint32_t>), dim3(1), dim3(kScanThreads), 0, st, d_sizes, (long)M,
                       (int)seg, -1L, d_offsets, d_total, nullptr);
    VBQ_CHECK_LAUNCH("rans_pack (scan)");
    if (M > 0) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_copy_segments<false, uint32_t>),
                           dim3((unsigned)((M + kCopyThreads / 64 - 1) / (kCopyThreads / 64))), dim3(kCopyThreads), 0, st,
                           d_words, d_sizes, (long)M, (int)seg, 0L, d_offsets, d_payload, nullptr);
        VBQ_CHECK_LAUNCH("rans_pack (copy)");
    }
    return VBQ_OK;
}

extern "C" int vbq_rans_unpack_u16(const uint16_t *d_payload, int64_t n_words, const uint16_t *d_sizes_in, int64_t n_streams,
                                   int64_t n, int32_t seg, uint16_t *d_words, uint32_t *d_sizes, int64_t *d_offsets,
                                   uint32_t *d_status, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n_words >= 0 && n_streams >= 0 && n >= 0 && seg >= 1 && seg <= 65533 && n_streams <= 65535,
                VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_unpack_u16: bad sizes n_words=%lld n_streams=%lld n=%lld seg=%d",
                (long long)n_words, (long long)n_streams, (long long)n, seg);
    const int64_t M = n_streams * ((n + seg - 1) / seg);
    VBQ_REQUIRE(M == 0 || (d_sizes_in && d_words && d_sizes && d_offsets), VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_unpack_u16: null pointer argument");
    VBQ_REQUIRE(n_words == 0 || d_payload, VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_unpack_u16: null d_payload");
    VBQ_REQUIRE((M + kCopyThreads / 64 - 1) / (kCopyThreads / 64) <= INT32_MAX, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_unpack_u16: %lld segments are too many", (long long)M);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_groups<true, uint16_t>), dim3(1), dim3(kScanThreads), 0, st, d_sizes_in, (long)M,
                       (int)seg, (long)n_words, d_offsets, nullptr, d_status);
    VBQ_CHECK_LAUNCH("rans_unpack (scan)");
    if (M > 0) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_copy_segments<true, uint16_t>),
                           dim3((unsigned)((M + kCopyThreads / 64 - 1) / (kCopyThreads / 64))), dim3(kCopyThreads), 0, st,
                           d_payload, d_sizes_in, (long)M, (int)seg, (long)n_words, d_offsets, d_words, d_sizes);
        VBQ_CHECK_LAUNCH("rans_unpack (copy)");
    }
    return VBQ_OK;
}

namespace vbq {
namespace {

// ---- row-wise decode of the embedding container (vbq_amd/bitstream.py, VBQe): ONE stream read straight from its packed
// payload into f32 values, without the padded layout of vbq_rans_unpack_u16 and without a u16 index array.
//   k_fill_offsets        after k_scan_groups<true, uint16_t>: every segment's exclusive offset, not only the group starts (one
//                         thread per segment adds the <= 15 sizes before it in its group to the group's offset)
//   k_rans_decode_values  one lane per segment as k_rans_decode; the decoded rank indexes a value table in LDS.  The frequency
//                         table may hold zeros (a model fitted to the data it codes: coder.exact_frequencies); the slot search
//                         then still ends on the one symbol whose slot range holds the slot, as every empty range is skipped.
//                         (Its staging stays its own: one pass also loads the values, rejects entries >= 2^15 before a
//                         cumulative sum could overflow, and fills start[] from the ranges without a bisection.)
constexpr int kFillThreads = 256;
constexpr int kValThreads = 64;                                  // one wave: the table staging scans with wave shuffles alone

__global__ void __launch_bounds__(kFillThreads)
k_fill_offsets(const uint16_t *__restrict__ sizes, long M, int seg, int64_t *__restrict__ offs) {
    const long g = (long)blockIdx.x * kFillThreads + threadIdx.x;
    if (g >= M) return;
    const long g0 = g - g % kGroup;
    if (g == g0) return;                                         // the group's own entry: written by k_scan_groups
    unsigned bad = 0;                                            // (reported by the scan already)
    long off = (long)offs[g0];
    for (long i = g0; i < g; ++i) off += segment_size<true>(sizes, i, seg, bad);
    offs[g] = off;
}

// Untrusted input as k_rans_decode, plus: a segment whose words [off, off + size) do not lie inside [0, n_words) counts as a bad
// size (bit 0), an entry of the frequency table above 2^15 - 1 makes the table invalid (bit 3), a listed segment id outside
// [0, nseg) sets bit 5 (32).  Segments with bits 0 / 3 / 5 decode to zeros.
__global__ void __launch_bounds__(kValThreads)
k_rans_decode_values(const uint16_t *__restrict__ payload, long n_words, const uint16_t *__restrict__ sizes,
                     const int64_t *__restrict__ offs, long n, int T, int seg, long nseg, const uint16_t *__restrict__ freq,
                     const float *__restrict__ values, const int64_t *__restrict__ segs, long count, float *__restrict__ out,
                     uint32_t *__restrict__ status) {
    __shared__ uint32_t fc_l[2048];
    __shared__ uint16_t c_l[2048 + 2];
    __shared__ uint16_t start[(1 << kPB) / 16];                  // start[b] = the symbol whose slot range holds slot 16 b
    __shared__ float val_l[2048];
    const int lane = threadIdx.x;
    const int per = (T + kValThreads - 1) / kValThreads;
    const int i0 = min(T, lane * per), i1 = min(T, (lane + 1) * per);
    unsigned sum = 0;
    bool big = false;
    for (int i = i0; i < i1; ++i) {
        const unsigned f = freq[i];
        fc_l[i] = f;
        val_l[i] = values[i];
        sum += f;
        big |= f >= (1u << kPB);
    }
    unsigned incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    const bool table_ok = __shfl(incl, 63, 64) == (1u << kPB) && !__any(big);
    if (table_ok) {                                              // every partial sum <= 2^15: c fits in 16 bits
        unsigned run = incl - sum;
        for (int i = i0; i < i1; ++i) {
            const unsigned f = fc_l[i];
            fc_l[i] = f | (run << 16);
            c_l[i] = (uint16_t)run;
            for (unsigned b = (run + 15u) >> 4; 16u * b < run + f; ++b) start[b] = (uint16_t)i;   // the ranges tile [0, 2^15)
            run += f;
        }
        if (lane == 63) c_l[T] = (uint16_t)(1u << kPB);          // > every slot: ends the walk below T
    }
    __syncthreads();
    const long t = (long)blockIdx.x * kValThreads + lane;
    if (t >= count) return;
    const long g = segs ? segs[t] : t;
    float *dst = out + t * (long)seg;
    if (g < 0 || g >= nseg) {                                    // (only a listed id can be out of range)
        for (int j = 0; j < seg; ++j) dst[j] = 0.0f;
        if (status) atomicOr(status, 32u);
        return;
    }
    const long a = g * (long)seg;
    const int len = (int)(a + seg < n ? seg : n - a);
    unsigned bad = table_ok ? 0u : 8u;
    const unsigned k0 = sizes[g];
    const long off = offs[g];
    if (k0 < 2u || k0 > (unsigned)seg + 2u || off < 0 || off > n_words - (long)k0) bad |= 1u;
    if (bad) {
        for (int j = 0; j < len; ++j) dst[j] = 0.0f;
        if (status) atomicOr(status, bad);
        return;
    }
    SegmentReader rd;
    rd.open(payload + off, k0);                                  // reads stay in [off, off + k0) within [0, n_words)
    bool starved = false;
    auto get = [&]() -> float {                                  // one value; after a starved stream: the value of symbol 0
        if (starved) return val_l[0];
        const unsigned sym = rans_pop(rd.x, start, c_l, fc_l);
        if (!rd.refill()) { bad |= 2u; starved = true; }
        return val_l[sym];
    };
    int j = 0;
    // four values per 16-byte store where every segment's slot starts 16-byte aligned
    if (seg % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0) {
        for (; j + 4 <= len; j += 4) {
            float4 v;
            v.x = get(); v.y = get(); v.z = get(); v.w = get();
            *reinterpret_cast<float4 *>(dst + j) = v;
        }
    }
    for (; j < len; ++j) dst[j] = get();
    if (!bad && !rd.clean()) bad |= 4u;
    if (bad && status) atomicOr(status, bad);
}

}  // namespace
}  // namespace vbq

extern "C" int vbq_rans_segment_offsets_u16(const uint16_t *d_sizes, int64_t M, int32_t seg, int64_t n_words,
                                            int64_t *d_offsets, uint32_t *d_status, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(M >= 0 && n_words >= 0 && seg >= 1 && seg <= 65533, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_segment_offsets_u16: bad sizes M=%lld seg=%d n_words=%lld", (long long)M, seg, (long long)n_words);
    VBQ_REQUIRE(M == 0 || (d_sizes && d_offsets), VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_segment_offsets_u16: null pointer argument");
    VBQ_REQUIRE((M + kFillThreads - 1) / kFillThreads <= INT32_MAX, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_segment_offsets_u16: %lld segments are too many", (long long)M);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_groups<true, uint16_t>), dim3(1), dim3(kScanThreads), 0, st, d_sizes, (long)M,
                       (int)seg, (long)n_words, d_offsets, nullptr, d_status);
    VBQ_CHECK_LAUNCH("rans_segment_offsets (scan)");
    if (M > 1) {
        hipLaunchKernelGGL(k_fill_offsets, dim3((unsigned)((M + kFillThreads - 1) / kFillThreads)), dim3(kFillThreads), 0, st,
                           d_sizes, (long)M, (int)seg, d_offsets);
        VBQ_CHECK_LAUNCH("rans_segment_offsets (fill)");
    }
    return VBQ_OK;
}

extern "C" int vbq_rans_decode_values_f32(const uint16_t *d_payload, int64_t n_words, const uint16_t *d_sizes,
                                          const int64_t *d_offsets, int64_t n, int32_t seg, int32_t N, const uint16_t *d_freq,
                                          const float *d_values, const int64_t *d_segments, int64_t n_sel, float *d_out,
                                          uint32_t *d_status, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n_words >= 0 && n >= 0 && seg >= 1 && seg <= 65533 && N >= 1 && N <= 10 && n_sel >= 0,
                VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_decode_values_f32: bad sizes n_words=%lld n=%lld seg=%d N=%d n_sel=%lld",
                (long long)n_words, (long long)n, seg, N, (long long)n_sel);
    const int64_t nseg = (n + seg - 1) / seg;
    const int64_t count = d_segments ? n_sel : nseg;
    if (count == 0) return VBQ_OK;
    VBQ_REQUIRE(d_sizes && d_offsets && d_freq && d_values && d_out, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_decode_values_f32: null pointer argument");
    VBQ_REQUIRE(n_words == 0 || d_payload, VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_decode_values_f32: null d_payload");
    VBQ_REQUIRE((count + kValThreads - 1) / kValThreads <= INT32_MAX, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_decode_values_f32: %lld segments are too many", (long long)count);
    hipLaunchKernelGGL(k_rans_decode_values, dim3((unsigned)((count + kValThreads - 1) / kValThreads)), dim3(kValThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), d_payload, (long)n_words, d_sizes, d_offsets, (long)n,
                       table_size(N), (int)seg, (long)nseg, d_freq, d_values, d_segments, (long)count, d_out, d_status);
    VBQ_CHECK_LAUNCH("rans_decode_values");
    return VBQ_OK;
}
