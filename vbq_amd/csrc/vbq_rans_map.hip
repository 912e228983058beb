// Class-mapped rANS: the segment coder of vbq_rans.hip with a frequency table that may change from symbol to symbol.  A class
// map cls[i] in [0, P), P <= 4, shared by every stream, picks for symbol i of stream s the table d_freq[cls[i]][s] -- one latent
// tensor coded at several lambdas (the lambda map of a VBQm file, vbq_amd/bitstream.py).  Format, constants, the per-symbol
// state updates, table staging, the bucket table, the segment reader and the size check are the segment coder's (include/vbq.h;
// vbq_rans_common.h): one lane per segment, the 64 segments of a workgroup belong to one stream, symbols are coded last to
// first.  A segment whose symbols all have class p comes out word for word what vbq_rans_encode_u16 writes with row d_freq[p][s].
//
// Tables in LDS, per class, only the n_classes in use (dynamic LDS, sized by the launch):
//   encoder / sizes   fc[sym] = f | c << 16                                    8 KB per class
//   decoder           c[0..T] (c[T] = 2^15) and start[2048]; f = c[sym + 1] - c[sym]: no fc table, 8 KB per class -- 32 KB at
//                     P = 4, where fc, c and start together would pass 64 KB
#include "vbq_rans_common.h"

namespace vbq {
namespace {

constexpr int kMapThreads = 64;

struct MapEncodeArgs {
    const uint16_t *idx;                                         // [n_planes][S][n]
    const uint8_t *cls;                                          // [n]
    const uint16_t *freq;                                        // [P][S][T]
    uint16_t *words;                                             // [S][nseg][seg + 2], unused by the sizes kernel
    uint32_t *sizes;                                             // [S][nseg]
    long n, plane;                                               // plane = S * n with n_planes == P, 0 with one plane
    int P, S, T, seg, nseg;
};

// kWords: the encoder; otherwise the sizes kernel (the same state machine over the same symbols in the same order, counting).
// Eight symbols per step where the layout allows it: their classes in one 8-byte load and, when the eight agree (a map is
// mostly smooth), the symbols in one 16-byte load from that class's plane.
template <bool kWords>
__global__ void __launch_bounds__(kMapThreads) k_rans_map_encode(const MapEncodeArgs a) {
    extern __shared__ uint32_t map_fc_l[];                       // [P][kMapT]
    const long s = blockIdx.y;
    const int T = a.T, P = a.P;
    for (int p = 0; p < P; ++p) stage_segment_table<true>(a.freq + ((long)p * a.S + s) * T, T, map_fc_l + p * kMapT, nullptr);
    __syncthreads();
    const int g = blockIdx.x * kMapThreads + threadIdx.x;
    if (g >= a.nseg) return;
    const long n = a.n;
    const long lo = (long)g * a.seg;
    const long hi = lo + a.seg < n ? lo + a.seg : n;
    const uint16_t *src = a.idx + s * n;                         // plane 0 of this stream
    uint16_t *out = kWords ? a.words + (s * a.nseg + g) * (long)(a.seg + 2) : nullptr;
    unsigned x = kRansL;
    int k = 0;
    auto put = [&](unsigned sym, unsigned p) {                   // p < P
        const unsigned fc = map_fc_l[p * kMapT + (sym < (unsigned)T ? sym : 0u)];   // (an index outside the table: memory-safe)
        const unsigned f = fc & 0xffffu, c = fc >> 16;
        if (x >= (f << (32 - kPB))) {
            if (kWords) out[k] = (uint16_t)(x & 0xffffu);
            ++k;
            x >>= 16;
        }
        x = rans_push(x, f, c);
    };
    auto cls_of = [&](unsigned c) -> unsigned { return c < (unsigned)P ? c : 0u; };   // (a class outside the palette: memory-safe)
    long i = hi;
    const bool vec = ((a.seg | n) % 8 == 0) && (reinterpret_cast<uintptr_t>(a.idx) % 16 == 0) &&
                     (reinterpret_cast<uintptr_t>(a.cls) % 8 == 0);
    if (vec) {
        for (; i - 8 >= lo; i -= 8) {
            const uint2 cv = *reinterpret_cast<const uint2 *>(a.cls + i - 8);
            const unsigned c0 = cv.x & 0xffu;
            if (cv.x == c0 * 0x01010101u && cv.y == cv.x) {
                const unsigned p = cls_of(c0);
                const uint4 v = *reinterpret_cast<const uint4 *>(src + p * a.plane + i - 8);
                put(v.w >> 16, p); put(v.w & 0xffffu, p); put(v.z >> 16, p); put(v.z & 0xffffu, p);
                put(v.y >> 16, p); put(v.y & 0xffffu, p); put(v.x >> 16, p); put(v.x & 0xffffu, p);
            } else {
#pragma unroll
                for (int j = 7; j >= 0; --j) {
                    const unsigned p = cls_of(((j < 4 ? cv.x : cv.y) >> (8 * (j & 3))) & 0xffu);
                    put(src[p * a.plane + i - 8 + j], p);
                }
            }
        }
    }
    for (--i; i >= lo; --i) {
        const unsigned p = cls_of(a.cls[i]);
        put(src[p * a.plane + i], p);
    }
    if (kWords) {
        out[k] = (uint16_t)(x & 0xffffu);
        out[k + 1] = (uint16_t)(x >> 16);
    }
    a.sizes[s * a.nseg + g] = (uint32_t)(k + 2);                 // + the final state's two words
}

// Untrusted input as k_rans_decode (vbq_rans.hip), status bits 0 - 3 with the same meaning; the classes are untrusted too: a
// class >= P in a segment sets bit 6 (64) and the segment decodes to zeros.  A class is compared with P before it indexes
// anything.
__global__ void __launch_bounds__(kMapThreads)
k_rans_map_decode(const uint16_t *__restrict__ words, const uint32_t *__restrict__ sizes, const uint8_t *__restrict__ cls, int P,
                  int S, long n, int T, int seg, int nseg, const uint16_t *__restrict__ freq, uint16_t *__restrict__ idx,
                  uint32_t *__restrict__ status) {
    extern __shared__ uint16_t map_dec_l[];                      // [P][kMapCStride] c, then [P][kMapBuckets] start
    uint16_t *c_all = map_dec_l;
    uint16_t *start_all = map_dec_l + P * kMapCStride;
    const long s = blockIdx.y;
    for (int p = 0; p < P; ++p) stage_segment_table<false>(freq + ((long)p * S + s) * T, T, nullptr, c_all + p * kMapCStride);
    __syncthreads();
    bool table_ok = true;
    for (int p = 0; p < P; ++p) table_ok &= c_all[p * kMapCStride + T] == (uint16_t)(1u << kPB);
    if (table_ok) {
        for (int t = threadIdx.x; t < P * kMapBuckets; t += kMapThreads) {
            const uint16_t *c_l = c_all + (t / kMapBuckets) * kMapCStride;
            start_all[t] = bucket_start(c_l, T, 16u * (t % kMapBuckets));
        }
    }
    __syncthreads();
    const int g = blockIdx.x * kMapThreads + threadIdx.x;
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
    bool dead = false;                                           // starved, or a class outside the palette: zeros from here on
    auto get = [&](unsigned c) -> unsigned {                     // one symbol of class c
        if (dead) return 0u;
        if (c >= (unsigned)P) { bad |= 64u; dead = true; return 0u; }
        const unsigned sym = rans_pop(rd.x, start_all + c * kMapBuckets, c_all + c * kMapCStride);
        if (!rd.refill()) { bad |= 2u; dead = true; }
        return sym;
    };
    long i = a;
    // eight symbols per 16-byte store, their classes in one 8-byte load, where the layout allows it
    if (((seg | n) % 8 == 0) && (reinterpret_cast<uintptr_t>(dst) % 16 == 0) && (reinterpret_cast<uintptr_t>(cls) % 8 == 0)) {
        for (; i + 8 <= b; i += 8) {
            const uint2 cv = *reinterpret_cast<const uint2 *>(cls + i);
            uint4 v;
            v.x = get(cv.x & 0xffu); v.x |= get((cv.x >> 8) & 0xffu) << 16;
            v.y = get((cv.x >> 16) & 0xffu); v.y |= get(cv.x >> 24) << 16;
            v.z = get(cv.y & 0xffu); v.z |= get((cv.y >> 8) & 0xffu) << 16;
            v.w = get((cv.y >> 16) & 0xffu); v.w |= get(cv.y >> 24) << 16;
            *reinterpret_cast<uint4 *>(dst + i) = v;
        }
    }
    for (; i < b; ++i) dst[i] = (uint16_t)get(cls[i]);
    if (bad & 64u)
        for (long j = a; j < b; ++j) dst[j] = 0;                 // the whole segment, what came before the bad class too
    if (!bad && !rd.clean()) bad |= 4u;
    if (bad && status) atomicOr(status, bad);
}

// What the three entry points take alike, before any device work: the palette, then the segment coder's sizes.
int map_check(const char *who, int32_t n_planes, int32_t n_classes, int64_t n_streams, int64_t n, int32_t N, int32_t seg,
              int64_t &nseg) {
    VBQ_REQUIRE(n_classes >= 1 && n_classes <= kMapMaxClasses, VBQ_ERR_INVALID_ARGUMENT, "%s: n_classes = %d outside [1, %d]", who,
                n_classes, kMapMaxClasses);
    VBQ_REQUIRE(n_planes == 1 || n_planes == n_classes, VBQ_ERR_INVALID_ARGUMENT, "%s: n_planes = %d is neither 1 nor n_classes = %d",
                who, n_planes, n_classes);
    return check_segments(who, n_streams, n, N, seg, nseg);
}

template <bool kWords>
int map_encode(const char *who, const uint16_t *d_idx, int32_t n_planes, const uint8_t *d_cls, int32_t n_classes, int64_t n_streams,
               int64_t n, int32_t N, int32_t seg, const uint16_t *d_freq, uint16_t *d_words, uint32_t *d_sizes, void *stream) {
    int64_t nseg;
    if (int r = map_check(who, n_planes, n_classes, n_streams, n, N, seg, nseg)) return r;
    if (n_streams == 0 || n == 0) return VBQ_OK;
    VBQ_REQUIRE(d_idx && d_cls && d_freq && d_sizes && (d_words || !kWords), VBQ_ERR_INVALID_ARGUMENT, "%s: null pointer argument", who);
    MapEncodeArgs a = {};
    a.idx = d_idx;
    a.cls = d_cls;
    a.freq = d_freq;
    a.words = d_words;
    a.sizes = d_sizes;
    a.n = (long)n;
    a.plane = n_planes > 1 ? (long)(n_streams * n) : 0L;
    a.P = n_classes;
    a.S = (int)n_streams;
    a.T = table_size(N);
    a.seg = seg;
    a.nseg = (int)nseg;
    hipLaunchKernelGGL(k_rans_map_encode<kWords>, segment_grid(nseg, n_streams), dim3(kMapThreads),
                       (size_t)n_classes * kMapT * sizeof(uint32_t), reinterpret_cast<hipStream_t>(stream), a);
    VBQ_CHECK_LAUNCH(who);
    return VBQ_OK;
}

}  // namespace
}  // namespace vbq

extern "C" int vbq_rans_map_encode_u16(const uint16_t *d_idx, int32_t n_planes, const uint8_t *d_cls, int32_t n_classes,
                                       int64_t n_streams, int64_t n, int32_t N, int32_t seg, const uint16_t *d_freq,
                                       uint16_t *d_words, uint32_t *d_sizes, void *stream) {
    return vbq::map_encode<true>("vbq_rans_map_encode_u16", d_idx, n_planes, d_cls, n_classes, n_streams, n, N, seg, d_freq, d_words,
                                 d_sizes, stream);
}

extern "C" int vbq_rans_map_sizes_u16(const uint16_t *d_idx, int32_t n_planes, const uint8_t *d_cls, int32_t n_classes,
                                      int64_t n_streams, int64_t n, int32_t N, int32_t seg, const uint16_t *d_freq,
                                      uint32_t *d_sizes, void *stream) {
    return vbq::map_encode<false>("vbq_rans_map_sizes_u16", d_idx, n_planes, d_cls, n_classes, n_streams, n, N, seg, d_freq, nullptr,
                                  d_sizes, stream);
}

extern "C" int vbq_rans_map_decode_u16(const uint16_t *d_words, const uint32_t *d_sizes, const uint8_t *d_cls, int32_t n_classes,
                                       int64_t n_streams, int64_t n, int32_t N, int32_t seg, const uint16_t *d_freq,
                                       uint16_t *d_idx, uint32_t *d_status, void *stream) {
    using namespace vbq;
    const char *who = "vbq_rans_map_decode_u16";
    int64_t nseg;
    if (int r = map_check(who, 1, n_classes, n_streams, n, N, seg, nseg)) return r;
    if (n_streams == 0 || n == 0) return VBQ_OK;
    VBQ_REQUIRE(d_words && d_sizes && d_cls && d_freq && d_idx, VBQ_ERR_INVALID_ARGUMENT, "%s: null pointer argument", who);
    hipLaunchKernelGGL(k_rans_map_decode, segment_grid(nseg, n_streams), dim3(kMapThreads),
                       (size_t)n_classes * (kMapCStride + kMapBuckets) * sizeof(uint16_t),
                       reinterpret_cast<hipStream_t>(stream), d_words, d_sizes, d_cls, (int)n_classes, (int)n_streams, (long)n,
                       table_size(N), (int)seg, (int)nseg, d_freq, d_idx, d_status);
    VBQ_CHECK_LAUNCH(who);
    return VBQ_OK;
}
