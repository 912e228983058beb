// Window decode of lambda-map files (vbq_amd/bitstream.py, magic "VBQm") and of files in segments at one lambda ("VBQb")
// together: the class-mapped twin of k_rans_decode_window (vbq_rans_window.hip).  A box of one file, or the same-sized boxes of
// many files, in ONE launch, straight from the packed payloads and the PACKED class blocks into channel-last f32 values -- no
// padded words, no u16 index tensor, no full-size Z_hat and no class byte per position in between.  Contract: include/vbq.h,
// "Mapped window decode".
//
// Geometry and work split are the plain kernel's: blocks of 64 listed segments x selected channel x file, one wave per
// workgroup, one lane decodes one listed segment in full and follows its row's position by increment and carry.  What differs:
// the table a symbol pops from is that of its position's class.  Per class of the file, c[0..T] and start[2048] in LDS
// (rans_pop without the fc table, as k_rans_map_decode), one val_l[2048] per workgroup since the code points do not depend on
// lambda: 8 KB + 8196 bytes per class, dynamic LDS sized by the launch's largest palette; a file of fewer classes stages only
// its own.  A lane reads its classes as the file stores them, 2 bits per position: one aligned 64-bit word per 32 symbols,
// the first one entered mid-word whenever g seg is not a multiple of 32.
//
// Table staging, the bucket table, the segment reader and the rules for untrusted words are vbq_rans_common.h's; the argument
// check and the grid are vbq_rans_window_common.h's, shared with the plain entry point.  The geometry check of a descriptor,
// the lookup of a listed segment, the position walk and the store (WindowFile, window_file_ok, window_segment, WindowCursor
// below) restate lines of k_rans_decode_window: moving those into functions that both kernels call changed the plain kernel's
// instruction stream (tools/isa_diff.py against the parent: 1188 of 2024 lines), so that kernel keeps its text.
#include "vbq_rans_window_common.h"

namespace vbq {
namespace {

constexpr int kMapFileFields = 16;                               // seg_base, n, D1, D2, a0, a1, a2, P, table[4], cls_base, 0, 0, 0

// Fields 0 - 6 of a descriptor: the geometry, as in the plain kernel's.
struct WindowFile {
    long seg_base, n, D1, D2, a0, a1, a2;
    __device__ __forceinline__ explicit WindowFile(const int64_t *d)
        : seg_base(d[0]), n(d[1]), D1(d[2]), D2(d[3]), a0(d[4]), a1(d[5]), a2(d[6]) {}
};

// The descriptor's geometry and EVERY listed channel: workgroup-uniform, so the whole workgroup leaves together on false.
__device__ __forceinline__ bool window_file_ok(const WindowFile &d, long w0, long w1, long w2, const int32_t *__restrict__ channels,
                                               int n_ch_sel, int n_ch) {
    bool ok = d.n >= 1 && d.D1 >= 1 && d.D2 >= 1 && d.D1 <= d.n && d.D2 <= d.n / d.D1;
    long D0 = 0;
    if (ok) {
        const long plane = d.D1 * d.D2;                          // <= n: no overflow
        D0 = d.n / plane;
        ok = D0 * plane == d.n;
    }
    // (w >= 1 each: an empty box is not launched)  a + w <= D without forming a + w
    ok = ok && d.a0 >= 0 && w0 <= D0 && d.a0 <= D0 - w0 && d.a1 >= 0 && w1 <= d.D1 && d.a1 <= d.D1 - w1 && d.a2 >= 0 &&
         w2 <= d.D2 && d.a2 <= d.D2 - w2;
    bool ch_ok = true;
    if (channels) {
        for (int i = threadIdx.x; i < n_ch_sel; i += kWinThreads) ch_ok &= channels[i] >= 0 && channels[i] < n_ch;
    } else {
        ch_ok = n_ch_sel <= n_ch;
    }
    return ok && !__any(!ch_ok);
}

// Listed segment g of channel c: false for an id outside [0, nseg) or a size entry outside [0, M) (status bit 5); else the
// entry e of sizes / offs, the segment's first row a and its length.
__device__ __forceinline__ bool window_segment(const WindowFile &d, long g, long c, int seg, long M, long &e, long &a, int &len) {
    const long nseg = (d.n + seg - 1) / seg;
    // entry seg_base + c nseg + g, inside [0, M): g < nseg <= room, then c <= (room - 1 - g) / nseg
    const long room = d.seg_base >= 0 && d.seg_base < M ? M - d.seg_base : 0;
    if (g < 0 || g >= nseg || nseg > room || c > (room - 1 - g) / nseg) return false;
    e = d.seg_base + c * nseg + g;
    a = g * (long)seg;
    len = (int)(a + seg < d.n ? seg : d.n - a);
    return true;
}

// The position of a segment's rows, by increment and carry: one divmod per segment, none per symbol.
struct WindowCursor {
    long i0, i1, i2;
    __device__ __forceinline__ WindowCursor(const WindowFile &d, long a) {
        const long q = a / d.D2;
        i2 = a - q * d.D2;
        i0 = q / d.D1;
        i1 = q - i0 * d.D1;
    }
    // v to the row's place in dst [w0][w1][w2][n_ch_sel] when the row lies inside the box, then on to the next row.
    __device__ __forceinline__ void put(const WindowFile &d, float *__restrict__ dst, float v, long w0, long w1, long w2, int n_ch_sel) {
        // unsigned compares: 0 <= i - a < w; inside the box every index is below the output's extents
        if ((unsigned long)(i0 - d.a0) < (unsigned long)w0 && (unsigned long)(i1 - d.a1) < (unsigned long)w1 &&
            (unsigned long)(i2 - d.a2) < (unsigned long)w2) {
            dst[(((i0 - d.a0) * w1 + (i1 - d.a1)) * w2 + (i2 - d.a2)) * n_ch_sel] = v;
        }
        if (++i2 == d.D2) {
            i2 = 0;
            if (++i1 == d.D1) { i1 = 0; ++i0; }
        }
    }
};

// Untrusted: everything k_rans_decode_window treats so, the palette fields of the descriptor and the class blocks.  Status
// bits per file: 0-3 and 32 as there; 64 a class >= P met while decoding (compared with P before it indexes anything; zeros
// from there on); 128 an inconsistent descriptor or channel list, P outside [1, max_P], a table[p < P] outside [0, n_tables)
// or a cls_base that is neither -1 nor an 8-byte-aligned offset with 8 ceil(n / 32) bytes inside [0, cls_bytes): nothing of
// that file is written.
__global__ void __launch_bounds__(kWinThreads)
k_rans_map_decode_window(const uint16_t *__restrict__ payload, long n_words, const uint16_t *__restrict__ sizes,
                         const int64_t *__restrict__ offs, long M, const int64_t *__restrict__ files,
                         const int32_t *__restrict__ segs, int n_sel, const int32_t *__restrict__ channels, int n_ch_sel, int n_ch,
                         int T, int seg, const uint16_t *__restrict__ freq, int n_tables, const float *__restrict__ values,
                         const uint8_t *__restrict__ cls, long cls_bytes, int max_P, long w0, long w1, long w2,
                         float *__restrict__ out, uint32_t *__restrict__ status) {
    extern __shared__ float map_win_l[];                         // val[2048], then [max_P][kMapCStride] c, [max_P][kMapBuckets] start
    float *val_l = map_win_l;
    uint16_t *c_all = reinterpret_cast<uint16_t *>(map_win_l + kMapT);
    uint16_t *start_all = c_all + max_P * kMapCStride;
    const int lane = threadIdx.x;
    const long f = blockIdx.z;
    const int j = blockIdx.y;                                    // the channel's place in the output
    const int64_t *fd = files + f * kMapFileFields;
    const WindowFile d(fd);
    const long P = fd[7], cls_base = fd[12];
    const long c = channels ? (long)channels[j] : (long)j;

    // ---- the descriptor and the channel list: workgroup-uniform
    bool ok = P >= 1 && P <= max_P;
    for (int p = 0; p < kMapMaxClasses; ++p) ok = ok && (p >= P || (fd[8 + p] >= 0 && fd[8 + p] < n_tables));
    if (cls_base != -1) {
        const long need = 8 * (d.n / 32 + (d.n % 32 != 0));      // (n >= 1 is checked below; no overflow for any n)
        ok = ok && cls_base >= 0 && cls_base % 8 == 0 && need <= cls_bytes && cls_base <= cls_bytes - need;
    }
    if (!window_file_ok(d, w0, w1, w2, channels, n_ch_sel, n_ch) || !ok) {
        if (lane == 0 && status) atomicOr(status + f, 128u);
        return;
    }

    // ---- the tables of (table[p], c), p < P, and the code points of c
    const int Pf = (int)P;
    for (int p = 0; p < Pf; ++p) stage_segment_table<false>(freq + (fd[8 + p] * n_ch + c) * T, T, nullptr, c_all + p * kMapCStride);
    for (int i = lane; i < T; i += kWinThreads) val_l[i] = values[c * T + i];
    __syncthreads();
    bool table_ok = true;
    for (int p = 0; p < Pf; ++p) table_ok &= c_all[p * kMapCStride + T] == (uint16_t)(1u << kPB);
    if (table_ok) {
        for (int t = lane; t < Pf * kMapBuckets; t += kWinThreads) {
            start_all[t] = bucket_start(c_all + (t / kMapBuckets) * kMapCStride, T, 16u * (t % kMapBuckets));
        }
    }
    __syncthreads();

    // ---- this lane's segment
    const long t = (long)blockIdx.x * kWinThreads + lane;
    if (t >= n_sel) return;
    const long g = segs[f * (long)n_sel + t];
    if (g == -1) return;                                         // padding of a shorter list
    long e, a;
    int len;
    if (!window_segment(d, g, c, seg, M, e, a, len)) {
        if (status) atomicOr(status + f, 32u);
        return;
    }
    unsigned bad = table_ok ? 0u : 8u;
    const unsigned k0 = sizes[e];
    const long off = offs[e];
    if (k0 < 2u || k0 > (unsigned)seg + 2u || off < 0 || off > n_words - (long)k0) bad |= 1u;
    SegmentReader rd;
    bool dead = bad != 0u;                                       // bits 0 / 3, starved or a class outside the palette: zeros from here
    if (!dead) rd.open(payload + off, k0);                       // reads stay in [off, off + k0) within [0, n_words)

    // the classes of rows a .. a + len - 1 < n: words a / 32 .. (a + len - 1) / 32 < ceil(n / 32) of the file's block
    const uint64_t *cw = nullptr;
    uint64_t cbits = 0;
    int cleft = 0;                                               // classes left in cbits
    if (cls_base != -1) {
        cw = reinterpret_cast<const uint64_t *>(cls + cls_base) + a / 32;
        cbits = *cw++ >> (2 * (int)(a % 32));
        cleft = 32 - (int)(a % 32);
    }

    WindowCursor at(d, a);
    float *dst = out + f * (w0 * w1 * w2 * n_ch_sel) + j;        // (the product was checked on the host)
    for (int s = 0; s < len; ++s) {
        unsigned p = 0u;
        if (cw) {
            if (cleft == 0) { cbits = *cw++; cleft = 32; }
            p = (unsigned)cbits & 3u;
            cbits >>= 2;
            --cleft;
        }
        float v = 0.0f;
        if (!dead) {
            if (p >= (unsigned)Pf) {
                bad |= 64u;
                dead = true;
            } else {
                v = val_l[rans_pop(rd.x, start_all + p * kMapBuckets, c_all + p * kMapCStride)];
                if (!rd.refill()) { bad |= 2u; dead = true; }
            }
        }
        at.put(d, dst, v, w0, w1, w2, n_ch_sel);
    }
    if (!bad && !rd.clean()) bad |= 4u;
    if (bad && status) atomicOr(status + f, bad);
}

}  // namespace
}  // namespace vbq

extern "C" int vbq_rans_map_decode_window_f32(const uint16_t *d_payload, int64_t n_words, const uint16_t *d_sizes,
                                              const int64_t *d_offsets, int64_t M, const int64_t *d_files, int32_t n_files,
                                              const int32_t *d_segs, int32_t n_sel, const int32_t *d_channels, int32_t n_ch_sel,
                                              int32_t n_ch, int32_t seg, int32_t N, const uint16_t *d_freq, int32_t n_tables,
                                              const float *d_values, const uint8_t *d_cls, int64_t cls_bytes, int32_t max_classes,
                                              int64_t w0, int64_t w1, int64_t w2, float *d_out, uint32_t *d_status, void *stream) {
    using namespace vbq;
    const char *who = "vbq_rans_map_decode_window_f32";
    long long total;                                             // elements of d_out
    if (int r = check_window(who, n_words, M, n_files, n_sel, d_channels != nullptr, n_ch_sel, n_ch, seg, N, n_tables, w0, w1, w2, total))
        return r;
    VBQ_REQUIRE(max_classes >= 1 && max_classes <= kMapMaxClasses, VBQ_ERR_INVALID_ARGUMENT, "%s: max_classes = %d outside [1, %d]",
                who, max_classes, kMapMaxClasses);
    VBQ_REQUIRE(cls_bytes >= 0 && cls_bytes % 8 == 0, VBQ_ERR_INVALID_ARGUMENT,
                "%s: cls_bytes = %lld is not a multiple of 8 bytes >= 0", who, (long long)cls_bytes);
    if (n_files == 0 || n_sel == 0 || n_ch_sel == 0 || total == 0) return VBQ_OK;
    VBQ_REQUIRE(d_sizes && d_offsets && d_files && d_segs && d_freq && d_values && d_out, VBQ_ERR_INVALID_ARGUMENT,
                "%s: null pointer argument", who);
    VBQ_REQUIRE(n_words == 0 || d_payload, VBQ_ERR_INVALID_ARGUMENT, "%s: null d_payload", who);
    VBQ_REQUIRE(cls_bytes == 0 || d_cls, VBQ_ERR_INVALID_ARGUMENT, "%s: null d_cls with cls_bytes = %lld", who, (long long)cls_bytes);
    VBQ_REQUIRE(reinterpret_cast<uintptr_t>(d_cls) % 8 == 0, VBQ_ERR_INVALID_ARGUMENT,
                "%s: d_cls is not aligned to 8 bytes (the class blocks are read in 64-bit words)", who);
    const size_t lds = kMapT * sizeof(float) + (size_t)max_classes * (kMapCStride + kMapBuckets) * sizeof(uint16_t);
    hipLaunchKernelGGL(k_rans_map_decode_window, window_grid(n_sel, n_ch_sel, n_files), dim3(kWinThreads), lds,
                       reinterpret_cast<hipStream_t>(stream), d_payload, (long)n_words, d_sizes, d_offsets, (long)M, d_files, d_segs,
                       (int)n_sel, d_channels, (int)n_ch_sel, (int)n_ch, table_size(N), (int)seg, d_freq, (int)n_tables, d_values,
                       d_cls, (long)cls_bytes, (int)max_classes, (long)w0, (long)w1, (long)w2, d_out, d_status);
    VBQ_CHECK_LAUNCH(who);
    return VBQ_OK;
}
