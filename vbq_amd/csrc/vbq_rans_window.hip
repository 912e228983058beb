// Window decode of latent files in segments (vbq_amd/bitstream.py, magic "VBQb"): a box of one file, or the same-sized boxes of
// many files, in ONE launch, straight from the packed payloads into channel-last f32 values -- no padded words, no u16 index
// tensor and no full-size Z_hat in between.  The latent-side counterpart of k_rans_decode_values (vbq_rans.hip): a table per
// (file's lambda, channel), several files per launch, the values written where the caller's [F][w0][w1][w2][n_ch_sel] tensor
// wants them.  Contract: include/vbq.h, "Window decode".
//
// One lane decodes one listed segment IN FULL, first symbol to last (a segment is the coder's unit: nothing shorter can be
// decoded, and the end-state check of SegmentReader then holds as in k_rans_decode); it follows its row's position (i0, i1, i2)
// in the file's three-level geometry by increment and carry and stores the symbols that fall inside the box.  The 64 lanes of a
// workgroup belong to one (file, channel) and share its tables in LDS: fc, c, start and the values, 24 KB.  Table staging, the
// bucket table and the rules for untrusted words are vbq_rans_common.h's.
#include "vbq_rans_window_common.h"

namespace vbq {
namespace {

constexpr int kFileFields = 8;                                   // seg_base, n, D1, D2, a0, a1, a2, table

// Untrusted: payload, sizes, offsets (as k_rans_decode_values) and, defensively, the descriptors and the two id lists -- every
// index formed from them is range-checked without overflow before it is used.  Status bits per file: 0-3 as k_rans_decode (a
// segment whose words do not lie in [0, n_words) counts as bit 0), 32 a listed id outside [0, nseg_f) or a size entry outside
// [0, M), 128 an inconsistent descriptor or channel list (nothing of that file is written).
__global__ void __launch_bounds__(kWinThreads)
k_rans_decode_window(const uint16_t *__restrict__ payload, long n_words, const uint16_t *__restrict__ sizes,
                     const int64_t *__restrict__ offs, long M, const int64_t *__restrict__ files,
                     const int32_t *__restrict__ segs, int n_sel, const int32_t *__restrict__ channels, int n_ch_sel, int n_ch,
                     int T, int seg, const uint16_t *__restrict__ freq, int n_tables, const float *__restrict__ values,
                     long w0, long w1, long w2, float *__restrict__ out, uint32_t *__restrict__ status) {
    __shared__ uint32_t fc_l[2048];
    __shared__ uint16_t c_l[2048 + 2];
    __shared__ uint16_t start[(1 << kPB) / 16];                  // start[b] = the symbol whose slot range holds slot 16 b
    __shared__ float val_l[2048];
    const int lane = threadIdx.x;
    const long f = blockIdx.z;
    const int j = blockIdx.y;                                    // the channel's place in the output
    const int64_t *d = files + f * kFileFields;
    const long seg_base = d[0], n = d[1], D1 = d[2], D2 = d[3], a0 = d[4], a1 = d[5], a2 = d[6], table = d[7];
    const long c = channels ? (long)channels[j] : (long)j;

    // ---- the descriptor and the channel list: workgroup-uniform, so the whole workgroup leaves together
    bool ok = n >= 1 && D1 >= 1 && D2 >= 1 && D1 <= n && D2 <= n / D1 && table >= 0 && table < n_tables;
    long D0 = 0;
    if (ok) {
        const long plane = D1 * D2;                              // <= n: no overflow
        D0 = n / plane;
        ok = D0 * plane == n;
    }
    // (w >= 1 each: an empty box is not launched)  a + w <= D without forming a + w
    ok = ok && a0 >= 0 && w0 <= D0 && a0 <= D0 - w0 && a1 >= 0 && w1 <= D1 && a1 <= D1 - w1 && a2 >= 0 && w2 <= D2 && a2 <= D2 - w2;
    bool ch_ok = true;                                           // EVERY listed channel: nothing of the file is written otherwise
    if (channels) {
        for (int i = lane; i < n_ch_sel; i += kWinThreads) ch_ok &= channels[i] >= 0 && channels[i] < n_ch;
    } else {
        ch_ok = n_ch_sel <= n_ch;
    }
    if (!ok || __any(!ch_ok)) {
        if (lane == 0 && status) atomicOr(status + f, 128u);
        return;
    }

    // ---- the tables of (table, c)
    stage_segment_table<true>(freq + ((long)table * n_ch + c) * T, T, fc_l, c_l);
    for (int i = lane; i < T; i += kWinThreads) val_l[i] = values[c * T + i];
    __syncthreads();
    const bool table_ok = c_l[T] == (uint16_t)(1u << kPB);
    if (table_ok) {
        for (int bkt = lane; bkt < (1 << kPB) / 16; bkt += kWinThreads) start[bkt] = bucket_start(c_l, T, 16u * bkt);
    }
    __syncthreads();

    // ---- this lane's segment
    const long t = (long)blockIdx.x * kWinThreads + lane;
    if (t >= n_sel) return;
    const long g = segs[f * (long)n_sel + t];
    if (g == -1) return;                                         // padding of a shorter list
    const long nseg = (n + seg - 1) / seg;
    // entry seg_base + c nseg + g of sizes / offs, inside [0, M): g < nseg <= room, then c <= (room - 1 - g) / nseg
    const long room = seg_base >= 0 && seg_base < M ? M - seg_base : 0;
    if (g < 0 || g >= nseg || nseg > room || c > (room - 1 - g) / nseg) {
        if (status) atomicOr(status + f, 32u);
        return;
    }
    const long e = seg_base + c * nseg + g;
    const long a = g * (long)seg;
    const int len = (int)(a + seg < n ? seg : n - a);
    unsigned bad = table_ok ? 0u : 8u;
    const unsigned k0 = sizes[e];
    const long off = offs[e];
    if (k0 < 2u || k0 > (unsigned)seg + 2u || off < 0 || off > n_words - (long)k0) bad |= 1u;
    SegmentReader rd;
    bool dead = bad != 0u;                                       // bits 0 / 3, or starved later on: zeros from here
    if (!dead) rd.open(payload + off, k0);                       // reads stay in [off, off + k0) within [0, n_words)

    // the position of row a, then by increment and carry: one divmod per segment, none per symbol
    long q = a / D2;
    long i2 = a - q * D2;
    long i0 = q / D1;
    long i1 = q - i0 * D1;
    float *dst = out + f * (w0 * w1 * w2 * n_ch_sel) + j;        // (the product was checked on the host)
    for (int s = 0; s < len; ++s) {
        float v = 0.0f;
        if (!dead) {
            v = val_l[rans_pop(rd.x, start, c_l, fc_l)];
            if (!rd.refill()) { bad |= 2u; dead = true; }
        }
        // unsigned compares: 0 <= i - a < w; inside the box every index is below the output's extents
        if ((unsigned long)(i0 - a0) < (unsigned long)w0 && (unsigned long)(i1 - a1) < (unsigned long)w1 &&
            (unsigned long)(i2 - a2) < (unsigned long)w2) {
            dst[(((i0 - a0) * w1 + (i1 - a1)) * w2 + (i2 - a2)) * n_ch_sel] = v;
        }
        if (++i2 == D2) {
            i2 = 0;
            if (++i1 == D1) { i1 = 0; ++i0; }
        }
    }
    if (!bad && !rd.clean()) bad |= 4u;
    if (bad && status) atomicOr(status + f, bad);
}

}  // namespace
}  // namespace vbq

extern "C" int vbq_rans_decode_window_f32(const uint16_t *d_payload, int64_t n_words, const uint16_t *d_sizes,
                                          const int64_t *d_offsets, int64_t M, const int64_t *d_files, int32_t n_files,
                                          const int32_t *d_segs, int32_t n_sel, const int32_t *d_channels, int32_t n_ch_sel,
                                          int32_t n_ch, int32_t seg, int32_t N, const uint16_t *d_freq, int32_t n_tables,
                                          const float *d_values, int64_t w0, int64_t w1, int64_t w2, float *d_out,
                                          uint32_t *d_status, void *stream) {
    using namespace vbq;
    long long total;                                             // elements of d_out
    if (int r = check_window("vbq_rans_decode_window_f32", n_words, M, n_files, n_sel, d_channels != nullptr, n_ch_sel, n_ch, seg, N,
                             n_tables, w0, w1, w2, total))
        return r;
    if (n_files == 0 || n_sel == 0 || n_ch_sel == 0 || total == 0) return VBQ_OK;
    VBQ_REQUIRE(d_sizes && d_offsets && d_files && d_segs && d_freq && d_values && d_out, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_decode_window_f32: null pointer argument");
    VBQ_REQUIRE(n_words == 0 || d_payload, VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_decode_window_f32: null d_payload");
    hipLaunchKernelGGL(k_rans_decode_window, window_grid(n_sel, n_ch_sel, n_files), dim3(kWinThreads), 0, reinterpret_cast<hipStream_t>(stream), d_payload, (long)n_words, d_sizes, d_offsets,
                       (long)M, d_files, d_segs, (int)n_sel, d_channels, (int)n_ch_sel, (int)n_ch, table_size(N), (int)seg, d_freq,
                       (int)n_tables, d_values, (long)w0, (long)w1, (long)w2, d_out, d_status);
    VBQ_CHECK_LAUNCH("rans_decode_window");
    return VBQ_OK;
}
