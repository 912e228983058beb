// Batch encode of lambda-map files (vbq_amd/bitstream.py, magic "VBQm"): every segment of every file of a batch in ONE launch,
// into the padded slots vbq_rans_pack_u16 then packs for all files at once.  k_rans_encode_files (vbq_rans_files.hip) with a
// table per symbol, as k_rans_map_encode (vbq_rans_map.hip) is k_rans_encode with one.  Contract: include/vbq.h, "Mapped batch
// encode".
//
// k_rans_map_encode gives a workgroup the 64 consecutive segments of ONE stream and stages up to four tables for them: a
// Kodak-shaped latent at segment 1024 has two segments per channel, so 2 of its 64 lanes work.  Here the host lists the work as
// items (file, segment) in blocks of 64 that share a PALETTE (an ordered list of 1..4 tables: the lambdas of the files' classes)
// and a workgroup takes one block of one channel: it stages the palette's tables once and its lanes code segments of DIFFERENT
// files, each following its own file's class bytes.  One lane codes one item in full, last symbol to first: the words and the
// size of a segment are those of k_rans_map_encode.  The constants, the per-symbol step, the table staging and the canon map
// are vbq_rans_common.h's; the walk of a lane over its segment is vbq_rans_map_common.h's.
#include "vbq_rans_map_common.h"

namespace vbq {
namespace {

constexpr int kMapFilesThreads = 64;                             // one wave: stage_segment_table scans with wave shuffles alone
constexpr int kMapEncFields = 8;                                 // idx_base, idx_stride, plane_stride, n, seg_base, palette, cls_base, reserved
constexpr unsigned kBadMapFile = 128u;                           // status bit 7

struct MapFilesArgs {
    const uint16_t *idx;                                         // [n_idx]
    const uint8_t *cls;                                          // [n_cls]
    const int64_t *files;                                        // [n_files][kMapEncFields]
    const int32_t *palettes;                                     // [n_palettes][kMapMaxClasses]
    const int32_t *items;                                        // [n_items][2]
    const uint16_t *freq;                                        // [n_tables][n_ch][T]
    const uint16_t *canon;                                       // [n_ch][T] or null
    uint16_t *words;                                             // [M][seg + 2], unused by the sizes kernel
    uint32_t *sizes;                                             // [M]
    uint32_t *status;                                            // [n_files] or null
    long n_idx, n_cls, M;
    int n_files, n_palettes, n_tables, max_classes, T, seg;
};

// kWords: the encoder; otherwise the sizes kernel (the same state machine over the same symbols in the same order, counting).
// The descriptors, the palettes and the items come from the caller's host plan; every index formed from them is range-checked
// without overflow before it is used, and an item that fails writes nothing and sets bit 7 of its file's status word.  The
// checks of a descriptor (palette, index range, class range, slot range) come out the same for every item of the file, so
// nothing of such a file is written; a segment id outside the file, or an item in a block of another palette, refuses that item
// alone.
template <bool kWords>
__global__ void __launch_bounds__(kMapFilesThreads) k_rans_map_encode_files(const MapFilesArgs a) {
    extern __shared__ uint32_t map_files_fc_l[];                 // [P of the block's palette][kMapT]
    const int lane = threadIdx.x;
    const long c = blockIdx.y;                                   // channel
    const long n_ch = gridDim.y;
    const int T = a.T, seg = a.seg;
    const long it = (long)blockIdx.x * kMapFilesThreads + lane;  // (the host checked n_items % 64 == 0: every lane has an item)
    const long f = a.items[2 * it], g = a.items[2 * it + 1];

    // ---- this lane's file: the descriptor as a whole, then the item
    const bool listed = f != -1;                                 // -1: padding of a palette's last block
    const bool known = f >= 0 && f < a.n_files;
    long idx_base = 0, stride = 0, plane = 0, n = 0, seg_base = 0, pal = -1, cls_base = 0, nseg = 0;
    int P = 0;
    bool ok = false;
    if (known) {
        const int64_t *d = a.files + f * kMapEncFields;
        idx_base = d[0], stride = d[1], plane = d[2], n = d[3], seg_base = d[4], pal = d[5], cls_base = d[6];
        if (pal < 0 || pal >= a.n_palettes) pal = -1;
        if (pal >= 0) {
            // P: the entries before the first -1; every one of them a table, and no more of them than the launch has LDS for
            const int32_t *row = a.palettes + pal * kMapMaxClasses;
            bool fine = true;
            for (P = 0; P < kMapMaxClasses; ++P) {
                const int t = row[P];
                if (t == -1) break;
                fine = fine && t >= 0 && t < a.n_tables;
            }
            if (!fine || P < 1 || P > a.max_classes) pal = -1;
        }
        // symbols [idx_base + p plane + c' stride, + n) of every plane p < P and every channel c' inside [0, n_idx), the classes
        // [cls_base, + n) inside [0, n_cls), without forming a sum that could overflow
        ok = pal >= 0 && n >= 1 && n <= a.n_idx && idx_base >= 0 && idx_base <= a.n_idx - n && stride >= 0 && plane >= 0 &&
             n <= a.n_cls && cls_base >= 0 && cls_base <= a.n_cls - n;
        if (ok) {
            long room = a.n_idx - n - idx_base;
            ok = P == 1 || plane <= room / (P - 1);
            if (ok) {
                room -= (P - 1) * plane;
                ok = n_ch == 1 || stride <= room / (n_ch - 1);
            }
        }
        if (ok) {
            nseg = (n - 1) / seg + 1;
            // slots [seg_base, seg_base + n_ch nseg) inside [0, M)
            ok = seg_base >= 0 && seg_base <= a.M && nseg <= (a.M - seg_base) / n_ch;
        }
    }

    // ---- the block's palette: that of its first item whose file names a valid one
    const unsigned long long has = __ballot(pal >= 0);
    if (has == 0ull) {                                           // workgroup-uniform: padding alone, or nothing that can be coded
        if (listed && a.status) atomicOr(a.status + (known ? f : 0), kBadMapFile);
        return;
    }
    const int first = __ffsll((long long)has) - 1;
    const long block_pal = __shfl((int)pal, first, 64);
    const int block_P = __shfl(P, first, 64);
    for (int p = 0; p < block_P; ++p) {
        const long t = a.palettes[block_pal * kMapMaxClasses + p];
        stage_segment_table<true>(a.freq + (t * n_ch + c) * T, T, map_files_fc_l + p * kMapT, nullptr);
    }
    if (a.canon)
        for (int p = 0; p < block_P; ++p) map_segment_table(a.canon + c * T, T, map_files_fc_l + p * kMapT);
    __syncthreads();

    if (!listed) return;
    if (!known || !ok || pal != block_pal || g < 0 || g >= nseg) {
        if (a.status) atomicOr(a.status + (known ? f : 0), kBadMapFile);   // (an unknown file has no word of its own: word 0)
        return;
    }

    // ---- this lane's segment, as k_rans_map_encode codes it
    const long lo = g * seg;
    const long hi = lo + seg < n ? lo + seg : n;
    const uint16_t *src = a.idx + idx_base + c * stride;         // plane 0 of this channel of this file
    const uint8_t *cl = a.cls + cls_base;
    const long slot = seg_base + c * nseg + g;
    uint16_t *out = kWords ? a.words + slot * (long)(seg + 2) : nullptr;
    unsigned x = kRansL;
    int k = 0;
    auto put = [&](unsigned sym, unsigned p) {                   // p < P
        const unsigned fc = map_files_fc_l[p * kMapT + (sym < (unsigned)T ? sym : 0u)];   // (an index outside the table: symbol 0)
        const unsigned fr = fc & 0xffffu, cu = fc >> 16;
        if (x >= (fr << (32 - kPB))) {
            if (kWords) out[k] = (uint16_t)(x & 0xffffu);
            ++k;
            x >>= 16;
        }
        x = rans_push(x, fr, cu);
    };
    // (the order of the symbols and the width of the loads: map_segment_walk, shared with the rates kernel)
    map_segment_walk(cl, lo, hi, P, [&](unsigned p) { return src + p * plane; }, put);
    if (kWords) {
        out[k] = (uint16_t)(x & 0xffffu);
        out[k + 1] = (uint16_t)(x >> 16);
    }
    a.sizes[slot] = (uint32_t)(k + 2);                           // + the final state's two words
}

template <bool kWords>
int map_encode_files(const char *who, const uint16_t *d_idx, int64_t n_idx, const uint8_t *d_cls, int64_t n_cls,
                     const int64_t *d_files, int32_t n_files, const int32_t *d_palettes, int32_t n_palettes, int32_t max_classes,
                     const int32_t *d_items, int64_t n_items, int32_t n_ch, int32_t seg, int32_t N, const uint16_t *d_freq,
                     int32_t n_tables, const uint16_t *d_canon, uint16_t *d_words, uint32_t *d_sizes, int64_t M,
                     uint32_t *d_status, void *stream) {
    VBQ_REQUIRE(n_idx >= 0 && n_cls >= 0 && n_files >= 0 && n_files <= 65535 && n_palettes >= 1 && max_classes >= 1 &&
                    max_classes <= kMapMaxClasses && n_items >= 0 && n_ch >= 0 && n_ch <= 65535 && seg >= 1 && seg <= 65533 &&
                    N >= 1 && N <= 10 && n_tables >= 1 && M >= 0,
                VBQ_ERR_INVALID_ARGUMENT,
                "%s: bad sizes n_idx=%lld n_cls=%lld n_files=%d n_palettes=%d max_classes=%d n_items=%lld n_ch=%d seg=%d N=%d "
                "n_tables=%d M=%lld",
                who, (long long)n_idx, (long long)n_cls, n_files, n_palettes, max_classes, (long long)n_items, n_ch, seg, N,
                n_tables, (long long)M);
    VBQ_REQUIRE(n_items % kMapFilesThreads == 0, VBQ_ERR_INVALID_ARGUMENT,
                "%s: n_items=%lld is not a multiple of %d (pad every palette's last block with file -1)", who,
                (long long)n_items, kMapFilesThreads);
    VBQ_REQUIRE(n_items / kMapFilesThreads <= INT32_MAX && M <= INT64_MAX / (2 * ((int64_t)seg + 2)), VBQ_ERR_INVALID_ARGUMENT,
                "%s: n_items=%lld items or M=%lld slots are too many", who, (long long)n_items, (long long)M);
    if (n_files == 0 || n_items == 0 || n_ch == 0) return VBQ_OK;
    VBQ_REQUIRE(d_idx && d_cls && d_files && d_palettes && d_items && d_freq && d_sizes && (d_words || !kWords),
                VBQ_ERR_INVALID_ARGUMENT, "%s: null pointer argument", who);
    MapFilesArgs a = {};
    a.idx = d_idx;
    a.cls = d_cls;
    a.files = d_files;
    a.palettes = d_palettes;
    a.items = d_items;
    a.freq = d_freq;
    a.canon = d_canon;
    a.words = d_words;
    a.sizes = d_sizes;
    a.status = d_status;
    a.n_idx = (long)n_idx;
    a.n_cls = (long)n_cls;
    a.M = (long)M;
    a.n_files = n_files;
    a.n_palettes = n_palettes;
    a.n_tables = n_tables;
    a.max_classes = max_classes;
    a.T = table_size(N);
    a.seg = seg;
    hipLaunchKernelGGL(k_rans_map_encode_files<kWords>, dim3((unsigned)(n_items / kMapFilesThreads), (unsigned)n_ch),
                       dim3(kMapFilesThreads), (size_t)max_classes * kMapT * sizeof(uint32_t),
                       reinterpret_cast<hipStream_t>(stream), a);
    VBQ_CHECK_LAUNCH(who);
    return VBQ_OK;
}

}  // namespace
}  // namespace vbq

extern "C" int vbq_rans_map_encode_files_u16(const uint16_t *d_idx, int64_t n_idx, const uint8_t *d_cls, int64_t n_cls,
                                             const int64_t *d_files, int32_t n_files, const int32_t *d_palettes,
                                             int32_t n_palettes, int32_t max_classes, const int32_t *d_items, int64_t n_items,
                                             int32_t n_ch, int32_t seg, int32_t N, const uint16_t *d_freq, int32_t n_tables,
                                             const uint16_t *d_canon, uint16_t *d_words, uint32_t *d_sizes, int64_t M,
                                             uint32_t *d_status, void *stream) {
    return vbq::map_encode_files<true>("vbq_rans_map_encode_files_u16", d_idx, n_idx, d_cls, n_cls, d_files, n_files, d_palettes,
                                       n_palettes, max_classes, d_items, n_items, n_ch, seg, N, d_freq, n_tables, d_canon, d_words,
                                       d_sizes, M, d_status, stream);
}

extern "C" int vbq_rans_map_sizes_files_u16(const uint16_t *d_idx, int64_t n_idx, const uint8_t *d_cls, int64_t n_cls,
                                            const int64_t *d_files, int32_t n_files, const int32_t *d_palettes,
                                            int32_t n_palettes, int32_t max_classes, const int32_t *d_items, int64_t n_items,
                                            int32_t n_ch, int32_t seg, int32_t N, const uint16_t *d_freq, int32_t n_tables,
                                            const uint16_t *d_canon, uint32_t *d_sizes, int64_t M, uint32_t *d_status,
                                            void *stream) {
    return vbq::map_encode_files<false>("vbq_rans_map_sizes_files_u16", d_idx, n_idx, d_cls, n_cls, d_files, n_files, d_palettes,
                                        n_palettes, max_classes, d_items, n_items, n_ch, seg, N, d_freq, n_tables, d_canon,
                                        nullptr, d_sizes, M, d_status, stream);
}
