// Batch encode of latent files in segments (vbq_amd/bitstream.py, magic "VBQb"): every segment of every file of a batch in ONE
// launch, into the padded slots vbq_rans_pack_u16 then packs for all files at once.  The writer's counterpart of
// k_rans_decode_window (vbq_rans_window.hip).  Contract: include/vbq.h, "Batch encode".
//
// k_rans_encode (vbq_rans.hip) gives a workgroup the 64 consecutive segments of ONE stream: a Kodak-shaped latent at segment
// 1024 has two segments per channel, so 2 of its 64 lanes work.  Here the host lists the work as items (file, segment) in blocks
// of 64 that share a frequency table (a lambda) and a workgroup takes one block of one channel: its lanes code segments of
// DIFFERENT files with the one table it stages.  One lane codes one item in full, last symbol to first, with the state machine,
// the renormalisation and the final-state flush of k_rans_encode: the words and the size of a segment are the same.
// The constants, the per-symbol step, the table staging and the canon map are vbq_rans_common.h's.
#include "vbq_rans_common.h"

namespace vbq {
namespace {

constexpr int kFilesThreads = 64;                                // one wave: stage_segment_table scans with wave shuffles alone
constexpr int kEncFields = 6;                                    // idx_base, idx_stride, n, seg_base, table, reserved
constexpr unsigned kBadFile = 128u;                              // status bit 7

// The descriptors and the items come from the caller's host plan; every index formed from them is range-checked without
// overflow before it is used, and an item that fails writes nothing and sets bit 7 of its file's status word.  The checks of a
// descriptor (table, index range, slot range) come out the same for every item of the file, so nothing of such a file is
// written; a segment id outside the file, or an item in a block of another table, refuses that item alone.
__global__ void __launch_bounds__(kFilesThreads)
k_rans_encode_files(const uint16_t *__restrict__ idx, long n_idx, const int64_t *__restrict__ files, int n_files,
                    const int32_t *__restrict__ items, int T, int seg, const uint16_t *__restrict__ freq, int n_tables,
                    const uint16_t *__restrict__ canon, uint16_t *__restrict__ words, uint32_t *__restrict__ sizes, long M,
                    uint32_t *__restrict__ status) {
    __shared__ uint32_t fc_l[2048];
    const int lane = threadIdx.x;
    const long c = blockIdx.y;                                   // channel
    const long n_ch = gridDim.y;
    const long it = (long)blockIdx.x * kFilesThreads + lane;     // (the host checked n_items % 64 == 0: every lane has an item)
    const long f = items[2 * it], g = items[2 * it + 1];

    // ---- this lane's file: the descriptor as a whole, then the item
    const bool listed = f != -1;                                 // -1: padding of a table's last block
    const bool known = f >= 0 && f < n_files;
    long idx_base = 0, stride = 0, n = 0, seg_base = 0, table = -1, nseg = 0;
    bool ok = false;
    if (known) {
        const int64_t *d = files + f * kEncFields;
        idx_base = d[0], stride = d[1], n = d[2], seg_base = d[3], table = d[4];
        if (table < 0 || table >= n_tables) table = -1;
        // symbols [idx_base + c' stride, + n) of every channel c' inside [0, n_idx), without forming a sum that could overflow
        ok = table >= 0 && n >= 1 && n <= n_idx && idx_base >= 0 && idx_base <= n_idx - n && stride >= 0 &&
             (n_ch == 1 || stride <= (n_idx - n - idx_base) / (n_ch - 1));
        if (ok) {
            nseg = (n - 1) / seg + 1;
            // slots [seg_base, seg_base + n_ch nseg) inside [0, M)
            ok = seg_base >= 0 && seg_base <= M && nseg <= (M - seg_base) / n_ch;
        }
    }

    // ---- the block's table: that of its first item whose file names one
    const unsigned long long has = __ballot(table >= 0);
    if (has == 0ull) {                                           // workgroup-uniform: padding alone, or nothing that can be coded
        if (listed && status) atomicOr(status + (known ? f : 0), kBadFile);
        return;
    }
    const long block_table = __shfl((int)table, __ffsll((long long)has) - 1, 64);
    stage_segment_table<true>(freq + (block_table * n_ch + c) * T, T, fc_l, nullptr);
    if (canon) map_segment_table(canon + c * T, T, fc_l);
    __syncthreads();

    if (!listed) return;
    if (!known || !ok || table != block_table || g < 0 || g >= nseg) {
        if (status) atomicOr(status + (known ? f : 0), kBadFile);     // (an unknown file has no word of its own: word 0)
        return;
    }

    // ---- this lane's segment, as k_rans_encode codes it
    const long a = g * seg;
    const long b = a + seg < n ? a + seg : n;
    const uint16_t *src = idx + idx_base + c * stride;
    const long slot = seg_base + c * nseg + g;
    uint16_t *out = words + slot * (long)(seg + 2);
    unsigned x = kRansL;
    int k = 0;
    auto put = [&](unsigned sym) {
        const unsigned fc = fc_l[sym < (unsigned)T ? sym : 0u];  // (an index outside the table: symbol 0, as k_rans_encode)
        const unsigned fr = fc & 0xffffu, cu = fc >> 16;
        if (x >= (fr << (32 - kPB))) { out[k++] = (uint16_t)(x & 0xffffu); x >>= 16; }
        x = rans_push(x, fr, cu);
    };
    long i = b;
    // the tail down to a 16-byte boundary by 2-byte loads, then eight symbols per 16-byte load, then the head: the same symbols
    // in the same order whatever the alignment of the segment
    while (i > a && reinterpret_cast<uintptr_t>(src + i) % 16 != 0) put(src[--i]);
    for (; i - 8 >= a; i -= 8) {
        const uint4 v = *reinterpret_cast<const uint4 *>(src + i - 8);
        put(v.w >> 16); put(v.w & 0xffffu); put(v.z >> 16); put(v.z & 0xffffu);
        put(v.y >> 16); put(v.y & 0xffffu); put(v.x >> 16); put(v.x & 0xffffu);
    }
    for (--i; i >= a; --i) put(src[i]);
    out[k++] = (uint16_t)(x & 0xffffu);
    out[k++] = (uint16_t)(x >> 16);
    sizes[slot] = (uint32_t)k;
}

}  // namespace
}  // namespace vbq

extern "C" int vbq_rans_encode_files_u16(const uint16_t *d_idx, int64_t n_idx, const int64_t *d_files, int32_t n_files,
                                         const int32_t *d_items, int64_t n_items, int32_t n_ch, int32_t seg, int32_t N,
                                         const uint16_t *d_freq, int32_t n_tables, const uint16_t *d_canon, uint16_t *d_words,
                                         uint32_t *d_sizes, int64_t M, uint32_t *d_status, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n_idx >= 0 && n_files >= 0 && n_files <= 65535 && n_items >= 0 && n_ch >= 0 && n_ch <= 65535 && seg >= 1 &&
                    seg <= 65533 && N >= 1 && N <= 10 && n_tables >= 1 && M >= 0,
                VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_encode_files_u16: bad sizes n_idx=%lld n_files=%d n_items=%lld n_ch=%d seg=%d N=%d n_tables=%d M=%lld",
                (long long)n_idx, n_files, (long long)n_items, n_ch, seg, N, n_tables, (long long)M);
    VBQ_REQUIRE(n_items % kFilesThreads == 0, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_encode_files_u16: n_items=%lld is not a multiple of %d (pad every table's last block with file -1)",
                (long long)n_items, kFilesThreads);
    VBQ_REQUIRE(n_items / kFilesThreads <= INT32_MAX && M <= INT64_MAX / (2 * ((int64_t)seg + 2)), VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_encode_files_u16: n_items=%lld items or M=%lld slots are too many", (long long)n_items, (long long)M);
    if (n_files == 0 || n_items == 0 || n_ch == 0) return VBQ_OK;
    VBQ_REQUIRE(d_idx && d_files && d_items && d_freq && d_words && d_sizes, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_encode_files_u16: null pointer argument");
    hipLaunchKernelGGL(k_rans_encode_files, dim3((unsigned)(n_items / kFilesThreads), (unsigned)n_ch), dim3(kFilesThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), d_idx, (long)n_idx, d_files, (int)n_files, d_items, table_size(N),
                       (int)seg, d_freq, (int)n_tables, d_canon, d_words, d_sizes, (long)M, d_status);
    VBQ_CHECK_LAUNCH("rans_encode_files");
    return VBQ_OK;
}
