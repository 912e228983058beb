// Batch sizes of latent files in segments (vbq_amd/bitstream.py, magic "VBQb"): the coded length of every file of a batch at
// every lambda of a list in ONE launch -- rate control for a directory of latents.  The sizes-only counterpart of
// k_rans_encode_files (vbq_rans_files.hip), as k_rans_sizes (vbq_rans.hip) is of k_rans_encode.  Contract: include/vbq.h,
// "Batch sizes".
//
// k_rans_sizes gives a workgroup the 64 consecutive segments of ONE stream: a Kodak-shaped latent at segment 1024 has two
// segments per channel, so 2 of its 64 lanes work.  Here the host lists the work as items (file, segment) in blocks of 64 and a
// workgroup takes one block of one channel at one lambda: its lanes size segments of DIFFERENT files with the one table
// d_freq[lambda][channel] it stages.  Every file is sized at every lambda, so -- unlike the encoder's -- a block's files need
// share nothing.  One lane runs one item in full, last symbol to first, with the state machine and the renormalisation of
// k_rans_sizes and the alignment-independent load order of k_rans_encode_files, and adds its word count to its file's total
// with one 64-bit atomic: integer adds commute, so the totals do not depend on scheduling.  (Lanes of one file are not merged
// before the atomic: a Kodak-shaped file puts 64 adds on a total, spread over 32 workgroups.)
// The constants, the per-symbol step, the table staging and the canon map are vbq_rans_common.h's.
#include "vbq_rans_common.h"

namespace vbq {
namespace {

constexpr int kSizesThreads = 64;                                // one wave: stage_segment_table scans with wave shuffles alone
constexpr int kEncFields = 6;                                    // the batch encoder's descriptor: idx_base, idx_stride, n, ...
constexpr unsigned kBadFile = 128u;                              // status bit 7

// The descriptors and the items come from the caller's host plan; every index formed from them is range-checked without
// overflow before it is used, and an item that fails adds nothing and sets bit 7 of its file's status word.  A lambda's
// symbols are the plane [l stride_l, (l + 1) stride_l) of idx (the host checked n_lambda stride_l <= n_idx): a descriptor is
// checked against [0, stride_l), the same for every lambda and every item of the file.
__global__ void __launch_bounds__(kSizesThreads)
k_rans_sizes_files(const uint16_t *__restrict__ idx, long stride_l, const int64_t *__restrict__ files, int n_files,
                   const int32_t *__restrict__ items, int T, int seg, const uint16_t *__restrict__ freq,
                   const uint16_t *__restrict__ canon, unsigned long long *__restrict__ totals, uint32_t *__restrict__ status) {
    __shared__ uint32_t fc_l[2048];
    const int lane = threadIdx.x;
    const long c = blockIdx.y;                                   // channel
    const long n_ch = gridDim.y;
    const long l = blockIdx.z;                                   // lambda
    const long it = (long)blockIdx.x * kSizesThreads + lane;     // (the host checked n_items % 64 == 0: every lane has an item)
    const long f = items[2 * it], g = items[2 * it + 1];

    // ---- this lane's file: the descriptor as a whole, then the item
    const bool listed = f != -1;                                 // -1: padding of the last block
    const bool known = f >= 0 && f < n_files;
    long idx_base = 0, stride = 0, n = 0;
    bool ok = false;
    if (known) {
        const int64_t *d = files + f * kEncFields;
        idx_base = d[0], stride = d[1], n = d[2];
        // symbols [idx_base + c' stride, + n) of every channel c' inside [0, stride_l), without forming a sum that could overflow
        ok = n >= 1 && n <= stride_l && idx_base >= 0 && idx_base <= stride_l - n && stride >= 0 &&
             (n_ch == 1 || stride <= (stride_l - n - idx_base) / (n_ch - 1));
        ok = ok && g >= 0 && g <= (n - 1) / seg;
    }
    if (listed && !ok && status) atomicOr(status + (known ? f : 0), kBadFile);     // (an unknown file has no word of its own: word 0)
    if (__ballot(ok) == 0ull) return;                            // workgroup-uniform: padding alone, or nothing that can be sized

    stage_segment_table<true>(freq + (l * n_ch + c) * T, T, fc_l, nullptr);
    if (canon) map_segment_table(canon + c * T, T, fc_l);
    __syncthreads();
    if (!ok) return;

    // ---- this lane's segment, as k_rans_sizes counts it
    const long a = g * seg;
    const long b = a + seg < n ? a + seg : n;
    const uint16_t *src = idx + l * stride_l + idx_base + c * stride;
    unsigned x = kRansL;
    int k = 0;
    auto put = [&](unsigned sym) {
        const unsigned fc = fc_l[sym < (unsigned)T ? sym : 0u];  // (an index outside the table: symbol 0, as k_rans_encode)
        const unsigned fr = fc & 0xffffu, cu = fc >> 16;
        if (x >= (fr << (32 - kPB))) { ++k; x >>= 16; }
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
    atomicAdd(totals + l * n_files + f, (unsigned long long)(k + 2));     // + the final state's two words
}

}  // namespace
}  // namespace vbq

extern "C" int vbq_rans_sizes_files_u16(const uint16_t *d_idx, int64_t n_idx, int64_t lambda_stride, const int64_t *d_files,
                                        int32_t n_files, const int32_t *d_items, int64_t n_items, int32_t n_ch, int32_t seg,
                                        int32_t N, const uint16_t *d_freq, int32_t n_lambda, const uint16_t *d_canon,
                                        uint64_t *d_totals, uint32_t *d_status, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n_idx >= 0 && lambda_stride >= 0 && n_files >= 0 && n_files <= 65535 && n_items >= 0 && n_ch >= 0 &&
                    n_ch <= 65535 && seg >= 1 && seg <= 65533 && N >= 1 && N <= 10 && n_lambda >= 1 && n_lambda <= 65535,
                VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_sizes_files_u16: bad sizes n_idx=%lld lambda_stride=%lld n_files=%d n_items=%lld n_ch=%d seg=%d N=%d "
                "n_lambda=%d",
                (long long)n_idx, (long long)lambda_stride, n_files, (long long)n_items, n_ch, seg, N, n_lambda);
    VBQ_REQUIRE(n_items % kSizesThreads == 0, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_sizes_files_u16: n_items=%lld is not a multiple of %d (pad the last block with file -1)",
                (long long)n_items, kSizesThreads);
    VBQ_REQUIRE(n_items / kSizesThreads <= INT32_MAX, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_sizes_files_u16: n_items=%lld items are too many", (long long)n_items);
    VBQ_REQUIRE(lambda_stride <= n_idx / n_lambda, VBQ_ERR_INVALID_ARGUMENT,     // n_lambda * lambda_stride <= n_idx, no product
                "vbq_rans_sizes_files_u16: n_lambda=%d planes of lambda_stride=%lld indices do not fit in n_idx=%lld", n_lambda,
                (long long)lambda_stride, (long long)n_idx);
    if (n_files == 0 || n_items == 0 || n_ch == 0) return VBQ_OK;
    VBQ_REQUIRE(d_idx && d_files && d_items && d_freq && d_totals, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_sizes_files_u16: null pointer argument");
    hipLaunchKernelGGL(k_rans_sizes_files, dim3((unsigned)(n_items / kSizesThreads), (unsigned)n_ch, (unsigned)n_lambda),
                       dim3(kSizesThreads), 0, reinterpret_cast<hipStream_t>(stream), d_idx, (long)lambda_stride, d_files,
                       (int)n_files, d_items, table_size(N), (int)seg, d_freq, d_canon,
                       reinterpret_cast<unsigned long long *>(d_totals), d_status);
    VBQ_CHECK_LAUNCH("rans_sizes_files");
    return VBQ_OK;
}
