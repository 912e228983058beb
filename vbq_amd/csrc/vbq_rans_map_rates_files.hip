// Batch rates of lambda-map files (vbq_amd/bitstream.py, magic "VBQm"): the coded length of every file of a batch under every
// palette of a list of candidates in ONE launch -- rate control over lambda maps.  k_rans_sizes_files
// (vbq_rans_sizes_files.hip) with a table per symbol, and the sizes form of k_rans_map_encode_files (vbq_rans_map_files.hip)
// with a candidate axis in its grid.  Contract: include/vbq.h, "Mapped batch rates".
//
// The caller solves every distinct lambda of its candidates once into one plane of indices per lambda and lists the work as
// items (file, segment) in blocks of 64.  A workgroup takes one block of one channel under one candidate k: it stages the P
// tables d_freq[d_palettes[k][p]][channel] and its lanes size segments of DIFFERENT files, each following its own file's class
// bytes: the class of a symbol picks both the lambda plane the symbol is read from and the table it is coded with.  Every file
// is sized under every candidate, so a block's files need share nothing.  One lane runs one item in full with the walk of
// vbq_rans_map_common.h and adds its word count to its (candidate, file) total with one 64-bit atomic: integer adds commute,
// so the totals do not depend on scheduling.  The constants, the per-symbol step, the table staging and the canon map are
// vbq_rans_common.h's.
#include "vbq_rans_map_common.h"

namespace vbq {
namespace {

constexpr int kMapRatesThreads = 64;                             // one wave: stage_segment_table scans with wave shuffles alone
constexpr int kMapRatesFields = 8;                               // the mapped batch encoder's descriptor
constexpr unsigned kBadMapRatesFile = 128u;                      // status bit 7

struct MapRatesArgs {
    const uint16_t *idx;                                         // [n_idx]: n_lambda planes of stride_l indices
    const uint8_t *cls;                                          // [n_cls]
    const int64_t *files;                                        // [n_files][kMapRatesFields]
    const int32_t *palettes;                                     // [gridDim.z][kMapMaxClasses]
    const int32_t *items;                                        // [n_items][2]
    const uint16_t *freq;                                        // [n_lambda][n_ch][T]
    const uint16_t *canon;                                       // [n_ch][T] or null
    unsigned long long *totals;                                  // [gridDim.z][n_files]
    uint32_t *status;                                            // [n_files] or null
    long stride_l, room, n_cls;                                  // room = n_idx - (n_lambda - 1) stride_l: what a file may span
    int n_files, n_lambda, max_classes, T, seg;
};

// The descriptors, the candidate rows and the items come from the caller's host plan; every index formed from them is
// range-checked without overflow before it is used, and an item that fails adds nothing and sets bit 7 of its file's status
// word.  A file's symbols at plane t are idx[t stride_l + idx_base + c' stride + i]: the host checked n_lambda stride_l <=
// n_idx, so they lie inside [0, n_idx) for every plane t < n_lambda and every channel c' exactly when idx_base + (n_ch - 1)
// stride + n <= room.
__global__ void __launch_bounds__(kMapRatesThreads) k_rans_map_rates_files(const MapRatesArgs a) {
    extern __shared__ uint32_t map_rates_fc_l[];                 // [P of the candidate][kMapT]
    const int lane = threadIdx.x;
    const long c = blockIdx.y;                                   // channel
    const long n_ch = gridDim.y;
    const long cand = blockIdx.z;                                // candidate palette
    const int T = a.T, seg = a.seg;
    const long it = (long)blockIdx.x * kMapRatesThreads + lane;  // (the host checked n_items % 64 == 0: every lane has an item)
    const long f = a.items[2 * it], g = a.items[2 * it + 1];

    // ---- the candidate, workgroup-uniform.  P: the entries before the first -1; every one of them a plane, and no more of
    // them than the launch has LDS for
    const int32_t *row = a.palettes + cand * kMapMaxClasses;
    int P;
    bool fine = true;
    for (P = 0; P < kMapMaxClasses; ++P) {
        const int t = row[P];
        if (t == -1) break;
        fine = fine && t >= 0 && t < a.n_lambda;
    }
    fine = fine && P >= 1 && P <= a.max_classes;

    // ---- this lane's file: the descriptor as a whole, then the item
    const bool listed = f != -1;                                 // -1: padding of the last block
    const bool known = f >= 0 && f < a.n_files;
    long idx_base = 0, stride = 0, n = 0, cls_base = 0;
    bool ok = false;
    if (known) {
        const int64_t *d = a.files + f * kMapRatesFields;
        idx_base = d[0], stride = d[1], n = d[3], cls_base = d[6];
        // symbols [idx_base + c' stride, + n) of every channel c' inside [0, room), the classes [cls_base, + n) inside
        // [0, n_cls), without forming a sum that could overflow
        ok = n >= 1 && n <= a.room && idx_base >= 0 && idx_base <= a.room - n && stride >= 0 &&
             (n_ch == 1 || stride <= (a.room - n - idx_base) / (n_ch - 1)) && n <= a.n_cls && cls_base >= 0 &&
             cls_base <= a.n_cls - n;
        ok = ok && g >= 0 && g <= (n - 1) / seg;
    }
    ok = ok && fine;                                             // (a defective candidate refuses every listed file of its blocks)
    if (listed && !ok && a.status) atomicOr(a.status + (known ? f : 0), kBadMapRatesFile);   // (an unknown file: word 0)
    if (__ballot(ok) == 0ull) return;                            // workgroup-uniform: padding alone, or nothing that can be sized

    // (some lane is ok, so the candidate is fine: 1 <= P <= max_classes entries, every one in [0, n_lambda))
    const long t0 = row[0], t1 = P > 1 ? row[1] : 0, t2 = P > 2 ? row[2] : 0, t3 = P > 3 ? row[3] : 0;   // its planes, class 0 first
    for (int p = 0; p < P; ++p)
        stage_segment_table<true>(a.freq + ((long)row[p] * n_ch + c) * T, T, map_rates_fc_l + p * kMapT, nullptr);
    if (a.canon)
        for (int p = 0; p < P; ++p) map_segment_table(a.canon + c * T, T, map_rates_fc_l + p * kMapT);
    __syncthreads();
    if (!ok) return;

    // ---- this lane's segment, as k_rans_map_encode_files sizes it
    const long lo = g * seg;
    const long hi = lo + seg < n ? lo + seg : n;
    const uint16_t *src = a.idx + idx_base + c * stride;         // plane 0 of this channel of this file
    const long stride_l = a.stride_l;
    unsigned x = kRansL;
    int k = 0;
    auto put = [&](unsigned sym, unsigned p) {                   // p < P
        const unsigned fc = map_rates_fc_l[p * kMapT + (sym < (unsigned)T ? sym : 0u)];   // (an index outside the table: symbol 0)
        const unsigned fr = fc & 0xffffu, cu = fc >> 16;
        if (x >= (fr << (32 - kPB))) { ++k; x >>= 16; }
        x = rans_push(x, fr, cu);
    };
    auto plane_of = [&](unsigned p) { return src + (p == 0 ? t0 : p == 1 ? t1 : p == 2 ? t2 : t3) * stride_l; };
    map_segment_walk(a.cls + cls_base, lo, hi, P, plane_of, put);
    atomicAdd(a.totals + cand * a.n_files + f, (unsigned long long)(k + 2));     // + the final state's two words
}

}  // namespace
}  // namespace vbq

extern "C" int vbq_rans_map_rates_files_u16(const uint16_t *d_idx, int64_t n_idx, int64_t lambda_stride, const uint8_t *d_cls,
                                            int64_t n_cls, const int64_t *d_files, int32_t n_files, const int32_t *d_palettes,
                                            int32_t n_palettes, int32_t max_classes, const int32_t *d_items, int64_t n_items,
                                            int32_t n_ch, int32_t seg, int32_t N, const uint16_t *d_freq, int32_t n_lambda,
                                            const uint16_t *d_canon, uint64_t *d_totals, uint32_t *d_status, void *stream) {
    using namespace vbq;
    const char *who = "vbq_rans_map_rates_files_u16";
    VBQ_REQUIRE(n_idx >= 0 && lambda_stride >= 0 && n_cls >= 0 && n_files >= 0 && n_files <= 65535 && n_palettes >= 1 &&
                    n_palettes <= 65535 && max_classes >= 1 && max_classes <= kMapMaxClasses && n_items >= 0 && n_ch >= 0 &&
                    n_ch <= 65535 && seg >= 1 && seg <= 65533 && N >= 1 && N <= 10 && n_lambda >= 1 && n_lambda <= 65535,
                VBQ_ERR_INVALID_ARGUMENT,
                "%s: bad sizes n_idx=%lld lambda_stride=%lld n_cls=%lld n_files=%d n_palettes=%d max_classes=%d n_items=%lld "
                "n_ch=%d seg=%d N=%d n_lambda=%d",
                who, (long long)n_idx, (long long)lambda_stride, (long long)n_cls, n_files, n_palettes, max_classes,
                (long long)n_items, n_ch, seg, N, n_lambda);
    VBQ_REQUIRE(n_items % kMapRatesThreads == 0, VBQ_ERR_INVALID_ARGUMENT,
                "%s: n_items=%lld is not a multiple of %d (pad the last block with file -1)", who, (long long)n_items,
                kMapRatesThreads);
    VBQ_REQUIRE(n_items / kMapRatesThreads <= INT32_MAX, VBQ_ERR_INVALID_ARGUMENT, "%s: n_items=%lld items are too many", who,
                (long long)n_items);
    VBQ_REQUIRE(lambda_stride <= n_idx / n_lambda, VBQ_ERR_INVALID_ARGUMENT,     // n_lambda * lambda_stride <= n_idx, no product
                "%s: n_lambda=%d planes of lambda_stride=%lld indices do not fit in n_idx=%lld", who, n_lambda,
                (long long)lambda_stride, (long long)n_idx);
    if (n_files == 0 || n_items == 0 || n_ch == 0) return VBQ_OK;
    VBQ_REQUIRE(d_idx && d_cls && d_files && d_palettes && d_items && d_freq && d_totals, VBQ_ERR_INVALID_ARGUMENT,
                "%s: null pointer argument", who);
    MapRatesArgs a = {};
    a.idx = d_idx;
    a.cls = d_cls;
    a.files = d_files;
    a.palettes = d_palettes;
    a.items = d_items;
    a.freq = d_freq;
    a.canon = d_canon;
    a.totals = reinterpret_cast<unsigned long long *>(d_totals);
    a.status = d_status;
    a.stride_l = (long)lambda_stride;
    a.room = (long)(n_idx - (int64_t)(n_lambda - 1) * lambda_stride);            // (the product is at most n_idx)
    a.n_cls = (long)n_cls;
    a.n_files = n_files;
    a.n_lambda = n_lambda;
    a.max_classes = max_classes;
    a.T = table_size(N);
    a.seg = seg;
    hipLaunchKernelGGL(k_rans_map_rates_files, dim3((unsigned)(n_items / kMapRatesThreads), (unsigned)n_ch, (unsigned)n_palettes),
                       dim3(kMapRatesThreads), (size_t)max_classes * kMapT * sizeof(uint32_t),
                       reinterpret_cast<hipStream_t>(stream), a);
    VBQ_CHECK_LAUNCH(who);
    return VBQ_OK;
}
