// Planned boxes (vbq_store.h): file ids and box origins that live on the device -> the descriptors and segment lists of the
// window decoders of vbq.h.  One 64-lane wave per sample, four samples per workgroup.  The box of a sample is w0 w1 runs of w2
// consecutive rows; lanes take runs in chunks of 64, a run's segments that no earlier run listed are
// max(lo_r, hi_{r-1} + 1) .. hi_r, and a wave-wide inclusive scan of the counts places them.  Ids and origins are untrusted: a
// sample is checked before anything is derived from it, and an invalid one reads row 0 of the table and nothing else.
// gfx950 / ROCm only.
#include "vbq_common.h"
#include "vbq_store.h"

namespace vbq {
namespace {

constexpr int kPlanThreads = 256;
constexpr int kPlanWaves = kPlanThreads / 64;
constexpr int64_t kPlanMaxGrid = 1 << 20;
constexpr unsigned kPlanCut = 32, kPlanBadSample = 128;          // status bits 5 and 7, as the decoders mean them

__global__ void __launch_bounds__(kPlanThreads)
k_plan_boxes(const long long *__restrict__ table, int n_files, int fields, const long long *__restrict__ ids,
             const long long *__restrict__ origins, long long S, long long w0, long long w1, long long w2, int seg, int n_sel,
             long long *__restrict__ desc, int *__restrict__ segs, unsigned *__restrict__ status) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long s = (long long)blockIdx.x * kPlanWaves + wave; s < S; s += (long long)gridDim.x * kPlanWaves) {
        const long long id = ids[s];
        const long long a0 = origins[3 * s], a1 = origins[3 * s + 1], a2 = origins[3 * s + 2];
        const bool in_range = id >= 0 && id < n_files;
        const long long *trow = table + (in_range ? id : 0) * fields;
        const long long n = trow[1], D1 = trow[2], D2 = trow[3];
        bool ok = in_range && n >= 0 && D1 >= 1 && D2 >= 1;
        if (ok) ok = D1 <= 0x7fffffffffffffffLL / D2;
        long long D0 = 0;
        if (ok) {
            const long long plane = D1 * D2;
            D0 = n / plane;
            ok = D0 * plane == n && (n == 0 ? 0 : (n - 1) / seg + 1) <= 0x7fffffffLL;
        }
        if (ok) ok = a0 >= 0 && a0 <= D0 - w0 && a1 >= 0 && a1 <= D1 - w1 && a2 >= 0 && a2 <= D2 - w2;
        unsigned bits = ok ? 0u : kPlanBadSample;
        if (lane < fields) {
            long long v = (ok ? trow : table)[lane];
            if (lane >= 4 && lane <= 6) v = !ok ? 0 : lane == 4 ? a0 : lane == 5 ? a1 : a2;
            desc[s * fields + lane] = v;
        }
        int *list = segs + s * n_sel;
        long long pos = 0;                                       // entries of the list so far; may pass n_sel, writes do not
        if (ok) {
            const long long R = w0 * w1;                         // <= D0 D1 <= n
            long long hi_before = -1;                            // hi of the run before this chunk's first
            for (long long r0 = 0; r0 < R; r0 += 64) {
                const long long r = r0 + lane;
                const bool active = r < R;
                long long lo = 0, hi = 0;
                if (active) {
                    const long long q = r / w1;
                    const long long first = ((a0 + q) * D1 + a1 + (r - q * w1)) * D2 + a2;
                    lo = first / seg;
                    hi = (first + w2 - 1) / seg;
                }
                long long hi_prev = __shfl_up(hi, 1);
                if (lane == 0) hi_prev = hi_before;
                long long start = 0;
                int count = 0;
                if (active) {
                    start = lo > hi_prev + 1 ? lo : hi_prev + 1;
                    count = (int)(hi - start + 1);               // >= 0: hi is non-decreasing in r
                }
                int incl = count;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int t = __shfl_up(incl, d);
                    if (lane >= d) incl += t;
                }
                const long long base = pos + incl - count;
                for (int j = 0; j < count && base + j < n_sel; ++j) list[base + j] = (int)(start + j);
                pos += __shfl(incl, 63);
                hi_before = __shfl(hi, 63);                      // read only when another chunk follows: lane 63 was active
            }
            if (pos > n_sel) bits |= kPlanCut;
        }
        for (long long p = (pos < n_sel ? pos : n_sel) + lane; p < n_sel; p += 64) list[p] = -1;
        if (bits && lane == 0) status[s] |= bits;
    }
}

}  // namespace
}  // namespace vbq

#pragma GCC visibility push(default)
extern "C" int vbqs_plan_boxes(const int64_t *d_table, int32_t n_files, int32_t fields, const int64_t *d_ids,
                               const int64_t *d_origins, int64_t S, int64_t w0, int64_t w1, int64_t w2, int32_t seg, int32_t n_sel,
                               int64_t *d_desc, int32_t *d_segs, uint32_t *d_status, void *stream) {
    using namespace vbq;
    const char *who = "vbqs_plan_boxes";
    VBQ_REQUIRE(fields == 8 || fields == 16, VBQ_ERR_INVALID_ARGUMENT, "%s: fields=%d (a descriptor has 8 or 16)", who, fields);
    VBQ_REQUIRE(n_files >= 1 && S >= 0 && w0 >= 0 && w1 >= 0 && w2 >= 0 && n_sel >= 0, VBQ_ERR_INVALID_ARGUMENT,
                "%s: bad arguments n_files=%d S=%lld box=%lld x %lld x %lld n_sel=%d (need n_files >= 1, every other size >= 0)",
                who, n_files, (long long)S, (long long)w0, (long long)w1, (long long)w2, n_sel);
    VBQ_REQUIRE(seg >= 1 && seg <= 65533, VBQ_ERR_INVALID_ARGUMENT, "%s: seg=%d outside 1..65533", who, seg);
    VBQ_REQUIRE(d_table && d_ids && d_origins && d_desc && d_segs && d_status, VBQ_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    if (S == 0 || w0 == 0 || w1 == 0 || w2 == 0 || n_sel == 0) return VBQ_OK;
    int64_t grid = S / kPlanWaves + (S % kPlanWaves != 0);
    if (grid > kPlanMaxGrid) grid = kPlanMaxGrid;
    hipLaunchKernelGGL(k_plan_boxes, dim3((unsigned)grid), dim3(kPlanThreads), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const long long *>(d_table), (int)n_files, (int)fields,
                       reinterpret_cast<const long long *>(d_ids), reinterpret_cast<const long long *>(d_origins), (long long)S,
                       (long long)w0, (long long)w1, (long long)w2, (int)seg, (int)n_sel, reinterpret_cast<long long *>(d_desc),
                       d_segs, d_status);
    VBQ_CHECK_LAUNCH(who);
    return VBQ_OK;
}
#pragma GCC visibility pop
