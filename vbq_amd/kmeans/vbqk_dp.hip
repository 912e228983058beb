// Exact 1-D k-means of many channels at every level count up to Kmax (include/vbq_kmeans.h, "Exact 1-D k-means"): the DP
//     D[q][j] = min_{i = q..j} D[q-1][i-1] + cost(i, j),   cost(i, j) = (S2[j] - S2[i-1]) - s * s / (j - i + 1),  s = S1[j] - S1[i-1]
// over the prefix sums of the sorted, median-shifted samples, each layer evaluated by the divide-and-conquer recursion the header
// states (the optimal split point is monotone in j), every f64 operation rounded separately.
// One workgroup per channel.  The recursion tree of a layer depends on (q, n) alone: node t of depth d is found by walking d
// halvings from the root [q, n], and its bounds il / ih are the back-pointers at jl - 1 / jh + 1, which are midpoints of its
// ancestors -- so the nodes of one depth are independent, and a layer is bit_length(n - q + 1) rounds with a barrier between them.
// A round has two phases: every lane takes the nodes t = tid, tid + 512, ... and scans the short ones itself; a node whose scan
// holds kDpWaveScan candidates or more goes into an LDS queue, and after a barrier each wave takes queued nodes, lanes over i,
// and reduces to the lowest i among equal minima -- the same index and the same bits as the scan in ascending i.  A full
// queue is no error: the lane scans the node itself.
// gfx950 / ROCm only.
#include <float.h>

#include "vbq_common.h"
#include "vbq_kmeans.h"

namespace vbq {
namespace {

constexpr int kDpThreads = 512;
constexpr int kDpWaves = kDpThreads / kWave;
constexpr int kDpWaveScan = 64;                  // candidates from which a node is scanned by a whole wave: one per lane at least
constexpr int kDpQueue = 2048;                   // queued nodes per round
constexpr int kDpMaxLevels = 64;                 // level counts per launch: one lane of the first wave each
constexpr int kDpMaxK = 1024;
constexpr int64_t kDpMaxN = 1 << 30;             // int indices with room for a loop's last step; a tree of at most 31 depths
constexpr size_t kDpLdsBytes = 160 * 1024;       // LDS of one CU: the most a single workgroup may take
constexpr size_t kDpLdsHead = 16 + sizeof(int) * kDpQueue;      // the two queue counters, the queue
constexpr int kDpWsWgPerCu = 2;                  // workgroups per CU the workspace is sized for

struct DpLevels {
    int k[kDpMaxLevels];
};

struct DpPlan {
    bool rows_in_lds;     // two value rows and the channel's S1, S2 in LDS
    size_t lds_bytes;     // dynamic LDS of one workgroup
    size_t bp_bytes;      // back-pointer bytes of one channel: 4 Kmax (n + 1), rounded up to 16
    size_t slice_bytes;   // workspace of one channel in flight
};

DpPlan dp_plan(int64_t n, int32_t Kmax) {
    DpPlan p;
    const size_t W = (size_t)n + 1;
    p.rows_in_lds = W <= (kDpLdsBytes - kDpLdsHead) / (4 * sizeof(double));
    p.lds_bytes = kDpLdsHead + (p.rows_in_lds ? 4 * W * sizeof(double) : 0);
    p.bp_bytes = ((size_t)Kmax * W * sizeof(int) + 15) & ~(size_t)15;
    p.slice_bytes = p.bp_bytes + (p.rows_in_lds ? 0 : 2 * W * sizeof(double));
    return p;
}

__device__ __forceinline__ bool not_finite(double v) { return !(fabs(v) <= DBL_MAX); }

// Node t of depth d of solve(q, n, ., .): its range [jl, jh], false when the recursion never gets there (an empty range has no
// children).  Bit d-1-s of t says which child step s takes.
__device__ __forceinline__ bool dp_node(int t, int d, int q, int n, int &jl, int &jh) {
    jl = q;
    jh = n;
    for (int b = d - 1; b >= 0; --b) {
        if (jl > jh) return false;
        const int mid = jl + ((jh - jl) >> 1);
        if ((t >> b) & 1) jl = mid + 1;
        else jh = mid - 1;
    }
    return jl <= jh;
}

__device__ __forceinline__ double dp_candidate(const double *Dprev, const double *S1, const double *S2, double s1j, double s2j,
                                               int i, int j) {
    const double a = __dsub_rn(s2j, S2[i - 1]);
    const double s = __dsub_rn(s1j, S1[i - 1]);
    const double c = __dsub_rn(a, __ddiv_rn(__dmul_rn(s, s), (double)(j - i + 1)));
    return __dadd_rn(Dprev[i - 1], c);
}

// The scan bounds of a node: i in [lo, hi], never empty.  A[q][.] >= q, so max(il, q) = il.  Layer 1 has D[0][i-1] = +inf for
// every i > 1: no later candidate is below the first, and the scan is cut to i = 1 (the same D and A, n log n adds fewer).
__device__ __forceinline__ void dp_bounds(const int *Aq, int q, int n, int jl, int jh, int j, int &lo, int &hi) {
    lo = jl > q ? Aq[jl - 1] : q;
    const int ih = jh < n ? Aq[jh + 1] : n;
    hi = ih < j ? ih : j;
    if (q == 1) hi = lo;
}

template <bool kRowsInLds>
__global__ void __launch_bounds__(kDpThreads)
k_kmeans1d(const double *__restrict__ S1g, const double *__restrict__ S2g, const double *__restrict__ shiftg, int n, int C,
           DpLevels lev, int S, int Kmax, int *__restrict__ out_starts, double *__restrict__ out_codes,
           long long *__restrict__ out_counts, double *__restrict__ out_sse, unsigned int *__restrict__ status,
           unsigned char *__restrict__ ws, size_t bp_bytes, size_t slice_bytes) {
    extern __shared__ double lds[];
    int *ctl = reinterpret_cast<int *>(lds);                         // [0], [1]: the queue length of even and odd rounds
    int *queue = ctl + 4;
    double *rows = lds + kDpLdsHead / sizeof(double);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const size_t W = (size_t)n + 1;
    unsigned char *slice = ws + (size_t)blockIdx.x * slice_bytes;
    int *A = reinterpret_cast<int *>(slice);                         // A[q][j] at A[(q - 1) * W + j]
    const double inf = __builtin_huge_val();
    if (tid < 2) ctl[tid] = 0;
    int par = 0;                                                     // which counter this round's lanes push to

    for (int c = blockIdx.x; c < C; c += gridDim.x) {
        const double *S1c = S1g + (size_t)c * W, *S2c = S2g + (size_t)c * W;
        double *Dprev = kRowsInLds ? rows : reinterpret_cast<double *>(slice + bp_bytes);
        double *Dcur = Dprev + W;
        const double *S1 = kRowsInLds ? rows + 2 * W : S1c;
        const double *S2 = kRowsInLds ? rows + 3 * W : S2c;
        for (int j = tid; j <= n; j += kDpThreads) {
            Dprev[j] = j == 0 ? 0.0 : inf;
            if (kRowsInLds) {
                rows[2 * W + j] = S1c[j];
                rows[3 * W + j] = S2c[j];
            }
        }
        const double shift = shiftg[c];
        __threadfence_block();
        __syncthreads();

        for (int q = 1; q <= Kmax; ++q) {
            int *Aq = A + (size_t)(q - 1) * W;
            const int depths = 32 - __clz(n - q + 1);                // bit_length(n - q + 1), n - q + 1 >= 1
            for (int d = 0; d < depths; ++d) {
                const int nodes = 1 << d;
                if (tid == 0) ctl[par ^ 1] = 0;                      // the next round's counter: nobody reads it in this round
                for (int t = tid; t < nodes; t += kDpThreads) {
                    int jl, jh, lo, hi;
                    if (!dp_node(t, d, q, n, jl, jh)) continue;
                    const int j = jl + ((jh - jl) >> 1);
                    dp_bounds(Aq, q, n, jl, jh, j, lo, hi);
                    if (hi - lo + 1 >= kDpWaveScan) {
                        const int slot = atomicAdd(&ctl[par], 1);
                        if (slot < kDpQueue) {
                            queue[slot] = t;
                            continue;
                        }
                    }
                    const double s1j = S1[j], s2j = S2[j];
                    double best = dp_candidate(Dprev, S1, S2, s1j, s2j, lo, j);
                    int bi = lo;
                    for (int i = lo + 1; i <= hi; ++i) {
                        const double v = dp_candidate(Dprev, S1, S2, s1j, s2j, i, j);
                        if (v < best) { best = v; bi = i; }
                    }
                    Dcur[j] = best;
                    Aq[j] = bi;
                }
                __syncthreads();
                const int queued = ctl[par] < kDpQueue ? ctl[par] : kDpQueue;
                for (int e = wave; e < queued; e += kDpWaves) {
                    int jl, jh, lo, hi;
                    dp_node(queue[e], d, q, n, jl, jh);
                    const int j = jl + ((jh - jl) >> 1);
                    dp_bounds(Aq, q, n, jl, jh, j, lo, hi);
                    const double s1j = S1[j], s2j = S2[j];
                    int bi = lo + lane;                              // hi - lo + 1 >= 64: every lane has a candidate
                    double best = dp_candidate(Dprev, S1, S2, s1j, s2j, bi, j);
                    for (int i = bi + kWave; i <= hi; i += kWave) {
                        const double v = dp_candidate(Dprev, S1, S2, s1j, s2j, i, j);
                        if (v < best) { best = v; bi = i; }
                    }
                    for (int m = kWave / 2; m >= 1; m >>= 1) {       // the lowest i among equal minima
                        const double ov = __shfl_xor(best, m);
                        const int oi = __shfl_xor(bi, m);
                        if (ov < best || (ov == best && oi < bi)) { best = ov; bi = oi; }
                    }
                    if (lane == 0) {
                        Dcur[j] = best;
                        Aq[j] = bi;
                    }
                }
                par ^= 1;
                __threadfence_block();
                __syncthreads();
            }
            if (tid == 0) out_sse[(size_t)c * Kmax + (q - 1)] = Dcur[n];
            double *t = Dprev; Dprev = Dcur; Dcur = t;
        }

        if (tid < S) {
            const int k = lev.k[tid];
            size_t at = 0;
            for (int s = 0; s < tid; ++s) at += (size_t)lev.k[s];
            at = at * (size_t)C + (size_t)c * k;                     // the level's slab, then the channel's k entries
            int j = n;
            for (int q = k; q >= 1; --q) {
                const int i = A[(size_t)(q - 1) * W + j];            // q <= i <= j by construction, for any input
                const double m = (double)(j - i + 1);
                out_starts[at + q - 1] = i;
                out_codes[at + q - 1] = __dadd_rn(shift, __ddiv_rn(__dsub_rn(S1[j], S1[i - 1]), m));
                out_counts[at + q - 1] = (long long)(j - i + 1);
                j = i - 1;
            }
        }
        if (tid == 0 && status && (not_finite(S1[n]) || not_finite(S2[n]) || not_finite(shift))) atomicOr(status, 1u);
        __syncthreads();                                             // the slice and the rows are the next channel's
    }
}

template <bool kRowsInLds>
int dp_launch(const char *who, const DpPlan &p, int64_t grid, const double *S1, const double *S2, const double *shift, int64_t n,
              int32_t C, const DpLevels &lev, int32_t S, int32_t Kmax, int32_t *out_starts, double *out_codes, int64_t *out_counts,
              double *out_sse, uint32_t *status, unsigned char *ws, hipStream_t st) {
    if (p.lds_bytes > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(k_kmeans1d<kRowsInLds>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)p.lds_bytes) != hipSuccess)
        (void)hipGetLastError();                                     // the launch below reports what is wrong, if anything
    hipLaunchKernelGGL((k_kmeans1d<kRowsInLds>), dim3((unsigned)grid), dim3(kDpThreads), p.lds_bytes, st, S1, S2, shift, (int)n,
                       (int)C, lev, (int)S, (int)Kmax, out_starts, out_codes, reinterpret_cast<long long *>(out_counts), out_sse,
                       status, ws, p.bp_bytes, p.slice_bytes);
    VBQ_CHECK_LAUNCH(who);
    return VBQ_OK;
}

int dp_check(const char *who, int64_t n, int32_t C, const int32_t *levels, int32_t S) {
    VBQ_REQUIRE(n >= 1 && n <= kDpMaxN && C >= 1, VBQ_ERR_INVALID_ARGUMENT,
                "%s: bad sizes n=%lld C=%d (need 1 <= n <= 2^30, C >= 1)", who, (long long)n, C);
    VBQ_REQUIRE(S >= 1 && S <= kDpMaxLevels, VBQ_ERR_INVALID_ARGUMENT, "%s: S=%d level counts, outside [1, 64]", who, S);
    VBQ_REQUIRE(levels, VBQ_ERR_INVALID_ARGUMENT, "%s: null pointer argument (levels)", who);
    for (int32_t s = 0; s < S; ++s) {
        VBQ_REQUIRE(levels[s] >= 1, VBQ_ERR_INVALID_ARGUMENT, "%s: levels[%d] = %d is below 1", who, s, levels[s]);
        VBQ_REQUIRE(s == 0 || levels[s] > levels[s - 1], VBQ_ERR_INVALID_ARGUMENT,
                    "%s: levels[%d] = %d does not exceed levels[%d] = %d (the level counts must be strictly ascending)", who, s,
                    levels[s], s - 1, levels[s - 1]);
    }
    const int32_t Kmax = levels[S - 1];
    VBQ_REQUIRE(Kmax <= kDpMaxK, VBQ_ERR_INVALID_ARGUMENT, "%s: Kmax = %d level counts, above 1024", who, Kmax);
    VBQ_REQUIRE((int64_t)Kmax <= n, VBQ_ERR_INVALID_ARGUMENT, "%s: Kmax = %d clusters of n = %lld samples (need Kmax <= n)", who, Kmax,
                (long long)n);
    return VBQ_OK;
}

}  // namespace
}  // namespace vbq

#pragma GCC visibility push(default)
extern "C" size_t vbqk_kmeans1d_workspace_bytes(int64_t n, int32_t C, int32_t Kmax) {
    using namespace vbq;
    if (n < 1 || n > kDpMaxN || C < 1 || Kmax < 1 || Kmax > kDpMaxK || (int64_t)Kmax > n) return 0;
    const DpPlan p = dp_plan(n, Kmax);
    const int64_t resident = (int64_t)num_cus() * kDpWsWgPerCu;
    return (size_t)(C < resident ? C : resident) * p.slice_bytes;
}

extern "C" int vbqk_kmeans1d_f64(const double *d_S1, const double *d_S2, const double *d_shift, int64_t n, int32_t C,
                                 const int32_t *levels, int32_t S, int32_t *d_out_starts, double *d_out_codes,
                                 int64_t *d_out_counts, double *d_out_sse, uint32_t *d_status, void *d_workspace,
                                 size_t workspace_bytes, void *stream) {
    using namespace vbq;
    const char *who = "vbqk_kmeans1d_f64";
    if (int rc = dp_check(who, n, C, levels, S)) return rc;
    VBQ_REQUIRE(d_S1 && d_S2 && d_shift && d_out_starts && d_out_codes && d_out_counts && d_out_sse, VBQ_ERR_INVALID_ARGUMENT,
                "%s: null pointer argument", who);
    const int32_t Kmax = levels[S - 1];
    const DpPlan p = dp_plan(n, Kmax);
    VBQ_REQUIRE(d_workspace && workspace_bytes >= p.slice_bytes, VBQ_ERR_WORKSPACE,
                "%s: workspace of %zu bytes holds no channel's slice (%zu bytes each; vbqk_kmeans1d_workspace_bytes gives the "
                "full size)", who, workspace_bytes, p.slice_bytes);
    VBQ_REQUIRE(reinterpret_cast<uintptr_t>(d_workspace) % 16 == 0, VBQ_ERR_WORKSPACE, "%s: workspace not 16-byte aligned", who);
    DpLevels lev = {};
    for (int32_t s = 0; s < S; ++s) lev.k[s] = levels[s];
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // as many workgroups as the workspace has slices, each walking over its share of the channels
    int64_t grid = (int64_t)(workspace_bytes / p.slice_bytes);
    const int64_t resident = (int64_t)num_cus() * kDpWsWgPerCu;
    if (grid > resident) grid = resident;
    if (grid > C) grid = C;
    unsigned char *ws = static_cast<unsigned char *>(d_workspace);
    if (p.rows_in_lds)
        return dp_launch<true>(who, p, grid, d_S1, d_S2, d_shift, n, C, lev, S, Kmax, d_out_starts, d_out_codes, d_out_counts,
                               d_out_sse, d_status, ws, st);
    return dp_launch<false>(who, p, grid, d_S1, d_S2, d_shift, n, C, lev, S, Kmax, d_out_starts, d_out_codes, d_out_counts,
                            d_out_sse, d_status, ws, st);
}
#pragma GCC visibility pop
