// Exact fixed-bit-budget allocation over the coordinates of a row (img-compression/utils.py:106-160, encode_mode_dp) and the
// patience scan of the Lagrangian encoder beside it (utils.py:163-208, encode_mode).  Both work on a table of per-level scores
// fhat[n][e] = "the best score of element e when it gets exactly n bits", float64 as in the reference, and never see the
// caller's squash / unsquash / f: those are evaluated where the caller defined them.
//   k_budget_dp      one workgroup per row; the DP runs over the coordinates k with lanes over the budget n:
//                        T[0][n] = fhat(0, n) (n <= N), -inf (n > N)
//                        T[k][n] = max_{m = 0..min(n, N)} fhat(k, m) + T[k-1][n-m]        one rounded add per candidate,
//                    the first maximum in ascending m (np.argmax at :137).  Two value rows [budget+1] and the current
//                    coordinate's N+1 scores live in LDS (the next coordinate's scores are loaded while this one is solved);
//                    one byte of back-pointer per (k, n) lives in LDS when K * (budget+1) fits beside them, else in a slice of
//                    the caller's workspace, one slice per resident workgroup.  Lane 0 walks the back-pointers; coordinate 0
//                    takes the remainder (:156).
//   k_budget_patience  per element: g_0 = fhat_0, g_b = fhat_b - lamb * b; a strict improvement resets the counter, `patience`
//                    non-improvements in a row end the scan (:186-203).
// gfx950 / ROCm only.
#include <float.h>

#include "vbq_common.h"

namespace vbq {
namespace {

constexpr int kBudgetMaxN = 52;                  // one byte per back-pointer, N+1 staging lanes inside one wave
constexpr size_t kBudgetLdsBytes = 160 * 1024;   // LDS of one CU: the most a single workgroup may take
constexpr int kBudgetWsWgPerCu = 2;              // resident workgroups per CU the workspace is sized for

struct BudgetPlan {
    int threads;          // 64, 128 or 256: lanes over n
    size_t lds_bytes;     // dynamic LDS of one workgroup
    size_t bp_row_bytes;  // back-pointer bytes of one row (K * (budget+1), rounded up to 16)
    bool bp_in_lds;
    bool ok;              // false: even the value rows do not fit
};

BudgetPlan budget_plan(int32_t K, int32_t N, int32_t budget) {
    BudgetPlan p;
    const size_t W = (size_t)budget + 1;
    p.threads = W <= 64 ? 64 : (W <= 128 ? 128 : 256);
    const size_t values = (2 * W + 2 * (size_t)(N + 1)) * sizeof(double) + 16;        // + the row's flag word
    p.bp_row_bytes = ((size_t)K * W + 15) & ~(size_t)15;
    p.ok = values <= kBudgetLdsBytes;
    p.bp_in_lds = p.ok && values + p.bp_row_bytes <= kBudgetLdsBytes;
    p.lds_bytes = values + (p.bp_in_lds ? p.bp_row_bytes : 0);
    return p;
}

__device__ __forceinline__ bool outside_contract(double v) { return !(v <= DBL_MAX); }      // NaN or +inf

template <bool kBpInLds>
__global__ void __launch_bounds__(256)
k_budget_dp(const double *__restrict__ fhat, long n_rows, int K, int N, int budget, int *__restrict__ out_bits,
            double *__restrict__ out_obj, unsigned int *__restrict__ status, unsigned char *__restrict__ ws, size_t bp_row_bytes) {
    extern __shared__ double lds[];
    const int W = budget + 1;
    const int tid = threadIdx.x, nt = blockDim.x;
    double *Ta = lds, *Tb = lds + W;
    double *fbuf = lds + 2 * (size_t)W;                              // [2][N+1]
    int *flag = reinterpret_cast<int *>(fbuf + 2 * (N + 1));         // 16 bytes reserved
    unsigned char *bp = kBpInLds ? reinterpret_cast<unsigned char *>(flag + 4) : ws + (size_t)blockIdx.x * bp_row_bytes;
    const long E = n_rows * K;
    const double ninf = -__builtin_huge_val();

    for (long r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const double *frow = fhat + r * K;                           // fhat(k, n) = frow[n * E + k]
        if (tid == 0) *flag = 0;
        double fnext = 0.0;
        if (tid <= N) fnext = frow[(long)tid * E];
        __syncthreads();
        if (tid <= N) {
            fbuf[tid] = fnext;
            if (outside_contract(fnext)) *flag = 1;
            if (K > 1) fnext = frow[(long)tid * E + 1];
        }
        __syncthreads();
        for (int n = tid; n < W; n += nt) Ta[n] = n <= N ? fbuf[n] : ninf;
        double *Tprev = Ta, *Tcur = Tb;
        for (int k = 1; k < K; ++k) {
            double *f = fbuf + (k & 1) * (N + 1);
            if (tid <= N) {
                f[tid] = fnext;
                if (outside_contract(fnext)) *flag = 1;
            }
            __syncthreads();
            if (tid <= N && k + 1 < K) fnext = frow[(long)tid * E + k + 1];
            unsigned char *bpk = bp + (size_t)k * W;
            for (int n = tid; n < W; n += nt) {
                const int top = n < N ? n : N;
                double best = __dadd_rn(f[0], Tprev[n]);
                int bm = 0;
                for (int m = 1; m <= top; ++m) {
                    const double v = __dadd_rn(f[m], Tprev[n - m]);
                    if (v > best) { best = v; bm = m; }
                }
                Tcur[n] = best;
                bpk[n] = (unsigned char)bm;
            }
            double *t = Tprev; Tprev = Tcur; Tcur = t;
        }
        if (!kBpInLds) __threadfence_block();
        __syncthreads();
        if (tid == 0) {
            out_obj[r] = Tprev[budget];
            const int bad = *flag;
            int n = budget;
            int *bits = out_bits + r * K;
            for (int k = K - 1; k >= 1; --k) {
                const int m = bp[(size_t)k * W + n];                 // <= min(n, N) by construction: n never goes below 0
                bits[k] = m;
                n -= m;
            }
            // the remainder (utils.py:156).  It is <= N whenever a finite allocation exists; a row outside the contract still
            // gets bits in [0, N]
            bits[0] = (bad && n > N) ? N : n;
            if (bad && status) atomicOr(status, 1u);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256)
k_budget_patience(const double *__restrict__ fhat, long E, int N, double lamb, int patience, int *__restrict__ out_bits,
                  double *__restrict__ out_g) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (long)gridDim.x * blockDim.x) {
        double best = -__builtin_huge_val();
        int best_b = 0, bad = 0;
        for (int b = 0; b <= N; ++b) {
            const double fb = fhat[(long)b * E + e];
            const double g = b == 0 ? fb : __dsub_rn(fb, __dmul_rn(lamb, (double)b));
            if (g > best) { best = g; best_b = b; bad = 0; }
            else if (++bad == patience) break;
        }
        out_bits[e] = best_b;
        out_g[e] = best;
    }
}

int budget_check(const char *who, int64_t n_rows, int32_t K, int32_t N, int32_t budget) {
    VBQ_REQUIRE(n_rows >= 0 && K >= 1 && N >= 0 && N <= kBudgetMaxN, VBQ_ERR_INVALID_ARGUMENT,
                "%s: bad sizes n_rows=%lld K=%d N=%d (need K >= 1, 0 <= N <= 52)", who, (long long)n_rows, K, N);
    VBQ_REQUIRE(budget >= 0 && (int64_t)budget <= (int64_t)K * N, VBQ_ERR_INVALID_ARGUMENT,
                "%s: budget %d outside [0, K*N = %lld]", who, budget, (long long)K * N);
    return VBQ_OK;
}

}  // namespace
}  // namespace vbq

extern "C" size_t vbq_budget_dp_workspace_bytes(int64_t n_rows, int32_t K, int32_t N, int32_t budget) {
    using namespace vbq;
    if (n_rows <= 0 || K < 1 || N < 0 || N > kBudgetMaxN || budget < 0 || (int64_t)budget > (int64_t)K * N) return 0;
    const BudgetPlan p = budget_plan(K, N, budget);
    if (!p.ok || p.bp_in_lds) return 0;
    const int64_t resident = (int64_t)num_cus() * kBudgetWsWgPerCu;
    return (size_t)(n_rows < resident ? n_rows : resident) * p.bp_row_bytes;
}

extern "C" int vbq_budget_dp_f64(const double *d_fhat, int64_t n_rows, int32_t K, int32_t N, int32_t budget, int32_t *d_out_bits,
                                 double *d_out_obj, uint32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream) {
    using namespace vbq;
    if (int rc = budget_check("vbq_budget_dp_f64", n_rows, K, N, budget)) return rc;
    if (n_rows == 0) return VBQ_OK;
    VBQ_REQUIRE(d_fhat && d_out_bits && d_out_obj, VBQ_ERR_INVALID_ARGUMENT, "vbq_budget_dp_f64: null pointer argument");
    const BudgetPlan p = budget_plan(K, N, budget);
    VBQ_REQUIRE(p.ok, VBQ_ERR_UNSUPPORTED, "vbq_budget_dp_f64: two value rows of budget+1 = %lld float64 do not fit the LDS",
                (long long)budget + 1);
    VBQ_REQUIRE(p.bp_in_lds || (d_workspace && workspace_bytes >= p.bp_row_bytes), VBQ_ERR_WORKSPACE,
                "vbq_budget_dp_f64: workspace of %zu bytes holds no row's back-pointers (%zu bytes each; "
                "vbq_budget_dp_workspace_bytes gives the full size)", workspace_bytes, p.bp_row_bytes);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int64_t grid = n_rows < (1 << 20) ? n_rows : (1 << 20);          // the rest of the rows: the kernel's row loop
    if (p.bp_in_lds) {
        if (p.lds_bytes > 64 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void *>(k_budget_dp<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)p.lds_bytes) != hipSuccess)
            (void)hipGetLastError();                                 // the launch below reports what is wrong, if anything
        hipLaunchKernelGGL(k_budget_dp<true>, dim3((unsigned)grid), dim3(p.threads), p.lds_bytes, st, d_fhat, (long)n_rows, (int)K,
                           (int)N, (int)budget, d_out_bits, d_out_obj, d_status, (unsigned char *)nullptr, p.bp_row_bytes);
    } else {
        // as many workgroups as the workspace has slices, each walking over its share of the rows
        const int64_t slices = (int64_t)(workspace_bytes / p.bp_row_bytes);
        const int64_t resident = (int64_t)num_cus() * kBudgetWsWgPerCu;
        if (grid > slices) grid = slices;
        if (grid > resident) grid = resident;
        // the value rows alone pass 64 KiB from budget + 1 = 4085 (N = 10) on
        if (p.lds_bytes > 64 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void *>(k_budget_dp<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)p.lds_bytes) != hipSuccess)
            (void)hipGetLastError();
        hipLaunchKernelGGL(k_budget_dp<false>, dim3((unsigned)grid), dim3(p.threads), p.lds_bytes, st, d_fhat, (long)n_rows, (int)K,
                           (int)N, (int)budget, d_out_bits, d_out_obj, d_status, static_cast<unsigned char *>(d_workspace),
                           p.bp_row_bytes);
    }
    VBQ_CHECK_LAUNCH("budget_dp");
    return VBQ_OK;
}

extern "C" int vbq_budget_patience_f64(const double *d_fhat, int64_t E, int32_t N, double lamb, int32_t patience,
                                       int32_t *d_out_bits, double *d_out_g, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(E >= 0 && N >= 0 && patience >= 1, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_budget_patience_f64: bad sizes E=%lld N=%d patience=%d", (long long)E, N, patience);
    if (E == 0) return VBQ_OK;
    VBQ_REQUIRE(d_fhat && d_out_bits && d_out_g, VBQ_ERR_INVALID_ARGUMENT, "vbq_budget_patience_f64: null pointer argument");
    int64_t gx = (E + 255) / 256;
    if (gx > 4096) gx = 4096;
    hipLaunchKernelGGL(k_budget_patience, dim3((unsigned)gx), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_fhat, (long)E,
                       (int)N, lamb, (int)patience, d_out_bits, d_out_g);
    VBQ_CHECK_LAUNCH("budget_patience");
    return VBQ_OK;
}
