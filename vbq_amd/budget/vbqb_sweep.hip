// The budget DP of vbq_budget.hip (img-compression/utils.py:106-160, encode_mode_dp) at many budgets in one forward pass
// (include/vbq_budget.h, "Budget sweep").  The recurrence
//     T[0][n] = fhat(0, n) (n <= N), -inf (n > N)
//     T[k][n] = max_{m = 0..min(n, N)} fhat(k, m) + T[k-1][n-m]        one rounded add per candidate, first maximum in ascending m
// does not depend on the budget: k_budget_sweep runs it over n = 0..width-1 exactly as k_budget_dp does (the same adds in the
// same order, so every T and every back-pointer has the same bits), and then
//   * lanes n < curve_len store the last value row T[K-1][n]: the optimal objective at every budget;
//   * lane s < S walks the back-pointers from n = budgets[s], as lane 0 of k_budget_dp does from its one budget.
// One workgroup per row, 64 / 128 / 256 lanes over n; two value rows and the double-buffered scores of a coordinate in LDS; a
// byte of back-pointer per (k, n) in LDS when it fits, else in a workspace slice per resident workgroup.  A curve-only pass
// (S == 0) keeps no back-pointers at all.
// The walks' stores: lane s's words out_bits[s][r][k] lie n_rows * K words apart across lanes, so a step of the walks is S
// scattered 4-byte stores.  They stay that way.  Staging the walks' bits as bytes in an LDS tile [S][K] and copying the tile out
// with coalesced stores was built and measured against this on an MI355X ([100000, 100], N = 10, medians of 10, three
// alternating rounds): 6 budgets 100..600 43.11 ms staged against 42.86 ms direct, 1 budget 43.03 against 42.93, 6 budgets
// 50..300 15.40 against 15.30, 64 budgets 44.42 against 45.34 -- within 0.6 % where users are, 2 % the other way at 64 budgets:
// the walks do not show beside the forward pass, and the tile (with a second path for a remainder that is no byte) is not kept.
// gfx950 / ROCm only.
#include <float.h>

#include "vbq_common.h"
#include "vbq_budget.h"

namespace vbq {
namespace {

constexpr int kSweepMaxN = 52;                   // one byte per back-pointer, N+1 staging lanes inside one wave
constexpr int kSweepMaxS = 64;                   // budgets per launch: one lane of the first wave each
constexpr size_t kSweepLdsBytes = 160 * 1024;    // LDS of one CU: the most a single workgroup may take
constexpr int kSweepWsWgPerCu = 2;               // resident workgroups per CU the workspace is sized for

struct SweepBudgets {
    int b[kSweepMaxS];
};

struct SweepPlan {
    int threads;          // 64, 128 or 256: lanes over n
    size_t lds_bytes;     // dynamic LDS of one workgroup
    size_t bp_row_bytes;  // back-pointer bytes of one row (K * width, rounded up to 16)
    bool bp_in_lds;
    bool ok;              // false: even the value rows do not fit
};

// S == 0: a curve-only pass.  Whether the back-pointers live in LDS depends on (K, N, width) alone, as in k_budget_dp's plan.
SweepPlan sweep_plan(int32_t K, int32_t N, int32_t width, int32_t S) {
    SweepPlan p;
    const size_t W = (size_t)width;
    p.threads = W <= 64 ? 64 : (W <= 128 ? 128 : 256);
    const size_t values = (2 * W + 2 * (size_t)(N + 1)) * sizeof(double) + 16;        // + the row's flag word
    p.bp_row_bytes = ((size_t)K * W + 15) & ~(size_t)15;
    p.ok = values <= kSweepLdsBytes;
    p.bp_in_lds = p.ok && values + p.bp_row_bytes <= kSweepLdsBytes;
    p.lds_bytes = values + (S > 0 && p.bp_in_lds ? p.bp_row_bytes : 0);
    return p;
}

__device__ __forceinline__ bool outside_contract(double v) { return !(v <= DBL_MAX); }      // NaN or +inf

// kTrace: budgets are walked (S >= 1); false is the curve-only pass.  W = width, W > every budget and W >= curve_len.
template <bool kTrace, bool kBpInLds>
__global__ void __launch_bounds__(256)
k_budget_sweep(const double *__restrict__ fhat, long n_rows, int K, int N, int W, SweepBudgets bud, int S,
               int *__restrict__ out_bits, double *__restrict__ out_obj, double *__restrict__ curve, int curve_len,
               unsigned int *__restrict__ status, unsigned char *__restrict__ ws, size_t bp_row_bytes) {
    extern __shared__ double lds[];
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
                if (kTrace) bpk[n] = (unsigned char)bm;
            }
            double *t = Tprev; Tprev = Tcur; Tcur = t;
        }
        if (kTrace && !kBpInLds) __threadfence_block();
        __syncthreads();
        for (int n = tid; n < curve_len; n += nt) curve[r * curve_len + n] = Tprev[n];
        if (kTrace) {
            const int bad = *flag;
            if (tid < S) {
                const int budget = bud.b[tid];
                const long row = (long)tid * n_rows + r;             // of out_obj [S][n_rows] and out_bits [S][n_rows][K]
                out_obj[row] = Tprev[budget];
                int n = budget;
                int *bits = out_bits + row * K;
                for (int k = K - 1; k >= 1; --k) {
                    const int m = bp[(size_t)k * W + n];             // <= min(n, N) by construction: n never goes below 0
                    bits[k] = m;
                    n -= m;
                }
                // the remainder (utils.py:156).  It is <= N whenever a finite allocation exists; a row outside the contract
                // still gets bits in [0, N]
                bits[0] = (bad && n > N) ? N : n;
            }
            if (tid == 0 && bad && status) atomicOr(status, 1u);
        } else if (tid == 0 && *flag && status) {
            atomicOr(status, 1u);
        }
        __syncthreads();
    }
}

int sweep_check(const char *who, int64_t n_rows, int32_t K, int32_t N, const int32_t *budgets, int32_t S, int32_t curve_len) {
    VBQ_REQUIRE(n_rows >= 0 && K >= 1 && N >= 0 && N <= kSweepMaxN, VBQ_ERR_INVALID_ARGUMENT,
                "%s: bad sizes n_rows=%lld K=%d N=%d (need n_rows >= 0, K >= 1, 0 <= N <= 52)", who, (long long)n_rows, K, N);
    VBQ_REQUIRE(S >= 0 && S <= kSweepMaxS, VBQ_ERR_INVALID_ARGUMENT, "%s: S=%d budgets, outside [0, 64]", who, S);
    const int64_t KN = (int64_t)K * N;
    VBQ_REQUIRE(curve_len >= 0 && (int64_t)curve_len <= KN + 1, VBQ_ERR_INVALID_ARGUMENT,
                "%s: curve_len %d outside [0, K*N + 1 = %lld]", who, curve_len, (long long)KN + 1);
    VBQ_REQUIRE(S == 0 || budgets, VBQ_ERR_INVALID_ARGUMENT, "%s: null pointer argument (budgets, with S=%d)", who, S);
    for (int32_t s = 0; s < S; ++s) {
        VBQ_REQUIRE(budgets[s] >= 0 && (int64_t)budgets[s] <= KN, VBQ_ERR_INVALID_ARGUMENT,
                    "%s: budgets[%d] = %d outside [0, K*N = %lld]", who, s, budgets[s], (long long)KN);
        VBQ_REQUIRE(s == 0 || budgets[s] > budgets[s - 1], VBQ_ERR_INVALID_ARGUMENT,
                    "%s: budgets[%d] = %d does not exceed budgets[%d] = %d (the budgets must be strictly ascending)", who, s,
                    budgets[s], s - 1, budgets[s - 1]);
    }
    return VBQ_OK;
}

template <bool kTrace, bool kBpInLds>
int sweep_launch(const char *who, const SweepPlan &p, int64_t grid, const double *fhat, int64_t n_rows, int32_t K, int32_t N,
                 int32_t width, const SweepBudgets &bud, int32_t S, int32_t *out_bits, double *out_obj, double *curve,
                 int32_t curve_len, uint32_t *status, unsigned char *ws, hipStream_t st) {
    if (p.lds_bytes > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(k_budget_sweep<kTrace, kBpInLds>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes) != hipSuccess)
        (void)hipGetLastError();                                     // the launch below reports what is wrong, if anything
    hipLaunchKernelGGL((k_budget_sweep<kTrace, kBpInLds>), dim3((unsigned)grid), dim3(p.threads), p.lds_bytes, st, fhat,
                       (long)n_rows, (int)K, (int)N, (int)width, bud, (int)S, out_bits, out_obj, curve,
                       (int)curve_len, status, ws, p.bp_row_bytes);
    VBQ_CHECK_LAUNCH(who);
    return VBQ_OK;
}

}  // namespace
}  // namespace vbq

#pragma GCC visibility push(default)
extern "C" size_t vbqb_budget_sweep_workspace_bytes(int64_t n_rows, int32_t K, int32_t N, int32_t width) {
    using namespace vbq;
    if (n_rows <= 0 || K < 1 || N < 0 || N > kSweepMaxN || width < 1 || (int64_t)width > (int64_t)K * N + 1) return 0;
    const SweepPlan p = sweep_plan(K, N, width, 1);
    if (!p.ok || p.bp_in_lds) return 0;
    const int64_t resident = (int64_t)num_cus() * kSweepWsWgPerCu;
    return (size_t)(n_rows < resident ? n_rows : resident) * p.bp_row_bytes;
}

extern "C" int vbqb_budget_sweep_f64(const double *d_fhat, int64_t n_rows, int32_t K, int32_t N, const int32_t *budgets, int32_t S,
                                     int32_t *d_out_bits, double *d_out_obj, double *d_curve, int32_t curve_len,
                                     uint32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream) {
    using namespace vbq;
    const char *who = "vbqb_budget_sweep_f64";
    if (int rc = sweep_check(who, n_rows, K, N, budgets, S, curve_len)) return rc;
    if (n_rows == 0 || (S == 0 && curve_len == 0)) return VBQ_OK;
    VBQ_REQUIRE(d_fhat && (S == 0 || (d_out_bits && d_out_obj)), VBQ_ERR_INVALID_ARGUMENT, "%s: null pointer argument", who);
    VBQ_REQUIRE((d_curve != nullptr) == (curve_len > 0), VBQ_ERR_INVALID_ARGUMENT,
                "%s: curve_len %d with d_curve %s (a curve needs both, no curve neither)", who, curve_len,
                d_curve ? "given" : "null");
    const int32_t top = S ? budgets[S - 1] + 1 : 0;
    const int32_t width = top > curve_len ? top : curve_len;
    const SweepPlan p = sweep_plan(K, N, width, S);
    VBQ_REQUIRE(p.ok, VBQ_ERR_UNSUPPORTED, "%s: two value rows of width = %d float64 do not fit the LDS", who, width);
    const bool in_ws = S > 0 && !p.bp_in_lds;
    VBQ_REQUIRE(!in_ws || (d_workspace && workspace_bytes >= p.bp_row_bytes), VBQ_ERR_WORKSPACE,
                "%s: workspace of %zu bytes holds no row's back-pointers (%zu bytes each; "
                "vbqb_budget_sweep_workspace_bytes gives the full size)", who, workspace_bytes, p.bp_row_bytes);
    SweepBudgets bud = {};
    for (int32_t s = 0; s < S; ++s) bud.b[s] = budgets[s];
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int64_t grid = n_rows < (1 << 20) ? n_rows : (1 << 20);          // the rest of the rows: the kernel's row loop
    if (S == 0)
        return sweep_launch<false, true>(who, p, grid, d_fhat, n_rows, K, N, width, bud, S, nullptr, nullptr, d_curve, curve_len,
                                         d_status, nullptr, st);
    if (!in_ws)
        return sweep_launch<true, true>(who, p, grid, d_fhat, n_rows, K, N, width, bud, S, d_out_bits, d_out_obj, d_curve,
                                        curve_len, d_status, nullptr, st);
    // as many workgroups as the workspace has slices, each walking over its share of the rows
    const int64_t slices = (int64_t)(workspace_bytes / p.bp_row_bytes);
    const int64_t resident = (int64_t)num_cus() * kSweepWsWgPerCu;
    if (grid > slices) grid = slices;
    if (grid > resident) grid = resident;
    return sweep_launch<true, false>(who, p, grid, d_fhat, n_rows, K, N, width, bud, S, d_out_bits, d_out_obj, d_curve, curve_len,
                                     d_status, static_cast<unsigned char *>(d_workspace), st);
}
#pragma GCC visibility pop
