// K3, the reductions and scans: per-channel moments, the rate-distortion sums of a solve, the input scans
// (largest index, non-finite means / spreads) and float32 sums in NumPy's own order.   gfx950 / CDNA4 only.
//
// Every entry point sits under its kernels.  The moments and the R-D sums accumulate in f64 (reports, never read by a
// kernel); the NumPy-order sums reproduce np.sum's float32 result operation for operation.
#include "vbq_common.h"

namespace vbq {
namespace {

// ---------------------------------------------------------------------------- moments
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// one channel per blockIdx.y, contiguous elements
__global__ void __launch_bounds__(256)
k_moments_flat(const float *__restrict__ x, long n_per_ch, double *__restrict__ out, int vec_ok) {
    const int c = blockIdx.y;
    const float *src = x + (long)c * n_per_ch;
    double s1 = 0.0, s2 = 0.0;
    const long nq = vec_ok ? (n_per_ch >> 2) : 0;
    // four 16-byte loads in flight per lane (one is not enough to cover the HBM latency at 8 waves per SIMD)
    const long stride = (long)gridDim.x * blockDim.x;
    long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (; q + 3 * stride < nq; q += 4 * stride) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4 *>(src + (q + u * stride) * 4);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double a = v[u].x, b = v[u].y, cc = v[u].z, d = v[u].w;
            s1 += (a + b) + (cc + d);
            s2 += (a * a + b * b) + (cc * cc + d * d);
        }
    }
    for (; q < nq; q += stride) {
        const float4 v = *reinterpret_cast<const float4 *>(src + q * 4);
        const double a = v.x, b = v.y, cc = v.z, d = v.w;
        s1 += (a + b) + (cc + d);
        s2 += (a * a + b * b) + (cc * cc + d * d);
    }
    for (long i = nq * 4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_per_ch;
         i += (long)gridDim.x * blockDim.x) {
        const double a = src[i];
        s1 += a;
        s2 += a * a;
    }
    __shared__ double r1[4], r2[4];
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { r1[w] = s1; r2[w] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&out[2 * c], (r1[0] + r1[1]) + (r1[2] + r1[3]));
        atomicAdd(&out[2 * c + 1], (r2[0] + r2[1]) + (r2[2] + r2[3]));
    }
}

// channel-last: thread t of a workgroup always sees channel (t % C) when blockDim % C == 0;
// generic C: each thread walks elements e = t0 + k*stride with stride a multiple of C.
__global__ void __launch_bounds__(256)
k_moments_bc(const float *__restrict__ x, long n_rows, int C, double *__restrict__ out) {
    extern __shared__ double acc[];   // [C][2]
    for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) acc[i] = 0.0;
    __syncthreads();
    const long E = n_rows * (long)C;
    const long nthreads = (long)gridDim.x * blockDim.x;
    const long stride = (nthreads / C) * C;     // <= nthreads (host guarantees nthreads >= C); a multiple of C
    const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t0 < stride) {
        const int c = (int)(t0 % C);
        double s1 = 0.0, s2 = 0.0;
        for (long e = t0; e < E; e += stride) {
            const double a = x[e];
            s1 += a;
            s2 += a * a;
        }
        atomicAdd(&acc[2 * c], s1);
        atomicAdd(&acc[2 * c + 1], s2);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += blockDim.x)
        if (acc[i] != 0.0) atomicAdd(&out[i], acc[i]);
}

}  // namespace
}  // namespace vbq

extern "C" int vbq_moments_f32(const float *d_x, int64_t n_rows, int32_t n_ch, int32_t layout, double *d_out,
                               void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n_rows == 0 || (d_x && d_out), VBQ_ERR_INVALID_ARGUMENT, "vbq_moments_f32: null pointer argument");
    VBQ_REQUIRE(n_rows >= 0 && n_ch >= 1 && n_ch <= 4096, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_moments_f32: bad sizes n_rows=%lld n_ch=%d (n_ch <= 4096)", (long long)n_rows, n_ch);
    VBQ_REQUIRE(layout == VBQ_LAYOUT_BC || layout == VBQ_LAYOUT_CB, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_moments_f32: unknown layout %d", layout);
    if (n_rows == 0) return VBQ_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t E = n_rows * (int64_t)n_ch;
    if (n_ch == 1 || layout == VBQ_LAYOUT_CB) {
        const int64_t n_per_ch = (n_ch == 1) ? E : n_rows;
        const int vec_ok = (reinterpret_cast<uintptr_t>(d_x) % 16 == 0) && (n_per_ch % 4 == 0 || n_ch == 1);
        int64_t gx = (n_per_ch / 4 + 255) / 256;
        const int64_t cap = 2048 / n_ch + 1;
        if (gx > cap) gx = cap;
        if (gx < 1) gx = 1;
        hipLaunchKernelGGL(k_moments_flat, dim3((unsigned)gx, (unsigned)n_ch), dim3(256), 0, st, d_x, (long)n_per_ch,
                           d_out, vec_ok);
    } else {
        int64_t gx = (E + 256 * 16 - 1) / (256 * 16);
        if (gx > 2048) gx = 2048;
        if (gx < (n_ch + 255) / 256) gx = (n_ch + 255) / 256;
        hipLaunchKernelGGL(k_moments_bc, dim3((unsigned)gx), dim3(256), sizeof(double) * 2 * n_ch, st, d_x,
                           (long)n_rows, (int)n_ch, d_out);
    }
    VBQ_CHECK_LAUNCH("moments");
    return VBQ_OK;
}

namespace vbq {
namespace {
// ---------------------------------------------------------------------------- rate-distortion sums
// out[l] = { sum_e ((z - mu)^2 / (2 sigma^2)),  sum_e rate[l][c(e)][idx] }  with z = sorted table[c(e)][idx], everything
// accumulated in f64: the two terms of the Lagrangian the solve minimises, as a report (never used by a kernel).
constexpr int kRdChunk = 8;            // lambdas per workgroup: (mu, sigma) are read once per chunk, not once per lambda
__global__ void __launch_bounds__(256)
k_rd_sums(const float *__restrict__ mu, const float *__restrict__ sg, const uint16_t *__restrict__ idx, long n_rows, int C,
          int layout, long E, int T, const float *__restrict__ tab_sorted, const float *__restrict__ rate, int rate_per_lambda,
          int L, double *__restrict__ out) {
    const int l0 = blockIdx.y * kRdChunk;
    double sd[kRdChunk], sr[kRdChunk];
#pragma unroll
    for (int j = 0; j < kRdChunk; ++j) sd[j] = sr[j] = 0.0;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (long)gridDim.x * blockDim.x) {
        const int c = (C == 1) ? 0 : (layout == VBQ_LAYOUT_BC ? (int)(e % C) : (int)(e / n_rows));
        const double m = (double)mu[e], s = (double)sg[e];
        const double w = 1.0 / (2.0 * s * s);
        const float *ts = tab_sorted + (long)c * T;
#pragma unroll
        for (int j = 0; j < kRdChunk; ++j) {
            const int l = l0 + j;
            if (l < L) {
                const int q = min((int)idx[(long)l * E + e], T - 1);
                const double d = (double)ts[q] - m;
                sd[j] += d * d * w;
                if (rate) sr[j] += (double)rate[(rate_per_lambda ? (long)l * C * T : 0) + (long)c * T + q];
            }
        }
    }
    __shared__ double part[2][kRdChunk][4];
    const int w4 = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < kRdChunk; ++j) {
        double a = sd[j], b = sr[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_down(a, o);
            b += __shfl_down(b, o);
        }
        if ((threadIdx.x & 63) == 0) { part[0][j][w4] = a; part[1][j][w4] = b; }
    }
    __syncthreads();
    if (threadIdx.x < kRdChunk && l0 + (int)threadIdx.x < L) {
        const int j = threadIdx.x;
        atomicAdd(&out[2 * (l0 + j)], part[0][j][0] + part[0][j][1] + part[0][j][2] + part[0][j][3]);
        atomicAdd(&out[2 * (l0 + j) + 1], part[1][j][0] + part[1][j][1] + part[1][j][2] + part[1][j][3]);
    }
}
}  // namespace
}  // namespace vbq

extern "C" int vbq_rd_sums_u16(const float *d_mu, const float *d_sigma, const uint16_t *d_idx, int64_t n_rows, int32_t n_ch,
                               int32_t layout, int32_t n_lambda, int32_t N, const float *d_tab_sorted, const float *d_rate,
                               int32_t rate_per_lambda, double *d_out, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n_rows >= 0 && n_ch >= 1 && n_lambda >= 1 && n_lambda <= 65535 && N >= 0 && N <= 15, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rd_sums_u16: bad sizes");
    VBQ_REQUIRE(layout == VBQ_LAYOUT_BC || layout == VBQ_LAYOUT_CB, VBQ_ERR_INVALID_ARGUMENT, "vbq_rd_sums_u16: unknown layout %d", layout);
    if (n_rows == 0) return VBQ_OK;
    VBQ_REQUIRE(d_mu && d_sigma && d_idx && d_tab_sorted && d_out, VBQ_ERR_INVALID_ARGUMENT, "vbq_rd_sums_u16: null pointer argument");
    const int64_t E = n_rows * (int64_t)n_ch;
    const int chunks = (n_lambda + kRdChunk - 1) / kRdChunk;
    int64_t gx = (E + 255) / 256;
    const int64_t cap = (int64_t)num_cus() * 8 / chunks + 1;
    if (gx > cap) gx = cap;
    hipLaunchKernelGGL(k_rd_sums, dim3((unsigned)gx, (unsigned)chunks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_mu,
                       d_sigma, d_idx, (long)n_rows, (int)n_ch, (int)layout, (long)E, table_size(N), d_tab_sorted, d_rate,
                       (int)rate_per_lambda, (int)n_lambda, d_out);
    VBQ_CHECK_LAUNCH("rd_sums");
    return VBQ_OK;
}

namespace vbq {
namespace {
__global__ void __launch_bounds__(256)
k_index_max(const uint16_t *__restrict__ idx, long n, unsigned int *__restrict__ out) {
    unsigned int m = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) m = max(m, (unsigned int)idx[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned int)__shfl_down(m, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}
}  // namespace
}  // namespace vbq

extern "C" int vbq_index_max_u16(const uint16_t *d_idx, int64_t n, uint32_t *d_max, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n >= 0, VBQ_ERR_INVALID_ARGUMENT, "vbq_index_max_u16: n < 0");
    if (n == 0) return VBQ_OK;
    VBQ_REQUIRE(d_idx && d_max, VBQ_ERR_INVALID_ARGUMENT, "vbq_index_max_u16: null pointer");
    int64_t gx = (n + 255) / 256;
    if (gx > 4096) gx = 4096;
    hipLaunchKernelGGL(k_index_max, dim3((unsigned)gx), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_idx, (long)n, d_max);
    VBQ_CHECK_LAUNCH("index_max");
    return VBQ_OK;
}

namespace vbq {
namespace {
__global__ void __launch_bounds__(256)
k_check_inputs(const float *__restrict__ mu, const float *__restrict__ sg, long n, unsigned int *__restrict__ out) {
    unsigned int bad_mu = 0, bad_sg = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float m = mu[i], s = sg[i];
        bad_mu += !(fabsf(m) <= 3.4028234e38f) ? 1u : 0u;                       // NaN or infinity
        bad_sg += !(s > 0.0f && s <= 3.4028234e38f) ? 1u : 0u;                  // NaN, infinity, zero or negative
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { bad_mu += __shfl_down(bad_mu, o, 64); bad_sg += __shfl_down(bad_sg, o, 64); }
    if ((threadIdx.x & 63) == 0 && (bad_mu | bad_sg)) { atomicAdd(&out[0], bad_mu); atomicAdd(&out[1], bad_sg); }
}
}  // namespace
}  // namespace vbq

extern "C" int vbq_check_inputs_f32(const float *d_mu, const float *d_sigma, int64_t n, uint32_t *d_bad, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n >= 0, VBQ_ERR_INVALID_ARGUMENT, "vbq_check_inputs_f32: n < 0");
    if (n == 0) return VBQ_OK;
    VBQ_REQUIRE(d_mu && d_sigma && d_bad, VBQ_ERR_INVALID_ARGUMENT, "vbq_check_inputs_f32: null pointer");
    int64_t gx = (n + 255) / 256;
    if (gx > 4096) gx = 4096;
    hipLaunchKernelGGL(k_check_inputs, dim3((unsigned)gx), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_mu, d_sigma, (long)n, d_bad);
    VBQ_CHECK_LAUNCH("check_inputs");
    return VBQ_OK;
}

// ---------------------------------------------------------------------------- the notebook's moment, in NumPy's order
// empirical_std = np.sqrt(np.mean(vecs_u.ravel()**2)) (ipynb:374) is a float32 reduction, and float32 sums depend on
// their order.  NumPy's order: the reduce loop hands its pairwise routine blocks of 8192 elements (the iterator's
// buffer) and accumulates the block results one after the other; inside a block, halves are split on multiples of 8
// down to runs of <= 128 elements, which are summed with 8 interleaved accumulators combined as
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) (loops_utils.h.src, *_pairwise_sum).  Reproduced here operation for operation:
// a full block is 64 runs of 128 -> one workgroup; the ragged last block and the chain over the block sums run on one
// thread out of LDS.  oracle/vbq_oracle.c restates the same order in C and is pinned against np.sum.
namespace vbq {
namespace {
constexpr int kNpBlock = 8192;
constexpr int kNpRunStride = 136;      // 128 + 8 words: the 64 runs of a block start on different LDS banks

// SQ: sum of squares (the notebook's moment), else the plain sum (np.sum of the per-image code lengths, utils.py:547-552).
// blockIdx.y: the row of a [rows][n] batch (row sums are independent reductions of n contiguous elements each).
template <bool SQ>
__global__ void __launch_bounds__(256)
k_np_block_sums(const float *__restrict__ x, long n, long nfull, float *__restrict__ block_sums, int vec) {
    __shared__ float sq[64 * kNpRunStride];
    __shared__ float racc[512];
    __shared__ float leaf[64];
    const float *src = x + (long)blockIdx.y * n + (long)blockIdx.x * kNpBlock;
    block_sums += (long)blockIdx.y * nfull;
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int e = (k * 256 + t) * 4;                      // element within the block; 4 | 128: one run per float4
        float4 v;
        if (vec) v = *reinterpret_cast<const float4 *>(src + e);
        else v = make_float4(src[e], src[e + 1], src[e + 2], src[e + 3]);      // rows that do not start on 16 bytes
        float *d = sq + (e >> 7) * kNpRunStride + (e & 127);
        if (SQ) { d[0] = __fmul_rn(v.x, v.x); d[1] = __fmul_rn(v.y, v.y); d[2] = __fmul_rn(v.z, v.z); d[3] = __fmul_rn(v.w, v.w); }
        else { d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = t + 256 * h, run = p >> 3, j = p & 7;
        const float *a = sq + run * kNpRunStride + j;
        float r = a[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) r = __fadd_rn(r, a[8 * i]);
        racc[p] = r;
    }
    __syncthreads();
    if (t < 64) {
        const float *r = racc + 8 * t;
        leaf[t] = __fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3])),
                            __fadd_rn(__fadd_rn(r[4], r[5]), __fadd_rn(r[6], r[7])));
    }
    __syncthreads();
    for (int s2 = 1; s2 < 64; s2 <<= 1) {
        if (t < 64 && (t & (2 * s2 - 1)) == 0) leaf[t] = __fadd_rn(leaf[t], leaf[t + s2]);
        __syncthreads();
    }
    if (t == 0) block_sums[blockIdx.x] = leaf[0];
}

// pairwise sum of n <= 8192 ready-made squares (one thread; recursion depth <= 7)
__device__ __noinline__ float np_pairwise(const float *a, int n) {
    if (n < 8) {
        float res = 0.0f;
        for (int i = 0; i < n; ++i) res = __fadd_rn(res, a[i]);
        return res;
    }
    if (n <= 128) {
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int i;
        for (i = 8; i < n - (n % 8); i += 8)
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = __fadd_rn(r[j], a[i + j]);
        float res = __fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3])),
                              __fadd_rn(__fadd_rn(r[4], r[5]), __fadd_rn(r[6], r[7])));
        for (; i < n; ++i) res = __fadd_rn(res, a[i]);
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    const float lo = np_pairwise(a, n2);
    return __fadd_rn(lo, np_pairwise(a + n2, n - n2));
}

template <bool SQ>
__global__ void __launch_bounds__(256)
k_np_finish(const float *__restrict__ x, long n, const float *__restrict__ block_sums, float *__restrict__ out) {
    __shared__ float buf[kNpBlock];
    const long nfull = n / kNpBlock;
    x += (long)blockIdx.x * n;
    block_sums += (long)blockIdx.x * nfull;
    float acc = 0.0f;
    for (long b0 = 0; b0 < nfull; b0 += kNpBlock) {           // the chain over the block sums, 8192 at a time out of LDS
        const int m = (int)(nfull - b0 < kNpBlock ? nfull - b0 : kNpBlock);
        for (int i = threadIdx.x; i < m; i += blockDim.x) buf[i] = block_sums[b0 + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < m; ++i) acc = __fadd_rn(acc, buf[i]);
        __syncthreads();
    }
    const int tail = (int)(n - nfull * kNpBlock);
    if (tail > 0) {
        for (int i = threadIdx.x; i < tail; i += blockDim.x) {
            const float v = x[nfull * kNpBlock + i];
            buf[i] = SQ ? __fmul_rn(v, v) : v;
        }
        __syncthreads();
        if (threadIdx.x == 0) acc = __fadd_rn(acc, np_pairwise(buf, tail));
    }
    if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

template <bool SQ>
int launch_np_sums(const float *d_x, int64_t n, int64_t rows, float *d_out, float *bs, hipStream_t st) {
    const int64_t nfull = n / kNpBlock;
    // a row of the batch starts on 16 bytes when the base does and 4 | n; otherwise 4-byte loads
    const int vec = (reinterpret_cast<uintptr_t>(d_x) & 15) == 0 && (rows == 1 || n % 4 == 0);
    if (nfull > 0) {
        hipLaunchKernelGGL((k_np_block_sums<SQ>), dim3((unsigned)nfull, (unsigned)rows), dim3(256), 0, st, d_x, (long)n, (long)nfull, bs, vec);
        VBQ_CHECK_LAUNCH("np_block_sums");
    }
    hipLaunchKernelGGL((k_np_finish<SQ>), dim3((unsigned)rows), dim3(256), 0, st, d_x, (long)n, bs, d_out);
    VBQ_CHECK_LAUNCH("np_finish");
    return VBQ_OK;
}
}  // namespace
}  // namespace vbq

extern "C" size_t vbq_numpy_sum_sq_workspace_bytes(int64_t n) {
    return n <= 0 ? 0 : (size_t)(n / vbq::kNpBlock + 1) * sizeof(float);
}

extern "C" int vbq_numpy_sum_sq_f32(const float *d_x, int64_t n, float *d_out, void *d_workspace, size_t workspace_bytes,
                                    void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n >= 0 && d_out, VBQ_ERR_INVALID_ARGUMENT, "vbq_numpy_sum_sq_f32: bad arguments");
    VBQ_REQUIRE(n == 0 || d_x, VBQ_ERR_INVALID_ARGUMENT, "vbq_numpy_sum_sq_f32: null pointer");
    VBQ_REQUIRE(n == 0 || (reinterpret_cast<uintptr_t>(d_x) & 15) == 0, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_numpy_sum_sq_f32: d_x must be 16-byte aligned");
    const size_t need = vbq_numpy_sum_sq_workspace_bytes(n);
    VBQ_REQUIRE(n == 0 || (d_workspace && workspace_bytes >= need), VBQ_ERR_WORKSPACE,
                "vbq_numpy_sum_sq_f32: workspace of %zu bytes given, %zu needed", workspace_bytes, need);
    VBQ_REQUIRE(n / kNpBlock <= 0x7fffffffLL, VBQ_ERR_UNSUPPORTED, "vbq_numpy_sum_sq_f32: more than 2^44 elements");
    return launch_np_sums<true>(d_x, n, 1, d_out, reinterpret_cast<float *>(d_workspace), reinterpret_cast<hipStream_t>(stream));
}

extern "C" size_t vbq_numpy_row_sums_workspace_bytes(int64_t n_rows, int64_t n) {
    return n_rows <= 0 || n <= 0 ? 0 : (size_t)n_rows * (size_t)(n / vbq::kNpBlock + 1) * sizeof(float);
}

extern "C" int vbq_numpy_row_sums_f32(const float *d_x, int64_t n_rows, int64_t n, float *d_out, void *d_workspace,
                                      size_t workspace_bytes, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n_rows >= 0 && n >= 0 && n_rows <= 65535, VBQ_ERR_INVALID_ARGUMENT, "vbq_numpy_row_sums_f32: bad sizes (at most 65535 rows)");
    if (n_rows == 0) return VBQ_OK;
    VBQ_REQUIRE(d_out && (n == 0 || d_x), VBQ_ERR_INVALID_ARGUMENT, "vbq_numpy_row_sums_f32: null pointer");
    VBQ_REQUIRE((reinterpret_cast<uintptr_t>(d_x) & 3) == 0, VBQ_ERR_INVALID_ARGUMENT, "vbq_numpy_row_sums_f32: d_x must be 4-byte aligned");
    const size_t need = vbq_numpy_row_sums_workspace_bytes(n_rows, n);
    VBQ_REQUIRE(n == 0 || (d_workspace && workspace_bytes >= need), VBQ_ERR_WORKSPACE,
                "vbq_numpy_row_sums_f32: workspace of %zu bytes given, %zu needed", workspace_bytes, need);
    VBQ_REQUIRE(n / kNpBlock <= 0x7fffffffLL, VBQ_ERR_UNSUPPORTED, "vbq_numpy_row_sums_f32: more than 2^44 elements per row");
    return launch_np_sums<false>(d_x, n, n_rows, d_out, reinterpret_cast<float *>(d_workspace), reinterpret_cast<hipStream_t>(stream));
}
