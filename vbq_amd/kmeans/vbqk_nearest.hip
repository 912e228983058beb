// Nearest code point of every channel of channel-last samples in one launch (include/vbq_kmeans.h): per channel the arithmetic
// of k_nearest_code (vbq_amd/csrc/vbq_baselines.hip, scipy.cluster.vq.vq for 1-D data) -- f64 squared distance, one rounded
// subtraction and one rounded product, first minimum in code-book order -- with the optional fused bincount.
// A workgroup of 256 lanes takes a tile of TC channels (a power of two, at most 64, as many as keep the tile's code rows within
// 56 KiB of LDS) and walks over rows; lane = (row, channel of the tile) with the channel fastest, so a wave reads 64 / TC rows
// of TC consecutive floats.  A code row is padded to an odd number of doubles: lanes of different channels that read code j of
// their rows at the same time then fall on different LDS banks.
// gfx950 / ROCm only.
#include "vbq_common.h"
#include "vbq_kmeans.h"

namespace vbq {
namespace {

constexpr int kNcThreads = 256;
constexpr int kNcMaxCodes = 1024;
constexpr size_t kNcLdsBytes = 56 * 1024;

__global__ void __launch_bounds__(kNcThreads)
k_nearest_code_channels(const float *__restrict__ x, long B, int C, const double *__restrict__ codes, int K, int kpad, int TC,
                        int *__restrict__ out_i, double *__restrict__ out_q, unsigned long long *__restrict__ counts) {
    extern __shared__ double cb[];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * TC;
    for (int e = tid; e < TC * K; e += kNcThreads) {
        const int cl = e / K, j = e - cl * K;
        if (c0 + cl < C) cb[cl * kpad + j] = codes[(size_t)(c0 + cl) * K + j];
    }
    __syncthreads();
    const int cl = tid & (TC - 1), c = c0 + cl, rows = kNcThreads / TC;
    if (c >= C) return;
    const double *row = cb + cl * kpad;
    for (long b = (long)blockIdx.y * rows + tid / TC; b < B; b += (long)gridDim.y * rows) {
        const size_t e = (size_t)b * C + c;
        const double v = (double)x[e];
        int best = 0;
        double bd = 0.0;
        for (int j = 0; j < K; ++j) {
            const double d = __dsub_rn(v, row[j]);
            const double d2 = __dmul_rn(d, d);
            if (j == 0 || d2 < bd) { bd = d2; best = j; }
        }
        if (out_i) out_i[e] = best;
        if (out_q) out_q[e] = row[best];
        if (counts) atomicAdd(&counts[(size_t)c * K + best], 1ULL);
    }
}

}  // namespace
}  // namespace vbq

#pragma GCC visibility push(default)
extern "C" int vbqk_nearest_code_channels_f64(const float *d_x, int64_t B, int32_t C, const double *d_codes, int32_t k,
                                              int32_t *d_out_index, double *d_out_value, int64_t *d_counts, void *stream) {
    using namespace vbq;
    const char *who = "vbqk_nearest_code_channels_f64";
    VBQ_REQUIRE(B >= 0 && C >= 1 && k >= 1 && k <= kNcMaxCodes, VBQ_ERR_INVALID_ARGUMENT,
                "%s: bad arguments B=%lld C=%d k=%d (need B >= 0, C >= 1, 1 <= k <= 1024)", who, (long long)B, C, k);
    if (B == 0) return VBQ_OK;
    VBQ_REQUIRE(d_x && d_codes, VBQ_ERR_INVALID_ARGUMENT, "%s: null input", who);
    const int kpad = k | 1;
    int TC = 64;
    while (TC > 1 && ((size_t)TC * kpad * sizeof(double) > kNcLdsBytes || TC / 2 >= C)) TC >>= 1;
    const int rows = kNcThreads / TC;
    int64_t gy = (B + rows - 1) / rows;
    if (gy > 1024) gy = 1024;
    hipLaunchKernelGGL(k_nearest_code_channels, dim3((unsigned)((C + TC - 1) / TC), (unsigned)gy), dim3(kNcThreads),
                       sizeof(double) * TC * kpad, reinterpret_cast<hipStream_t>(stream), d_x, (long)B, (int)C, d_codes, (int)k,
                       kpad, TC, d_out_index, d_out_value, reinterpret_cast<unsigned long long *>(d_counts));
    VBQ_CHECK_LAUNCH(who);
    return VBQ_OK;
}
#pragma GCC visibility pop
