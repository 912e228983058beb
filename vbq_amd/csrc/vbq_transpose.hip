// The layout changes: in [rows][cols] -> out [cols][rows] in 64 x 64 tiles through LDS.   gfx950 / CDNA4 only.
//
//   transpose_tile             the ONE tile walk: whole-tile vector block, ragged vector block, scalar block
//   k_transpose_batched[_vec]  planes of 2- or 4-byte elements (vbq_transpose_planes, vbq_transpose_f32): the u16 form turns
//                              the plane indices [L][C][B] of the fast kernels back into the caller's channel-last [L][B][C]
//   k_prep_planes              channel-last means / spreads [B][C] -> channel-major planes [C][B] in one launch
//                              (quantizer.py:163-164,223), with sigma = sqrt(exp(logvar)) folded in when the caller hands the
//                              log-variances as they come out of the encoder (quantizer.py:197,202: `tf.exp(posterior_logvars)
//                              ** 0.5`): sqrtf is the IEEE root (__fsqrt_rn is NOT on gfx950) and expf is the device library's
//                              exp -- the numbers torch's `exp(x) ** 0.5` gives on this device for every one of the 2^32 float32
//                              inputs (tests/test_gpu_api.py::test_logvar_to_sigma_is_torchs_for_every_float32)
#include "vbq_common.h"

namespace vbq {
namespace {

struct Copy {
    template <typename T>
    __device__ __forceinline__ T operator()(T x) const { return x; }
};

// Tile (r0, c0) of in [rows][cols] to out [cols][rows], f applied to every element on its way into the LDS; 256 threads.
// vec (workgroup-uniform): 16-byte global accesses on both sides -- rows and cols multiples of the vector width V, in and out
// 16-byte aligned; a vector then lies inside the matrix or outside it as a whole.
// Row pitch of the LDS tile in elements: 65 for 4-byte elements, 66 for 2-byte ones (33 words) -- the column reads of the
// second half walk the rows with an odd word stride.
template <typename T, typename F>
__device__ __forceinline__ void transpose_tile(const T *__restrict__ in, long rows, long cols, T *__restrict__ out, long r0, long c0,
                                               bool vec, F f) {
    constexpr int V = 16 / sizeof(T);                        // elements per 16-byte access
    constexpr int VPR = 64 / V;                              // vectors per tile row
    constexpr int PER = 64 * VPR / 256;                      // vectors per thread
    struct alignas(16) Vec { T e[V]; };
    __shared__ T tile[64][sizeof(T) == 4 ? 65 : 66];
    if (vec) {
        if (r0 + 64 <= rows && c0 + 64 <= cols) {
            // whole tile (workgroup-uniform): the loads of a thread go out together, then the LDS writes -- with the bounds test
            // around every access each load was waited for before the next one was issued
            Vec v[PER];
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i = threadIdx.x + 256 * k, lr = i / VPR, lc = (i % VPR) * V;
                v[k] = *reinterpret_cast<const Vec *>(in + (r0 + lr) * cols + c0 + lc);
            }
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i = threadIdx.x + 256 * k, lr = i / VPR, lc = (i % VPR) * V;
#pragma unroll
                for (int e = 0; e < V; ++e) tile[lr][lc + e] = f(v[k].e[e]);
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i = threadIdx.x + 256 * k, lc = i / VPR, lr = (i % VPR) * V;
#pragma unroll
                for (int e = 0; e < V; ++e) v[k].e[e] = tile[lr + e][lc];
            }
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i = threadIdx.x + 256 * k, lc = i / VPR, lr = (i % VPR) * V;
                *reinterpret_cast<Vec *>(out + (c0 + lc) * rows + r0 + lr) = v[k];
            }
            return;
        }
        // a tile on the right or the bottom edge
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = threadIdx.x + 256 * k, lr = i / VPR, lc = (i % VPR) * V;
            const long r = r0 + lr, c = c0 + lc;
            if (r < rows && c < cols) {
                const Vec v = *reinterpret_cast<const Vec *>(in + r * cols + c);
#pragma unroll
                for (int e = 0; e < V; ++e) tile[lr][lc + e] = f(v.e[e]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = threadIdx.x + 256 * k, lc = i / VPR, lr = (i % VPR) * V;
            const long c = c0 + lc, r = r0 + lr;
            if (r < rows && c < cols) {
                Vec v;
#pragma unroll
                for (int e = 0; e < V; ++e) v.e[e] = tile[lr + e][lc];
                *reinterpret_cast<Vec *>(out + c * rows + r) = v;
            }
        }
        return;
    }
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;          // 64 x 4, one element at a time: any shape, any alignment
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const long r = r0 + ty + 4 * k, c = c0 + tx;
        if (r < rows && c < cols) tile[ty + 4 * k][tx] = f(in[r * cols + c]);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const long c = c0 + ty + 4 * k, r = r0 + tx;
        if (r < rows && c < cols) out[c * rows + r] = tile[tx][ty + 4 * k];
    }
}

// ---------------------------------------------------------------------------- planes of 2- or 4-byte elements
// in [batch][rows][cols] -> out [batch][cols][rows]: tiles numbered along blockIdx.x (columns fastest: no 65535-tile limit on
// rows), planes on blockIdx.y.  Moving a 4-byte element is the same for float and uint32_t: vbq_transpose_f32 is one plane.
template <typename T, bool kVec>
__device__ __forceinline__ void transpose_plane_tile(const T *__restrict__ in, long rows, long cols, T *__restrict__ out) {
    in += (long)blockIdx.y * rows * cols;
    out += (long)blockIdx.y * rows * cols;
    const long ctiles = (cols + 63) / 64;
    transpose_tile(in, rows, cols, out, ((long)blockIdx.x / ctiles) * 64, ((long)blockIdx.x % ctiles) * 64, kVec, Copy{});
}

// rows and cols multiples of the vector width, 16-byte aligned planes
template <typename T>
__global__ void __launch_bounds__(256)
k_transpose_batched_vec(const T *__restrict__ in, long rows, long cols, T *__restrict__ out) {
    transpose_plane_tile<T, true>(in, rows, cols, out);
}

template <typename T>
__global__ void __launch_bounds__(256)
k_transpose_batched(const T *__restrict__ in, long rows, long cols, T *__restrict__ out) {
    transpose_plane_tile<T, false>(in, rows, cols, out);
}

template <typename T>
int launch_transpose_batched(const T *in, int64_t batch, int64_t rows, int64_t cols, T *out, hipStream_t st) {
    constexpr int V = 16 / sizeof(T);
    const bool vec = rows % V == 0 && cols % V == 0 && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0 &&
                     (rows * cols * (int64_t)sizeof(T)) % 16 == 0;
    const dim3 grid((unsigned)(((cols + 63) / 64) * ((rows + 63) / 64)), (unsigned)batch);      // tiles on x, planes on y
    if (vec)
        hipLaunchKernelGGL((k_transpose_batched_vec<T>), grid, dim3(256), 0, st, in, (long)rows, (long)cols, out);
    else
        hipLaunchKernelGGL((k_transpose_batched<T>), grid, dim3(256), 0, st, in, (long)rows, (long)cols, out);
    VBQ_CHECK_LAUNCH("transpose_planes");
    return VBQ_OK;
}

}  // namespace
}  // namespace vbq

extern "C" int vbq_transpose_planes(const void *d_in, int64_t n_batch, int64_t n_rows, int64_t n_cols, int32_t elem_bytes,
                                    void *d_out, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n_batch >= 0 && n_rows >= 0 && n_cols >= 0, VBQ_ERR_INVALID_ARGUMENT, "vbq_transpose_planes: bad sizes");
    VBQ_REQUIRE(elem_bytes == 2 || elem_bytes == 4, VBQ_ERR_INVALID_ARGUMENT, "vbq_transpose_planes: elem_bytes %d (2 or 4)", elem_bytes);
    if (n_batch == 0 || n_rows == 0 || n_cols == 0) return VBQ_OK;
    VBQ_REQUIRE(d_in && d_out && d_in != d_out, VBQ_ERR_INVALID_ARGUMENT, "vbq_transpose_planes: null or aliased pointers");
    VBQ_REQUIRE(((n_rows + 63) / 64) * ((n_cols + 63) / 64) <= 0x7fffffffll && n_batch <= 65535, VBQ_ERR_UNSUPPORTED,
                "vbq_transpose_planes: more than 2^31 - 1 tiles of 64 x 64 per plane or more than 65535 planes");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (elem_bytes == 2)
        return launch_transpose_batched<uint16_t>(static_cast<const uint16_t *>(d_in), n_batch, n_rows, n_cols,
                                                  static_cast<uint16_t *>(d_out), st);
    return launch_transpose_batched<uint32_t>(static_cast<const uint32_t *>(d_in), n_batch, n_rows, n_cols,
                                              static_cast<uint32_t *>(d_out), st);
}

extern "C" int vbq_transpose_f32(const float *d_in, int64_t n_rows, int64_t n_cols, float *d_out, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n_rows >= 0 && n_cols >= 0, VBQ_ERR_INVALID_ARGUMENT, "vbq_transpose_f32: bad sizes");
    if (n_rows == 0 || n_cols == 0) return VBQ_OK;
    VBQ_REQUIRE(d_in && d_out && d_in != d_out, VBQ_ERR_INVALID_ARGUMENT, "vbq_transpose_f32: null or aliased pointers");
    const int64_t tiles = ((n_rows + 63) / 64) * ((n_cols + 63) / 64);
    VBQ_REQUIRE(tiles <= 0x7fffffffll, VBQ_ERR_UNSUPPORTED, "vbq_transpose_f32: more than 2^31 - 1 tiles of 64 x 64");
    const bool v4 = n_rows % 4 == 0 && n_cols % 4 == 0 && ((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & 15) == 0;
    const dim3 grid((unsigned)tiles);                       // one plane of 4-byte elements
    const uint32_t *in = reinterpret_cast<const uint32_t *>(d_in);
    uint32_t *out = reinterpret_cast<uint32_t *>(d_out);
    if (v4)
        hipLaunchKernelGGL(k_transpose_batched_vec<uint32_t>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), in,
                           (long)n_rows, (long)n_cols, out);
    else
        hipLaunchKernelGGL(k_transpose_batched<uint32_t>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), in,
                           (long)n_rows, (long)n_cols, out);
    VBQ_CHECK_LAUNCH("transpose");
    return VBQ_OK;
}

// ---------------------------------------------------------------------------- planes from channel-last latents
namespace vbq {
namespace {
struct Spread {
    int kind;                                                // 0: copy, 1: sqrt(x), 2: sqrt(exp(x))
    __device__ __forceinline__ float operator()(float x) const { return kind == 0 ? x : sqrtf(kind == 2 ? expf(x) : x); }
};

// blockIdx.y = 0: means, 1: spreads (sqrt when asked).
__global__ void __launch_bounds__(256)
k_prep_planes(const float *__restrict__ in0, const float *__restrict__ in1, long rows, long cols, float *__restrict__ out0,
              float *__restrict__ out1, int sqrt1, int v4) {
    const bool second = blockIdx.y == 1;
    const long ctiles = (cols + 63) / 64;
    transpose_tile(second ? in1 : in0, rows, cols, second ? out1 : out0, ((long)blockIdx.x / ctiles) * 64,
                   ((long)blockIdx.x % ctiles) * 64, v4 != 0, Spread{second ? sqrt1 : 0});
}
}  // namespace
}  // namespace vbq

extern "C" int vbq_prep_planes_f32(const float *d_means_bc, const float *d_spread_bc, int32_t spread_kind, int64_t n_rows,
                                   int32_t n_ch, float *d_mu_cb, float *d_sigma_cb, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n_rows >= 0 && n_ch >= 1, VBQ_ERR_INVALID_ARGUMENT, "vbq_prep_planes_f32: bad sizes");
    VBQ_REQUIRE(spread_kind >= VBQ_SPREAD_SIGMA && spread_kind <= VBQ_SPREAD_LOGVAR, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_prep_planes_f32: unknown spread_kind %d", spread_kind);
    if (n_rows == 0) return VBQ_OK;
    VBQ_REQUIRE(d_means_bc && d_spread_bc && d_mu_cb && d_sigma_cb && d_means_bc != d_mu_cb && d_spread_bc != d_sigma_cb,
                VBQ_ERR_INVALID_ARGUMENT, "vbq_prep_planes_f32: null or aliased pointers");
    const int64_t tiles = ((n_rows + 63) / 64) * (((int64_t)n_ch + 63) / 64);
    VBQ_REQUIRE(tiles <= 0x7fffffffll, VBQ_ERR_UNSUPPORTED, "vbq_prep_planes_f32: more than 2^31 - 1 tiles of 64 x 64");
    const uintptr_t all = reinterpret_cast<uintptr_t>(d_means_bc) | reinterpret_cast<uintptr_t>(d_spread_bc) |
                          reinterpret_cast<uintptr_t>(d_mu_cb) | reinterpret_cast<uintptr_t>(d_sigma_cb);
    const int v4 = n_rows % 4 == 0 && n_ch % 4 == 0 && (all & 15) == 0;
    hipLaunchKernelGGL(k_prep_planes, dim3((unsigned)tiles, 2), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_means_bc,
                       d_spread_bc, (long)n_rows, (long)n_ch, d_mu_cb, d_sigma_cb, (int)spread_kind, v4);
    VBQ_CHECK_LAUNCH("prep_planes");
    return VBQ_OK;
}
