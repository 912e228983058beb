// Test-only: put a known byte into every LDS byte of every CU, and read back what a workgroup finds there.
// Compiled by tests/lds_state.py into a temporary directory; not part of any product library (tests/lds_state.py says what
// the three kernels are for).
//
// Geometry of lds_fill and lds_probe: 256 threads, ALL 160 KiB of a CU as dynamic LDS, so one workgroup fits a CU and the
// first <CU count> workgroups of a grid land on that many different CUs.  Each workgroup then keeps its CU for `hold_ticks`
// ticks of the 100 MHz constant clock -- a loop with a hard iteration cap that reads the clock and nothing else: no
// workgroup waits for another, for memory or for a flag, so the kernel ends whatever the rest of the machine does.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kLdsBytes = 160 * 1024;
constexpr int kLdsWords = kLdsBytes / 4;
constexpr int kThreads = 256;
constexpr int kHoldCap = 1 << 14;           // iterations of the hold loop at the very most (each sleeps ~0.25 us: < 5 ms)
constexpr int kToyWords = 256;              // lds_toy: 1 KiB

// 12 bits: XCC_ID[3:0] (hardware register 20) above HW_ID[15:8] = SE_ID | SH_ID | CU_ID (hardware register 4).
__device__ __forceinline__ unsigned int cu_identity() {
    const unsigned int xcc = __builtin_amdgcn_s_getreg(((4 - 1) << 11) | (0 << 6) | 20);
    const unsigned int hw = __builtin_amdgcn_s_getreg(((8 - 1) << 11) | (8 << 6) | 4);
    return (xcc << 8) | hw;
}

__device__ __forceinline__ void hold(long long ticks) {
    const long long t0 = wall_clock64();
    for (int it = 0; it < kHoldCap; ++it) {
        if (wall_clock64() - t0 >= ticks) break;
        __builtin_amdgcn_s_sleep(8);
    }
}

// seen: u32 [128], one bit per CU identity, OR-ed.
__global__ __launch_bounds__(kThreads) void k_lds_fill(unsigned int word, unsigned int *seen, long long hold_ticks) {
    extern __shared__ unsigned int v[];        // (the LDS outlives the kernel as far as the compiler knows: every store is made)
    for (int i = threadIdx.x; i < kLdsWords; i += kThreads) v[i] = word;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int id = cu_identity();
        atomicOr(&seen[id >> 5], 1u << (id & 31));
    }
    hold(hold_ticks);
}

// out: u32 [gridDim.x][2] = (CU identity, LDS bytes equal to `byte`), zero before the launch.  Nothing is written to the LDS.
__global__ __launch_bounds__(kThreads) void k_lds_probe(unsigned int byte, unsigned int *out, long long hold_ticks) {
    extern __shared__ unsigned int v[];        // (contents unknown to the compiler: every load is made)
    unsigned int n = 0;
    for (int i = threadIdx.x; i < kLdsWords; i += kThreads) {
        const unsigned int w = v[i];
        for (int b = 0; b < 4; ++b) n += ((w >> (8 * b)) & 0xFFu) == byte;
    }
    atomicAdd(&out[2 * blockIdx.x + 1], n);
    if (threadIdx.x == 0) out[2 * blockIdx.x] = cu_identity();
    hold(hold_ticks);
}

// DELIBERATELY WRONG (the sensitivity control): out[block] = sum of 1 KiB of LDS the kernel never wrote.
__global__ __launch_bounds__(kToyWords) void k_lds_toy(unsigned int *out) {
    extern __shared__ unsigned int v[];        // (contents unknown to the compiler: every load is made)
    atomicAdd(&out[blockIdx.x], v[threadIdx.x]);
}

template <typename K>
int whole_cu(K kernel) {
    return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
}

}  // namespace

// Each returns the hipError_t of its launch (0: enqueued).  `grid` workgroups; d_seen: 128 u32; d_out: see the kernels.
extern "C" int lds_fill(int byte, int grid, long long hold_ticks, void *d_seen, void *stream) {
    if (byte < 0 || byte > 255 || grid < 1 || hold_ticks < 0 || !d_seen) return (int)hipErrorInvalidValue;
    if (int e = whole_cu(k_lds_fill)) return e;
    hipLaunchKernelGGL(k_lds_fill, dim3(grid), dim3(kThreads), kLdsBytes, (hipStream_t)stream, 0x01010101u * (unsigned int)byte,
                       (unsigned int *)d_seen, hold_ticks);
    return (int)hipGetLastError();
}

extern "C" int lds_probe(int byte, int grid, long long hold_ticks, void *d_out, void *stream) {
    if (byte < 0 || byte > 255 || grid < 1 || hold_ticks < 0 || !d_out) return (int)hipErrorInvalidValue;
    if (int e = whole_cu(k_lds_probe)) return e;
    hipLaunchKernelGGL(k_lds_probe, dim3(grid), dim3(kThreads), kLdsBytes, (hipStream_t)stream, (unsigned int)byte, (unsigned int *)d_out,
                       hold_ticks);
    return (int)hipGetLastError();
}

extern "C" int lds_toy(int grid, void *d_out, void *stream) {
    if (grid < 1 || !d_out) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_lds_toy, dim3(grid), dim3(kToyWords), kToyWords * 4, (hipStream_t)stream, (unsigned int *)d_out);
    return (int)hipGetLastError();
}
