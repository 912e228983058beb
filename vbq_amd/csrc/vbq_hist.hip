// K2, the rank histogram, and what its flush uses.   gfx950 / CDNA4 only.
//
// K2 replaces the per-channel np.bincount of quantizer.py:104-105,138-140 and the Counter
// of ipynb:453.  One workgroup privatises the bins of one (lambda, channel[-group]) in LDS
// (u32), streams its share of the u16 indices with 16-B loads, and flushes the non-zero
// bins with one 64-bit global atomic each.  Integer adds: the result does not depend on
// the order of arrival, the grid shape or the number of GPUs.
// Behind it: the code-length lookups of the counts (k_lut_*) and the 3 x 21-bit counter packing of the all-reduce.
// The reductions (moments, R-D sums, scans, NumPy-order sums) are in vbq_reduce.hip, the tile transposes in
// vbq_transpose.hip, the table lookups (vbq_gather_f32 among them) in vbq_latents.hip.
#include <stdlib.h>

#include "vbq_common.h"

namespace vbq {
namespace {

#ifndef VBQ_HIST_THREADS
#define VBQ_HIST_THREADS 512
#endif
constexpr int kHistThreads = VBQ_HIST_THREADS;
#ifndef VBQ_HIST_U
#define VBQ_HIST_U 3
#endif
// Cut-off level of the lane-private hot counters (hist_add8_hot): 0 = none (hist_add8 at every depth), else 64 << (Lh + 1) more
// LDS words.  3 and 4 measured alike (both at the kernel's load-only time), 3 takes 4 KB instead of 8.
#ifndef VBQ_HIST_HOT
#define VBQ_HIST_HOT 3
#endif

// LDS slot of rank index q.  In rank order every code point of bit levels 0..5 sits at
// q = 31 (mod 32) -- one LDS bank -- and those are exactly the bins that fill up at large
// lambda.  q ^ (q >> 6) is a bijection of [0, 2^11) that spreads every level evenly over the
// 32 banks (measured: the histogram pass went from 0.65 ms to the load-bound time).
// Indices that did not come from K1 may be anything up to 65535: the slot is masked into the 8192-word bin
// array (memory-safe, counts of such indices are meaningless -- vbq_index_max_u16 tells the caller beforehand).
template <int N>
__device__ __forceinline__ unsigned int bin_slot(unsigned int q) { return (q ^ (q >> 6)) & ((2u << N) - 1u); }

// Eight indices of one thread (one 16-B load) into the LDS histogram: the form of N = 11 and 12, whose bins leave no room
// for hot words (N <= 10: hist_add8_hot below).
// An LDS atomic wave-instruction costs ~3 cycles per lane that shares a bank with another
// lane (same address included, unless ALL lanes agree), and at large lambda 50-90 % of the
// indices are one and the same bin.  So: (1) the thread counts how many of its eight indices
// equal its first one and issues the other seven adds only where they differ (few active
// lanes); (2) the lanes whose first index equals the wave leader's are summed with four
// ballots and added by one lane.  Spread-out distributions pay ~10 extra VALU ops per index.
// private copies of the bins per workgroup (lane & (K-1) picks one): 4 for up to 2048 bins (8 copies measured
// slower), 2 / 1 for the 4095 / 8191 bins of N = 11 / 12 -- always 32 KB of LDS
__host__ __device__ constexpr int hist_slots(int T) { return T + 1 <= 2048 ? 2048 : (T + 1 <= 4096 ? 4096 : 8192); }
__host__ __device__ constexpr int hist_copies(int T) { return 8192 / hist_slots(T); }
// The copies of a bin are adjacent words (word = 4 * slot + copy): lanes of different copies never meet on a
// bank, and zeroing / flushing the 32 KB moves 16 bytes per LDS instruction.

template <int N, int kHistCopies>
__device__ __forceinline__ void hist_add8(unsigned int *h, const uint4 v) {
    unsigned int s[8];
    {
        const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s[2 * k] = bin_slot<N>(w[k] & 0xffffu);
            s[2 * k + 1] = bin_slot<N>(w[k] >> 16);
        }
    }
    unsigned int cnt = 1;
    bool eq[8];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        eq[k] = s[k] == s[0];
        cnt += eq[k] ? 1u : 0u;
    }
    const unsigned int lead = __builtin_amdgcn_readfirstlane(s[0]);
    const bool same = s[0] == lead;
    unsigned int tot = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        tot += (unsigned int)__popcll(__ballot(same && ((cnt >> b) & 1u))) << b;
    const unsigned long long same_mask = __ballot(same);
    const int first = __ffsll((long long)same_mask) - 1;
    const int lane = threadIdx.x & 63;
    unsigned int *hc = h + (lane & (kHistCopies - 1));                      // this lane's copy of the bins
    if (lane == first) atomicAdd(&hc[kHistCopies * lead], tot);
    if (!same) atomicAdd(&hc[kHistCopies * s[0]], cnt);
#pragma unroll
    for (int k = 1; k < 8; ++k)
        if (!eq[k]) atomicAdd(&hc[kHistCopies * s[k]], 1u);
}

// ---- lane-private counters for the shallow levels (N <= 10, where the bins have four copies)
// In rank order the code points of bit levels 0 .. Lh are the ranks q with m = q + 1 a multiple of 2^(N - Lh): k = m >> (N - Lh)
// in [1, 2^(Lh+1) - 1].  Those few ranks hold most of a row from lambda ~ 0.02 up (on the Kodak-24 sweep, Lh = 3: 21 % at
// 2^-8, 43 % at 0.022, 92 % at 1) and no single one of them dominates, so hist_add8's merging of ONE bin per wave-instruction
// leaves every ds_add with most of its 64 lanes on a handful of words.  Here a hot rank's counter is the word
// hot[k * 64 + lane]: its bank is the lane number, and however many lanes of a wave-instruction hold hot ranks they never
// meet on a bank.  The waves of the workgroup share the words through the same ds_add_u32; hist_fold_hot adds them into the
// bins before the flush.  Any index that is not hot -- foreign values up to 65535 included: m = 65536 has its low bits clear,
// hence the range test on k, folded into hot_bits -- takes hist_add8's word, so the counts of every u16 input are what they
// were.  Eight unpredicated ds_add_u32 per octet, ~11 VALU operations per index, no ballots and no branches: K2 on the
// Kodak-24 planes 147 -> 117 us, 3 us above the same kernel with the counting taken out (EXPERIMENTS.md).
__host__ __device__ constexpr int hist_hot_level(int N, int T) {
    return hist_copies(T) == 4 && VBQ_HIST_HOT > 0 ? (VBQ_HIST_HOT < N ? VBQ_HIST_HOT : N) : 0;
}
__host__ __device__ constexpr int hist_hot_words(int Lh) { return Lh == 0 ? 0 : 128 << Lh; }

template <int N, int Lh>
__device__ __forceinline__ void hist_add8_hot(unsigned int *h, const uint4 v) {
    constexpr int sh = N - Lh;
    constexpr unsigned int hot_bits = ((2u << Lh) - 1u) << sh;          // the bits of m that a hot rank may have set
    const unsigned int lane = threadIdx.x & 63;
    const unsigned int hot0 = 4u * (8192u + lane), bin0 = 4u * (lane & 3u);     // byte offsets into h
    const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const unsigned int q = (j & 1) ? w[j >> 1] >> 16 : w[j >> 1] & 0xffffu;
        const unsigned int m = q + 1u;                                  // 1 .. 65536
        const bool is_hot = (m & ~hot_bits) == 0u;
        // both offsets computed outside the ?: -- one v_cndmask; written inside it, each side lands behind an exec-masked branch
        const unsigned int cold = (bin_slot<N>(q) << 4) | bin0;
        const unsigned int hot = ((m >> sh) << 8) | hot0;
        atomicAdd(reinterpret_cast<unsigned int *>(reinterpret_cast<char *>(h) + (is_hot ? hot : cold)), 1u);
    }
    // one octet at a time: scheduled across the octets of a stage, the offsets of all its indices are live at once and the
    // kernel no longer fits the 64 registers of eight waves per SIMD
    __builtin_amdgcn_sched_barrier(0);
}

// Behind the counting barrier: the 64 lane words of every hot rank summed and ADDED to copy 0 of the rank's bin (the scalar
// paths of k_hist_flat count hot ranks in the bins).  One 16-byte LDS read per thread, 16 threads per rank.
template <int N, int Lh, int kThreads>
__device__ __forceinline__ void hist_fold_hot(unsigned int *h) {
    constexpr int n4 = hist_hot_words(Lh) / 4;
    static_assert(n4 % 64 == 0, "whole waves take part in the shuffles");
    for (int i = (int)threadIdx.x; i < n4; i += kThreads) {
        const uint4 w = reinterpret_cast<const uint4 *>(h + 8192)[i];
        unsigned int sum = (w.x + w.y) + (w.z + w.w);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        const unsigned int k = (unsigned int)i >> 4;                    // k = 0 is no rank: its words stay zero
        if ((i & 15) == 0 && k && sum) h[4u * bin_slot<N>((k << (N - Lh)) - 1u)] += sum;
    }
}

// One 16-byte load of eight indices, non-temporal: every index is read exactly once.  Without the hint the loads alone take
// 128 instead of 110-114 us on the Kodak-24 planes, and in the build step, right behind K1's index writes, the whole kernel
// 165 instead of 144 us (EXPERIMENTS.md, "K2 through an LDS ring").
__device__ __forceinline__ uint4 load_octet(const uint16_t *p) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    return make_uint4(t.x, t.y, t.z, t.w);
}

// The flush of a histogram workgroup: its bins out of LDS into row (l, c) of counts, added (assign == 0) or stored with the
// code-length model lut[count] next to them (see k_hist_flat).
template <int N, typename CountT, int kThreads>
__device__ __forceinline__ void hist_flush(const unsigned int *h, int l, int c, int C, CountT *__restrict__ counts, int assign,
                                           const float *__restrict__ assign_lut, long lut_n, float *__restrict__ models) {
    constexpr int T = table_size(N);
    constexpr int kHistCopies = hist_copies(T);
    CountT *dst = counts + ((long)l * C + c) * T;
    // Flush, the bins of a thread first read and summed, then written (and looked up) together: the LDS reads, the table
    // gathers and the stores of its FI bins overlap instead of following each other through per-bin branches.
    constexpr int FI = (T + kThreads - 1) / kThreads;
    unsigned int v[FI];
#pragma unroll
    for (int r = 0; r < FI; ++r) {
        const int i = (int)threadIdx.x + r * kThreads;
        const int ii = i < T ? i : T - 1;
        if constexpr (kHistCopies == 4) {
            const uint4 q4 = reinterpret_cast<const uint4 *>(h)[bin_slot<N>(ii)];
            v[r] = (q4.x + q4.y) + (q4.z + q4.w);
        } else if constexpr (kHistCopies == 2) {
            const uint2 q2 = reinterpret_cast<const uint2 *>(h)[bin_slot<N>(ii)];
            v[r] = q2.x + q2.y;
        } else {
            v[r] = h[bin_slot<N>(ii)];
        }
    }
    if (assign) {
#pragma unroll
        for (int r = 0; r < FI; ++r) {
            const int i = (int)threadIdx.x + r * kThreads;
            if (i < T) dst[i] = (CountT)v[r];
        }
        if (models) {
            float m[FI];
#pragma unroll
            for (int r = 0; r < FI; ++r) m[r] = assign_lut[(long)v[r] < lut_n ? (long)v[r] : lut_n - 1];
            float *mdst = models + ((long)l * C + c) * T;
#pragma unroll
            for (int r = 0; r < FI; ++r) {
                const int i = (int)threadIdx.x + r * kThreads;
                if (i < T) mdst[i] = m[r];
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < FI; ++r) {
            const int i = (int)threadIdx.x + r * kThreads;
            if (i < T && v[r]) atomicAdd(&dst[i], (CountT)v[r]);
        }
    }
}

// All indices of the workgroup belong to one channel: [l][c][n_per_ch] contiguous.
// assign_lut != nullptr (only with ONE workgroup per (lambda, channel), gridDim.x == 1): the workgroup owns its whole row of
// bins, so it STORES them (zeros included: no memset of the 67 MB array beforehand, no atomics) and writes the code-length
// model lut[count] next to them (quantizer.py:141-146 fused into the flush; models may be nullptr).
// Lh: cut-off level of the lane-private hot counters behind the bins (0: none, the bins alone with hist_add8).
// The LDS (32 KB + 4 KB of hot words) admits four workgroups per CU, that is kHistThreads / 64 waves per SIMD: the registers
// must allow as many.
template <int N, typename CountT, int Lh = hist_hot_level(N, table_size(N))>
__global__ void __launch_bounds__(kHistThreads) __attribute__((amdgpu_waves_per_eu(kHistThreads / 64)))
k_hist_flat(const uint16_t *__restrict__ idx, long n_per_ch, long ch_stride, int C, long E,
            CountT *__restrict__ counts, int vec_ok, int assign = 0, const float *__restrict__ assign_lut = nullptr,
            long lut_n = 0, float *__restrict__ models = nullptr) {
    constexpr int T = table_size(N);
    constexpr int kHistCopies = hist_copies(T);
    static_assert(T + 1 <= 8192, "bins are laid out for at most 8192 slots");
    constexpr int kWords = 8192 + hist_hot_words(Lh);               // 32 KB of bins, then the hot words
    __shared__ __align__(16) unsigned int h[kWords];
    auto add8 = [&](const uint4 v) {
        if constexpr (Lh > 0) hist_add8_hot<N, Lh>(h, v);
        else hist_add8<N, kHistCopies>(h, v);
    };
    // assign == 2: the grid is (1, L, C) and walks the channels from the LAST one down, all lambdas of a channel together --
    // the order in which the solve kernel's output is most recent (and still in the memory-side cache) comes first
    const int c = assign == 2 ? C - 1 - (int)blockIdx.z : (int)blockIdx.y;
    const int l = assign == 2 ? (int)blockIdx.y : (int)blockIdx.z;
    // The 16-byte loads start at the first 16-byte boundary of this (lambda, channel) row: up to seven leading indices (odd
    // row counts shift every other row by two bytes) are counted one by one by the row's first workgroup, like the tail.
    const uint16_t *src0 = idx + (long)l * E + (long)c * ch_stride;
    const long head_max = (long)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(src0) & 15u)) & 15u) >> 1);
    const long head = vec_ok ? (head_max < n_per_ch ? head_max : n_per_ch) : 0;
    const uint16_t *src = src0 + head;
    const long n_body = n_per_ch - head;
    const long noct = vec_ok ? (n_body >> 3) : 0;
    const long stride = (long)gridDim.x * blockDim.x;
    long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    // iterations in which every lane of the wave has two full loads take the aggregated path
    const int lane = threadIdx.x & 63;
    // Software-pipelined in two register stages of U 16-byte loads per lane: one stage is in flight while the
    // other is counted (Little's law: 20 waves per CU x 64 lanes x U x 16 B must cover the HBM latency); the
    // first stage is issued before the bins are cleared.  "full": every lane of the wave has all U loads.
    constexpr int U = VBQ_HIST_U;
    auto full = [&](long qq, int n) { return (qq - lane) + 63 + (long)(n - 1) * stride < noct; };
    // STAGES of U loads that every lane of this wave has (wave-uniform): stage s reads octets q0 + (s U + u) stride.  The loop
    // over them is written on that count, with NO condition around a load: with `if (haveB) load B` the compiler cannot tell
    // whether B is in flight, waits with vmcnt(1) / vmcnt(0) for A -- i.e. for B as well -- and the two register stages take
    // turns instead of overlapping (the same effect cost k_lookup_lds 10 %, EXPERIMENTS.md round 4).
    const long wq = q - lane;
    const long room = noct - 64 - wq - (long)(U - 1) * stride;
    const long stages = room >= 0 ? room / ((long)U * stride) + 1 : 0;
    uint4 A[U], B[U];
    auto load_stage = [&](uint4 (&R)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) R[u] = load_octet(src + (q + u * stride) * 8);
        q += U * stride;
    };
    if (stages > 0) load_stage(A);
#pragma unroll
    for (int r = 0; r < (kWords / 4 + kHistThreads - 1) / kHistThreads; ++r) {                      // 32 KB + the hot words
        const int i = (int)threadIdx.x + r * kHistThreads;
        if ((r + 1) * kHistThreads <= kWords / 4 || i < kWords / 4) reinterpret_cast<uint4 *>(h)[i] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    if (stages > 0) {
        const long pairs = (stages - 1) / 2;                    // iterations in which BOTH refills exist
        for (long p = 0; p < pairs; ++p) {
            load_stage(B);
#pragma unroll
            for (int u = 0; u < U; ++u) add8(A[u]);
            load_stage(A);
#pragma unroll
            for (int u = 0; u < U; ++u) add8(B[u]);
        }
        // one more stage after the one A holds: counted by the code below, through A (with the counting of the last stage
        // written out on both sides of this branch the compiler computes its common part ahead of it and spills)
        if (stages - (2 * pairs + 1) > 0) {
            load_stage(B);
#pragma unroll
            for (int u = 0; u < U; ++u) add8(A[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) A[u] = B[u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) add8(A[u]);
    }
    for (; full(q, 1); q += stride) add8(load_octet(src + q * 8));
    for (; q < noct; q += stride) {
        const uint4 v = load_octet(src + q * 8);
        const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            atomicAdd(&h[kHistCopies * bin_slot<N>(w[k] & 0xffffu)], 1u);
            atomicAdd(&h[kHistCopies * bin_slot<N>(w[k] >> 16)], 1u);
        }
    }
    for (long i = noct * 8 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_body; i += stride)
        atomicAdd(&h[kHistCopies * bin_slot<N>(src[i])], 1u);
    if (blockIdx.x == 0 && (long)threadIdx.x < head) atomicAdd(&h[kHistCopies * bin_slot<N>(src0[threadIdx.x])], 1u);
    __syncthreads();
    if constexpr (Lh > 0) {
        hist_fold_hot<N, Lh, kHistThreads>(h);
        __syncthreads();
    }
    hist_flush<N, CountT, kHistThreads>(h, l, c, C, counts, assign, assign_lut, lut_n, models);
}

// Channel-last [rows][C], C > 1: a workgroup owns 16 consecutive channels of one lambda.
constexpr int kHistTiledThreads = 1024;

template <int N, typename CountT>
__global__ void __launch_bounds__(kHistTiledThreads)
k_hist_tiled(const uint16_t *__restrict__ idx, long n_rows, int C, long E,
             CountT *__restrict__ counts) {
    constexpr int T = table_size(N);
    constexpr int TS = T + 2;
    extern __shared__ unsigned int hs[];
    const int c0 = blockIdx.y * kTileChannels, l = blockIdx.z;
    const int ncg = min(kTileChannels, C - c0);
    for (int i = threadIdx.x; i < kTileChannels * TS; i += blockDim.x) hs[i] = 0;
    __syncthreads();
    const int cl = threadIdx.x & (kTileChannels - 1);
    const int slot = threadIdx.x >> 4;
    const uint16_t *src = idx + (long)l * E;
    if (cl < ncg) {
        for (long r = (long)blockIdx.x * 64 + slot; r < n_rows; r += (long)gridDim.x * 64)
            atomicAdd(&hs[cl * TS + bin_slot<N>(src[r * C + c0 + cl])], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ncg * T; i += blockDim.x) {
        const int ch = i / T, s = i - ch * T;
        const unsigned int v = hs[ch * TS + bin_slot<N>(s)];
        if (v) atomicAdd(&counts[((long)l * C + c0 + ch) * T + s], (CountT)v);
    }
}

// Rows [row_begin, row_end) of the full [L][n_rows x n_ch] index array (lambda planes E = n_rows * n_ch apart).
template <int N, typename CountT>
int launch_hist(const uint16_t *idx, int64_t n_rows, int32_t n_ch, int32_t layout, int32_t L,
                CountT *counts, int64_t row_begin, int64_t row_end, hipStream_t st) {
    const int64_t E = n_rows * (int64_t)n_ch;
    const int64_t n_sub = row_end - row_begin;
    const bool flat = (n_ch == 1) || (layout == VBQ_LAYOUT_CB);
    if (flat) {
        const uint16_t *src = idx + row_begin;
        const int64_t n_per_ch = n_sub;
        const int vec_ok = reinterpret_cast<uintptr_t>(src) % 2 == 0;       // every row finds its own 16-byte boundary (k_hist_flat)
        int64_t gx = (n_per_ch / 8 + kHistThreads - 1) / kHistThreads;
        int64_t cap = (int64_t)2048 / ((int64_t)n_ch * L) + 1;
        if (gx > cap) gx = cap;
        if (gx < 1) gx = 1;
        hipLaunchKernelGGL((k_hist_flat<N, CountT>), dim3((unsigned)gx, (unsigned)n_ch, (unsigned)L), dim3(kHistThreads), 0, st,
                           src, (long)n_per_ch, (long)n_rows, (int)n_ch, (long)E, counts, vec_ok);
        VBQ_CHECK_LAUNCH("hist_flat");
    } else if constexpr (N <= 10) {                              // (N > 10: refused by histogram_entry)
        constexpr int T = table_size(N);
        const size_t lds = sizeof(unsigned int) * kTileChannels * (T + 2);
        {   // per device and cheap: set on every call (a process may drive several GPUs)
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_hist_tiled<N, CountT>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) {
                set_error("hipFuncSetAttribute(%zu B LDS): %s", lds, hipGetErrorString(e));
                return VBQ_ERR_LAUNCH;
            }
        }
        const int groups = (n_ch + kTileChannels - 1) / kTileChannels;
        int64_t gx = 512 / ((int64_t)groups * L) + 1;
        const int64_t iters = (n_sub + 63) / 64;
        if (gx > iters) gx = iters;
        if (gx < 1) gx = 1;
        hipLaunchKernelGGL((k_hist_tiled<N, CountT>), dim3((unsigned)gx, (unsigned)groups, (unsigned)L),
                           dim3(kHistTiledThreads), lds, st, idx + row_begin * n_ch, (long)n_sub, (int)n_ch, (long)E, counts);
        VBQ_CHECK_LAUNCH("hist_tiled");
    }
    return VBQ_OK;
}

int histogram_entry(const char *who, const uint16_t *d_idx, int64_t n_rows, int32_t n_ch, int32_t layout,
                    int32_t n_lambda, int32_t N, void *cnt, bool counts_are_i32, int64_t row_begin, int64_t row_end, void *stream) {
    VBQ_REQUIRE(n_rows >= 0 && n_ch >= 1 && n_lambda >= 1 && n_lambda <= 65535 && n_ch <= 65535,
                VBQ_ERR_INVALID_ARGUMENT, "%s: bad sizes n_rows=%lld n_ch=%d n_lambda=%d", who, (long long)n_rows, n_ch,
                n_lambda);
    VBQ_REQUIRE(0 <= row_begin && row_begin <= row_end && row_end <= n_rows, VBQ_ERR_INVALID_ARGUMENT,
                "%s: row range [%lld, %lld) outside [0, %lld)", who, (long long)row_begin, (long long)row_end, (long long)n_rows);
    VBQ_REQUIRE(row_begin == row_end || (d_idx && cnt), VBQ_ERR_INVALID_ARGUMENT, "%s: null pointer argument", who);
    VBQ_REQUIRE(layout == VBQ_LAYOUT_BC || layout == VBQ_LAYOUT_CB, VBQ_ERR_INVALID_ARGUMENT, "%s: unknown layout %d",
                who, layout);
    VBQ_REQUIRE(!counts_are_i32 || n_rows <= 0x7fffffffLL, VBQ_ERR_INVALID_ARGUMENT,
                "%s: %lld rows per channel can overflow 32-bit counters", who, (long long)n_rows);
    if (row_begin == row_end) return VBQ_OK;
    VBQ_REQUIRE(n_is_built(N), VBQ_ERR_UNSUPPORTED, "%s: max_bits_per_coord N=%d not built (have 4 ... 12; only 10 with VBQ_ONLY_N10)",
                who, N);
    VBQ_REQUIRE(n_ch == 1 || layout == VBQ_LAYOUT_CB || N <= 10, VBQ_ERR_UNSUPPORTED,
                "histogram: N=%d is built for channel-major planes only (VBQ_LAYOUT_CB, or n_ch = 1)", N);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define VBQ_DISPATCH_N(NN)                                                                                                       \
    case NN:                                                                                                                     \
        return counts_are_i32 ? launch_hist<NN, unsigned int>(d_idx, n_rows, n_ch, layout, n_lambda, static_cast<unsigned int *>(cnt), \
                                                              row_begin, row_end, st)                                            \
                              : launch_hist<NN, unsigned long long>(d_idx, n_rows, n_ch, layout, n_lambda,                      \
                                                                    static_cast<unsigned long long *>(cnt), row_begin, row_end, st);
    switch (N) {
        VBQ_FOR_EACH_N(VBQ_DISPATCH_N)
        default: return VBQ_ERR_UNSUPPORTED;                 // not reached: n_is_built(N) was asked above
    }
#undef VBQ_DISPATCH_N
}
}  // namespace
}  // namespace vbq

extern "C" int vbq_histogram_u16(const uint16_t *d_idx, int64_t n_rows, int32_t n_ch, int32_t layout,
                                 int32_t n_lambda, int32_t N, int64_t *d_counts, void *stream) {
    return vbq::histogram_entry("vbq_histogram_u16", d_idx, n_rows, n_ch, layout, n_lambda, N, d_counts, false, 0, n_rows, stream);
}

extern "C" int vbq_histogram_u16_i32(const uint16_t *d_idx, int64_t n_rows, int32_t n_ch, int32_t layout,
                                     int32_t n_lambda, int32_t N, int32_t *d_counts, void *stream) {
    return vbq::histogram_entry("vbq_histogram_u16_i32", d_idx, n_rows, n_ch, layout, n_lambda, N, d_counts, true, 0, n_rows, stream);
}

extern "C" int vbq_histogram_rows_u16(const uint16_t *d_idx, int64_t n_rows, int32_t n_ch, int32_t layout,
                                      int32_t n_lambda, int32_t N, void *d_counts, int32_t counts_are_i32,
                                      int64_t row_begin, int64_t row_end, void *stream) {
    return vbq::histogram_entry("vbq_histogram_rows_u16", d_idx, n_rows, n_ch, layout, n_lambda, N, d_counts, counts_are_i32 != 0,
                                row_begin, row_end, stream);
}

namespace vbq {
namespace {
template <int N, typename CountT>
int launch_hist_assign(const uint16_t *idx, int64_t n_rows, int32_t n_ch, int32_t L, CountT *counts, const float *lut,
                       int64_t lut_n, float *models, hipStream_t st) {
    const int64_t E = n_rows * (int64_t)n_ch;
    const int vec_ok = reinterpret_cast<uintptr_t>(idx) % 2 == 0;           // every row finds its own 16-byte boundary (k_hist_flat)
    // last channel first (measured on the Kodak-24 build of round 2, whose K1 walked the channels in order: 0.7745 against
    // 0.7793 ms per step, three runs each; K1's resident grid of round 3 writes all channels side by side, so what is still in
    // the memory-side cache is the tail of EVERY row and the order no longer matters)
    if (n_ch <= 65535)
        hipLaunchKernelGGL((k_hist_flat<N, CountT>), dim3(1u, (unsigned)L, (unsigned)n_ch), dim3(kHistThreads), 0, st, idx, (long)n_rows,
                           (long)n_rows, (int)n_ch, (long)E, counts, vec_ok, 2, lut, (long)lut_n, models);
    else
        hipLaunchKernelGGL((k_hist_flat<N, CountT>), dim3(1u, (unsigned)n_ch, (unsigned)L), dim3(kHistThreads), 0, st, idx, (long)n_rows,
                           (long)n_rows, (int)n_ch, (long)E, counts, vec_ok, 1, lut, (long)lut_n, models);
    VBQ_CHECK_LAUNCH("hist_assign");
    return VBQ_OK;
}
}  // namespace
}  // namespace vbq

extern "C" int vbq_histogram_models_u16(const uint16_t *d_idx, int64_t n_rows, int32_t n_ch, int32_t n_lambda, int32_t N,
                                        void *d_counts, int32_t counts_are_i32, const float *d_lut, int64_t lut_n,
                                        float *d_models, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n_rows >= 0 && n_ch >= 1 && n_lambda >= 1 && n_lambda <= 65535 && n_ch <= 65535, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_histogram_models_u16: bad sizes n_rows=%lld n_ch=%d n_lambda=%d", (long long)n_rows, n_ch, n_lambda);
    VBQ_REQUIRE(d_idx && d_counts && (!d_models || (d_lut && lut_n >= 1)), VBQ_ERR_INVALID_ARGUMENT,
                "vbq_histogram_models_u16: null pointer argument");
    VBQ_REQUIRE(!counts_are_i32 || n_rows <= 0x7fffffffLL, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_histogram_models_u16: %lld rows per channel can overflow 32-bit counters", (long long)n_rows);
    // (before the memset of d_counts below: the plain histogram would find an N that is not built only after it)
    VBQ_REQUIRE(n_rows == 0 || n_is_built(N), VBQ_ERR_UNSUPPORTED, "vbq_histogram_models_u16: max_bits_per_coord N=%d not built", N);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t n_bins = (int64_t)n_lambda * n_ch * table_size(N);
    // one workgroup per (lambda, channel) is the launch shape of the plain histogram whenever there are at least 2048 rows of
    // bins (cap = 2048 / (C L) + 1 = 1): then the fused form applies; otherwise compose it from the plain entry points
    const bool fused = (int64_t)n_ch * n_lambda >= 2048 && N >= 4 && N <= 12 && n_rows > 0;
    if (fused) {
#define VBQ_DISPATCH_N(NN)                                                                                                   \
    case NN:                                                                                                                 \
        return counts_are_i32 ? launch_hist_assign<NN, unsigned int>(d_idx, n_rows, n_ch, n_lambda,                          \
                                                                     reinterpret_cast<unsigned int *>(d_counts), d_lut, lut_n, \
                                                                     d_models, st)                                           \
                              : launch_hist_assign<NN, unsigned long long>(d_idx, n_rows, n_ch, n_lambda,                    \
                                                                           reinterpret_cast<unsigned long long *>(d_counts), \
                                                                           d_lut, lut_n, d_models, st);
        switch (N) {
            VBQ_FOR_EACH_N(VBQ_DISPATCH_N)
            default: return VBQ_ERR_UNSUPPORTED;             // not reached: n_is_built(N) was asked above
        }
#undef VBQ_DISPATCH_N
    }
    if (hipMemsetAsync(d_counts, 0, (size_t)n_bins * (counts_are_i32 ? 4 : 8), st) != hipSuccess) {
        set_error("vbq_histogram_models_u16: hipMemsetAsync failed");
        return VBQ_ERR_LAUNCH;
    }
    int r = vbq_histogram_rows_u16(d_idx, n_rows, n_ch, VBQ_LAYOUT_CB, n_lambda, N, d_counts, counts_are_i32, 0, n_rows, stream);
    if (r != VBQ_OK || !d_models) return r;
    return vbq_code_lengths_from_counts(d_counts, counts_are_i32, n_bins, d_lut, lut_n, 0, nullptr, d_models, stream);
}

namespace vbq {
namespace {
// out[i] = (period ? i % period : 0) + lut[min(counts[i], lut_n - 1)]
template <typename CountT>
__global__ void __launch_bounds__(256)
k_lut_lengths(const CountT *__restrict__ counts, long n, const float *__restrict__ lut, long lut_n, int period,
              float *__restrict__ out, float *__restrict__ out_model) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        long k = (long)counts[i];
        k = k < 0 ? 0 : (k >= lut_n ? lut_n - 1 : k);
        const float m = lut[k];
        if (out_model) out_model[i] = m;
        if (out) out[i] = period ? __fadd_rn((float)(int)(i % period), m) : m;
    }
}
// period == 0, model output only, n % 4 == 0, 16-byte aligned: 4 entries per thread and iteration (the [L][C][T] model table
// of a Kodak-size build is 16.7 M entries: 67 + 67 MB through this kernel)
template <typename CountT>
__global__ void __launch_bounds__(256)
k_lut_models_v4(const CountT *__restrict__ counts, long n4, const float *__restrict__ lut, long lut_n, float *__restrict__ out) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        long k[4];
        if constexpr (sizeof(CountT) == 4) {
            const int4 c = reinterpret_cast<const int4 *>(counts)[i];
            k[0] = c.x; k[1] = c.y; k[2] = c.z; k[3] = c.w;
        } else {
            const longlong2 a = reinterpret_cast<const longlong2 *>(counts)[2 * i], b = reinterpret_cast<const longlong2 *>(counts)[2 * i + 1];
            k[0] = a.x; k[1] = a.y; k[2] = b.x; k[3] = b.y;
        }
        float m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long kk = k[j] < 0 ? 0 : (k[j] >= lut_n ? lut_n - 1 : k[j]);
            m[j] = lut[kk];
        }
        reinterpret_cast<float4 *>(out)[i] = make_float4(m[0], m[1], m[2], m[3]);
    }
}
}  // namespace
}  // namespace vbq

extern "C" int vbq_code_lengths_from_counts(const void *d_counts, int32_t counts_are_i32, int64_t n,
                                            const float *d_lut, int64_t lut_n, int32_t level_period,
                                            float *d_out_len, float *d_out_model, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n >= 0 && lut_n >= 1 && level_period >= 0, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_code_lengths_from_counts: bad sizes n=%lld lut_n=%lld period=%d", (long long)n, (long long)lut_n, level_period);
    if (n == 0) return VBQ_OK;
    VBQ_REQUIRE(d_counts && d_lut && (d_out_len || d_out_model), VBQ_ERR_INVALID_ARGUMENT,
                "vbq_code_lengths_from_counts: null pointer argument");
    int64_t gx = (n + 255) / 256;
    if (gx > 4096) gx = 4096;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (level_period == 0 && !d_out_len && n % 4 == 0 &&
        ((reinterpret_cast<uintptr_t>(d_counts) | reinterpret_cast<uintptr_t>(d_out_model)) & 15) == 0) {
        int64_t g4 = (n / 4 + 255) / 256;
        if (g4 > 8192) g4 = 8192;
        if (counts_are_i32)
            hipLaunchKernelGGL(k_lut_models_v4<int32_t>, dim3((unsigned)g4), dim3(256), 0, st, reinterpret_cast<const int32_t *>(d_counts),
                               (long)(n / 4), d_lut, (long)lut_n, d_out_model);
        else
            hipLaunchKernelGGL(k_lut_models_v4<long long>, dim3((unsigned)g4), dim3(256), 0, st,
                               reinterpret_cast<const long long *>(d_counts), (long)(n / 4), d_lut, (long)lut_n, d_out_model);
        VBQ_CHECK_LAUNCH("code_lengths_from_counts");
        return VBQ_OK;
    }
    if (counts_are_i32)
        hipLaunchKernelGGL(k_lut_lengths<int32_t>, dim3((unsigned)gx), dim3(256), 0, st, reinterpret_cast<const int32_t *>(d_counts),
                           (long)n, d_lut, (long)lut_n, (int)level_period, d_out_len, d_out_model);
    else
        hipLaunchKernelGGL(k_lut_lengths<long long>, dim3((unsigned)gx), dim3(256), 0, st,
                           reinterpret_cast<const long long *>(d_counts), (long)n, d_lut, (long)lut_n, (int)level_period, d_out_len,
                           d_out_model);
    VBQ_CHECK_LAUNCH("code_lengths_from_counts");
    return VBQ_OK;
}

// ---------------------------------------------------------------------------- packed counters for the all-reduce
// Three 21-bit counters per int64 word: an integer SUM all-reduce of the words adds the three fields
// independently as long as every global count stays below 2^21 (no carry between fields), and moves
// 2.67 instead of 4 bytes per bin over xGMI.  n bins -> ceil(n / 3) words; missing fields are zero.
namespace vbq {
namespace {
__global__ void __launch_bounds__(256)
k_pack3x21(const int32_t *__restrict__ c, long n, long nw, unsigned long long *__restrict__ w, unsigned int limit,
           unsigned int *__restrict__ overflow) {
    bool over = false;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (long)gridDim.x * blockDim.x) {
        const long b = 3 * i;
        const unsigned int f0 = (unsigned int)c[b];
        const unsigned int f1 = b + 1 < n ? (unsigned int)c[b + 1] : 0u;
        const unsigned int f2 = b + 2 < n ? (unsigned int)c[b + 2] : 0u;
        over = over || f0 >= limit || f1 >= limit || f2 >= limit;        // negative counts are huge as unsigned
        w[i] = (unsigned long long)(f0 & 0x1fffffu) | ((unsigned long long)(f1 & 0x1fffffu) << 21) |
               ((unsigned long long)(f2 & 0x1fffffu) << 42);
    }
    if (overflow && __ballot(over) != 0ull && (threadIdx.x & 63) == 0) atomicOr(overflow, 1u);
}
__global__ void __launch_bounds__(256)
k_unpack3x21(const unsigned long long *__restrict__ w, long n, long nw, int32_t *__restrict__ c) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (long)gridDim.x * blockDim.x) {
        const unsigned long long v = w[i];
        const long b = 3 * i;
        c[b] = (int32_t)(v & 0x1fffffu);
        if (b + 1 < n) c[b + 1] = (int32_t)((v >> 21) & 0x1fffffu);
        if (b + 2 < n) c[b + 2] = (int32_t)((v >> 42) & 0x1fffffu);
    }
}
}  // namespace
}  // namespace vbq

extern "C" int vbq_pack_counts_3x21(const int32_t *d_counts, int64_t n, int64_t *d_words, int32_t n_ranks,
                                    uint32_t *d_overflow, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n >= 0, VBQ_ERR_INVALID_ARGUMENT, "vbq_pack_counts_3x21: n < 0");
    VBQ_REQUIRE(n_ranks >= 1 && n_ranks <= (1 << 20), VBQ_ERR_INVALID_ARGUMENT, "vbq_pack_counts_3x21: n_ranks=%d", n_ranks);
    if (n == 0) return VBQ_OK;
    VBQ_REQUIRE(d_counts && d_words, VBQ_ERR_INVALID_ARGUMENT, "vbq_pack_counts_3x21: null pointer");
    const int64_t nw = (n + 2) / 3;
    int64_t gx = (nw + 255) / 256;
    if (gx > 8192) gx = 8192;
    hipLaunchKernelGGL(k_pack3x21, dim3((unsigned)gx), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_counts, (long)n, (long)nw,
                       reinterpret_cast<unsigned long long *>(d_words), (unsigned int)((1u << 21) / (unsigned)n_ranks), d_overflow);
    VBQ_CHECK_LAUNCH("pack_counts");
    return VBQ_OK;
}

extern "C" int vbq_unpack_counts_3x21(const int64_t *d_words, int64_t n, int32_t *d_counts, void *stream) {
    using namespace vbq;
    VBQ_REQUIRE(n >= 0, VBQ_ERR_INVALID_ARGUMENT, "vbq_unpack_counts_3x21: n < 0");
    if (n == 0) return VBQ_OK;
    VBQ_REQUIRE(d_counts && d_words, VBQ_ERR_INVALID_ARGUMENT, "vbq_unpack_counts_3x21: null pointer");
    const int64_t nw = (n + 2) / 3;
    int64_t gx = (nw + 255) / 256;
    if (gx > 8192) gx = 8192;
    hipLaunchKernelGGL(k_unpack3x21, dim3((unsigned)gx), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const unsigned long long *>(d_words), (long)n, (long)nw, d_counts);
    VBQ_CHECK_LAUNCH("unpack_counts");
    return VBQ_OK;
}
