// What the threshold kernels share -- K1t (k_level_counts_hull) and K1e (k_quant_hull_idx) in vbq_quantize_fast.hip, K1nt
// (k_quant_notebook_hull) in vbq_notebook.hip: a whole lambda (or beta) sweep solved from the lower envelope of the eleven
// cost lines of an element.  Ten thresholds, their positions in the sorted sweep through a bucket table, a guard band around
// each; the mathematics and the exactness argument stand at K1t.  The host side (sorting, the bucket table) is
// vbq_sweep_host.h.  The f32 pieces only: K1nt's f64 scoring stays in its file.
//
// Every kernel here must keep its instruction stream when a piece moves (tools/isa_diff.py): where a kernel restates a
// routine of this header inline, sharing changed its code, and a comment there names the routine.
#pragma once
#include "vbq_common.h"
#include "vbq_sweep_host.h"

namespace vbq {

// v_min_f32 / v_max_f32 as they are (IEEE mode: a NaN operand loses).  fminf / fmaxf make the compiler canonicalise
// operands it cannot prove quiet (a v_max x, x in front of every second min of the threshold recurrences).
__device__ __forceinline__ float vmin(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vmax(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vmax3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float vmin3abs(float a, float b, float c) {       // min(|a|, |b|, |c|)
    float r;
    asm("v_min3_f32 %0, |%1|, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// The ten thresholds T_n = max_{j > n} min_{i <= n} (du_i - du_j) / (j - i) of an element, clamped into the tables' range
// (inf / NaN only come from non-finite costs, which are flagged separately).
template <int N>
__device__ __forceinline__ void sweep_thresholds(const float (&du)[N + 1], float (&Tn)[N]) {
    constexpr int N1 = N + 1;
    float Pm[N1];                                              // Pm[j] = min_{i <= n} (du_i - du_j) / (j - i)
#pragma unroll
    for (int n = 0; n < N; ++n) {
#pragma unroll
        for (int j = n + 1; j < N1; ++j) {
            const float r = __fmul_rn(__fsub_rn(du[n], du[j]), 1.0f / (float)(j - n));
            Pm[j] = n == 0 ? r : vmin(Pm[j], r);
        }
        float t = Pm[n + 1];
        int j = n + 2;
#pragma unroll
        for (; j + 1 < N1; j += 2) t = vmax3(t, Pm[j], Pm[j + 1]);
        if (j < N1) t = vmax(t, Pm[j]);
        Tn[n] = vmin(t, 1.0e38f);
    }
}

// The largest distortion of an element: not below kSweepBig, or not a number, sends the element to the literal scan.
template <int N>
__device__ __forceinline__ float sweep_max_du(const float (&du)[N + 1]) {
    constexpr int N1 = N + 1;
    float big = du[0];
#pragma unroll
    for (int j = 1; j + 1 < N1; j += 2) big = vmax3(big, du[j], du[j + 1]);
    if ((N1 & 1) == 0) big = vmax(big, du[N1 - 1]);
    return big;
}

// Bucket of a threshold: its bit pattern shifted (an arithmetic shift keeps T <= 0 negative, so one median clamps "below the
// sweep", "above it" and the table range).
// The median is written out: min(max(x, 0), nkeys - 1) only folds into one when the compiler can prove 0 <= nkeys - 1, and
// from a kernel argument it cannot (it emits v_max_i32 and v_min_i32, three 4-cycle instructions with the subtraction).
// nkeys >= 2 on every table build_sweep_table accepts (vbq_sweep_host.h), so the median of { x, 0, nkeys - 1 } is the clamp.
template <int SHIFT>
__device__ __forceinline__ int sweep_bucket(float t, int key0, int nkeys) {
    const int x = ((int)__float_as_uint(t) >> SHIFT) - key0;
    int r;
    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(x), "s"(nkeys - 1));
    return r;
}

// Position of a threshold in the sorted sweep, a = #{ l : val_(l) < T }: the count of sweep points below its bucket, then the
// one sweep point that may share the bucket.  nb = { val_(cnt-1), val_(cnt), val_(cnt+1) }: T lies between the outer two,
// so its distance to the sweep is the smallest of the three distances.
template <int SHIFT>
__device__ __forceinline__ uint32_t sweep_position(float t, int key0, int nkeys, const unsigned char *lut, const float4 *rec,
                                                   float4 &nb) {
    const uint32_t cnt = lut[sweep_bucket<SHIFT>(t, key0, nkeys)];
    nb = rec[cnt];
    return cnt + (nb.y < t ? 1u : 0u);                        // val_(a-1) < T <= val_(a)
}

// Guard band |lambda - T_n| <= 2^-20 (du_n + |T_n| (n + 1)): every sweep point outside it is decided by the lines.
__device__ __forceinline__ float sweep_band(float t, int n, float du_n) {
    return __fmul_rn(fmaf(fabsf(t), (float)(n + 1), du_n), 9.5367431640625e-07f);
}

// Distance of a threshold to the sweep, from the three neighbours sweep_position left in nb.
__device__ __forceinline__ float sweep_distance(float t, const float4 &nb) {
    return vmin3abs(__fsub_rn(t, nb.x), __fsub_rn(t, nb.y), __fsub_rn(t, nb.z));
}

// Prologue: entry i of the neighbour table, rec[i] = { val[i-1], val[i], val[i+1], - } with -big / +big outside the sweep
// (i in 0 .. MAXL + 1), and the bucket table out of the kernel arguments into LDS.
template <int MAXL>
__device__ __forceinline__ float4 sweep_rec(const float (&val)[MAXL], int L, int i) {
    auto at = [&](int l) { return l < 0 ? -kSweepBig : (l < L ? val[l < MAXL ? l : MAXL - 1] : kSweepBig); };
    return make_float4(at(i - 1), at(i), at(i + 1), 0.0f);
}
template <int NKEYS>
__device__ __forceinline__ void stage_sweep_lut(unsigned char *lut, const unsigned char (&arg)[NKEYS]) {
    for (int k = threadIdx.x; k < NKEYS / 4; k += blockDim.x)
        reinterpret_cast<uint32_t *>(lut)[k] = reinterpret_cast<const uint32_t *>(arg)[k];
}

// Emission (K1e, K1nt): byte offset of a rank in the lane's rank table for sweep point j of a word.  P holds the word's eight
// running sums of "levels lost" in 4-bit fields; field j, the level index N - level, goes to bits 10 .. 13 over the lane's
// part `base` (bits 0 .. 9): a shift and one v_and_or_b32.
__device__ __forceinline__ uint32_t sweep_rank_offset(uint32_t P, int j, uint32_t base) {
    const uint32_t sh = j < 3 ? (P << (10 - 4 * j)) : (P >> (4 * j - 10));
    return (sh & 0x3c00u) | base;
}

}  // namespace vbq
