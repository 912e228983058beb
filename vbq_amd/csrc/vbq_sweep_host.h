// The sorted sweep and its bucket table, as the threshold kernels take them in their arguments: K1t and K1e
// (vbq_quantize_fast.hip, a lambda sweep) and K1nt (vbq_notebook.hip, a beta sweep).  Host code only and nothing from HIP, so
// that tests/host/sweep_table_check.cpp can build it alone under sanitizers; the device side is vbq_sweep.h.
#pragma once
#include <stdint.h>
#include <string.h>

namespace vbq {

constexpr float kSweepBig = 3.0e38f;     // fills the value slots past L; the kernels' "no sweep point here"

// MAXL values at most, NKEYS buckets.  A bucket is one value of key = float bits >> SHIFT (sign, exponent and the top
// 23 - SHIFT mantissa bits); bucket k stands for key0 + k.
template <int MAXL, int NKEYS>
struct SweepTable {
    float val[MAXL];                     // the sweep as f32, ascending; kSweepBig beyond L
    unsigned char perm[MAXL];            // position of val[l] in the caller's order
    int L, key0, nkeys;                  // key0: the key of val[0]; nkeys = last key - key0 + 2, buckets in use
    unsigned char lut[NKEYS];            // lut[k] = #{ l : val[l] below the lower edge of bucket k }
};

// Sort v[0 .. L) and fill S's val, perm, L, key0, nkeys and lut (S: the members of SweepTable, more if it likes; the maximum
// length and the number of keys are the sizes of its val and lut).  false: the sweep is not eligible for the threshold
// kernels -- no value or more than the maximum, a value outside [lo, hi] (NaN included), two values in one bucket (equal
// ones among them), or more octaves than the table has keys for -- and the caller takes its per-point kernel.
template <int SHIFT, class S>
bool build_sweep_table(const float *v, int L, float lo, float hi, S &sw) {
    constexpr int MAXL = (int)(sizeof(S::val) / sizeof(float)), NKEYS = (int)sizeof(S::lut);
    auto key_of = [](float x) {
        uint32_t bits;
        memcpy(&bits, &x, 4);
        return (int)(bits >> SHIFT);
    };
    if (L < 1 || L > MAXL) return false;
    int order[MAXL];
    for (int i = 0; i < L; ++i) order[i] = i;
    for (int i = 1; i < L; ++i)                              // insertion sort by the f32 value
        for (int j = i; j > 0 && v[order[j]] < v[order[j - 1]]; --j) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
    int prev_key = -1;
    for (int i = 0; i < MAXL; ++i) { sw.val[i] = kSweepBig; sw.perm[i] = 0; }
    for (int i = 0; i < L; ++i) {
        const float x = v[order[i]];
        if (!(x >= lo && x <= hi)) return false;
        const int key = key_of(x);
        if (key <= prev_key) return false;                   // two sweep points in one bucket (or equal)
        prev_key = key;
        sw.val[i] = x;
        sw.perm[i] = (unsigned char)order[i];
    }
    sw.key0 = key_of(sw.val[0]);
    sw.nkeys = prev_key - sw.key0 + 2;
    sw.L = L;
    if (sw.nkeys > NKEYS) return false;
    int l = 0;
    for (int k = 0; k < NKEYS; ++k) {
        while (l < L && key_of(sw.val[l]) < sw.key0 + k) ++l;
        sw.lut[k] = (unsigned char)l;
    }
    return true;
}

}  // namespace vbq
