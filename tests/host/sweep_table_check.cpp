// Stand-alone check of build_sweep_table (vbq_amd/csrc/vbq_sweep_host.h) against its definition, by brute force, for the two
// parametrisations in use: the lambda sweeps of K1t / K1e (32 values, key shift 16, 2048 keys, 1.9e-12 .. 1.8e19) and the
// beta sweep of K1nt (64, 17, 1536, 2e-12 .. 2e18).  tests/test_sweep_table_host.py builds it with the host compiler under the
// address and undefined-behaviour sanitizers and runs it; the exit status is the verdict, the findings go to stderr.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "vbq_sweep_host.h"

using vbq::build_sweep_table;
using vbq::kSweepBig;
using vbq::SweepTable;

static int failures = 0;
#define EXPECT(cond, ...)                         \
    do {                                          \
        if (!(cond)) {                            \
            ++failures;                           \
            std::fprintf(stderr, "FAIL %s:%d [%s] %s: ", __FILE__, __LINE__, what, #cond); \
            std::fprintf(stderr, __VA_ARGS__);    \
            std::fprintf(stderr, "\n");           \
        }                                         \
    } while (0)

static float from_bits(uint32_t b) {
    float x;
    memcpy(&x, &b, 4);
    return x;
}
static uint32_t bits_of(float x) {
    uint32_t b;
    memcpy(&b, &x, 4);
    return b;
}

template <int MAXL, int SHIFT, int NKEYS>
struct Param {
    float lo, hi;
    static int key(float x) { return (int)(bits_of(x) >> SHIFT); }

    // An eligible sweep: every field against the definition.
    void accepted(const char *what, const std::vector<float> &v) const {
        SweepTable<MAXL, NKEYS> sw;
        memset(&sw, 0xa5, sizeof(sw));
        const int L = (int)v.size();
        const bool ok = build_sweep_table<SHIFT>(v.data(), L, lo, hi, sw);
        EXPECT(ok, "refused, L = %d", L);
        if (!ok) return;
        EXPECT(sw.L == L, "L = %d, expected %d", sw.L, L);
        std::vector<int> seen(L, 0);
        for (int i = 0; i < L; ++i) {
            const int p = sw.perm[i];
            EXPECT(p < L, "perm[%d] = %d", i, p);
            if (p >= L) return;
            ++seen[p];
            EXPECT(bits_of(sw.val[i]) == bits_of(v[p]), "val[%d] = %a, v[perm] = %a", i, sw.val[i], v[p]);
            if (i > 0) EXPECT(sw.val[i - 1] < sw.val[i], "val[%d] = %a not above val[%d] = %a", i, sw.val[i], i - 1, sw.val[i - 1]);
        }
        for (int i = 0; i < L; ++i) EXPECT(seen[i] == 1, "index %d appears %d times in perm", i, seen[i]);
        for (int i = L; i < MAXL; ++i) EXPECT(sw.val[i] == kSweepBig, "unused slot %d holds %a", i, sw.val[i]);
        int kmin = key(v[0]), kmax = kmin;
        for (float x : v) {
            kmin = key(x) < kmin ? key(x) : kmin;
            kmax = key(x) > kmax ? key(x) : kmax;
        }
        EXPECT(sw.key0 == kmin, "key0 = %d, expected %d", sw.key0, kmin);
        EXPECT(sw.nkeys == kmax - kmin + 2, "nkeys = %d, expected %d", sw.nkeys, kmax - kmin + 2);
        for (int k = 0; k < NKEYS; ++k) {
            int below = 0;
            for (float x : v) below += key(x) < kmin + k ? 1 : 0;
            EXPECT(sw.lut[k] == below, "lut[%d] = %d, expected %d", k, sw.lut[k], below);
        }
    }

    void refused(const char *what, const std::vector<float> &v) const {
        SweepTable<MAXL, NKEYS> sw;
        EXPECT(!build_sweep_table<SHIFT>(v.data(), (int)v.size(), lo, hi, sw), "accepted, L = %d", (int)v.size());
    }

    // MAXL values in MAXL consecutive buckets from `first` on, then the shared cases.
    void common(float first) const {
        const float inf = std::numeric_limits<float>::infinity();
        const float eps_same = std::ldexp(1.0f, SHIFT - 23 - 2), eps_next = std::ldexp(1.0f, SHIFT - 23);  // in [1, 2) a bucket is 2^(SHIFT-23) wide
        accepted("single value", {0.37f});
        accepted("adjacent buckets", {1.0f, 1.0f + eps_next, 4.0f});
        refused("two values in one bucket", {1.0f, 1.0f + eps_same, 4.0f});
        refused("two values in one bucket, far ends of it", {4.0f, 1.0f + eps_next - std::ldexp(1.0f, -23), 1.0f});
        refused("a repeated value", {2.0f, 0.5f, 2.0f});
        refused("no value", {});
        refused("NaN", {1.0f, std::numeric_limits<float>::quiet_NaN(), 4.0f});
        refused("NaN alone", {std::numeric_limits<float>::quiet_NaN()});
        std::vector<float> longest;
        for (int i = 0; i < MAXL; ++i) longest.push_back(from_bits(bits_of(first) + ((uint32_t)i << SHIFT)));
        accepted("the longest admissible sweep, consecutive buckets", longest);
        longest.push_back(1.0e6f);
        refused("one value more than the maximum", longest);
        // too many octaves: the last key NKEYS - 2 above the first fills the table, one more does not fit
        const float last_in = from_bits(bits_of(first) + ((uint32_t)(NKEYS - 2) << SHIFT));
        const float last_out = from_bits(bits_of(first) + ((uint32_t)(NKEYS - 1) << SHIFT));
        const float mid = from_bits(bits_of(first) + (5u << SHIFT));
        accepted("nkeys equal to the key count", {last_in, first, mid});
        refused("nkeys one above the key count", {last_out, first, mid});
        // the value range, each end on both sides
        accepted("lower end of the range", {4.0f * lo, lo});
        refused("below the range", {4.0f * lo, std::nextafter(lo, 0.0f)});
        accepted("upper end of the range", {0.25f * hi, hi});
        refused("above the range", {0.25f * hi, std::nextafter(hi, inf)});
        refused("zero", {0.0f, 1.0f});
        refused("negative", {-1.0f, 1.0f});
        refused("infinity", {1.0f, inf});
    }
};

int main() {
    const Param<32, 16, 2048> lam{1.9e-12f, 1.8e19f};
    const Param<64, 17, 1536> beta{2e-12f, 2e18f};
    std::vector<float> lam16, lam32, desc, wide, beta50;
    for (int i = 0; i < 16; ++i) lam16.push_back((float)std::pow(2.0, -8.0 + i));                  // post_process.py:115
    for (int i = 0; i < 32; ++i) lam32.push_back((float)std::pow(2.0, -8.0 + 15.5 * i / 31.0));    // 2 ** linspace(-8, 7.5, 32)
    for (int i = 0; i < 50; ++i)                                                                    // ipynb cell 32, b = fl32(2 beta)
        beta50.push_back((float)(2.0 * std::exp(std::log(0.01) + (std::log(1.0e5) - std::log(0.01)) * i / 49.0)));
    for (int i = 0; i < 16; ++i) desc.push_back((float)std::pow(2.0, 7.0 - i));
    for (int i = 0; i < 19; ++i) wide.push_back((float)std::pow(2.0, -10.0 + i));                  // 18 octaves
    lam.accepted("16 lambdas 2^-8 .. 2^7", lam16);
    lam.accepted("32 lambdas 2^linspace(-8, 7.5)", lam32);
    lam.accepted("descending", desc);
    lam.refused("50 values in a 32-value table", beta50);
    lam.refused("18 octaves in a 16-octave table", wide);
    lam.common(1.0f);
    beta.accepted("16 lambdas as betas", lam16);
    beta.accepted("32 lambdas as betas", lam32);
    beta.accepted("the notebook's 50 betas", beta50);
    beta.accepted("the notebook's 50 betas, descending", std::vector<float>(beta50.rbegin(), beta50.rend()));
    beta.accepted("descending", desc);
    beta.accepted("18 octaves in a 24-octave table", wide);
    beta.common(std::ldexp(1.0f, -20));
    if (failures) std::fprintf(stderr, "%d check(s) failed\n", failures);
    return failures ? 1 : 0;
}
