// What the rANS coders share -- vbq_rans.hip (segments, one lane per segment), vbq_rans_map.hip (the same with a table per
// symbol) and vbq_rans_il.hip (parts, the 64 lanes of a wave together): the coder's constants and the per-symbol state updates
// of the encoder and of the decoder.  32-bit state, start state 2^16, 16-bit renormalisation words, 15 probability bits;
// format: include/vbq.h.  How the tables reach LDS is each kernel's own business (the staging routines map lanes to symbols
// differently).
#pragma once
#include "vbq_common.h"

namespace vbq {

constexpr int kPB = 15;
constexpr unsigned kRansL = 1u << 16;

// x / f and x % f for 1 <= f < 2^15 and x < f 2^17 (the encoder's invariant after renormalisation) without the ~35-instruction
// expansion of a 32-bit division: the quotient is below 2^17, a float estimate of it is off by at most one, and the remainder says
// which way (exact by construction: the result is verified, not trusted).
__device__ __forceinline__ void divmod_small(unsigned x, unsigned f, unsigned &q, unsigned &r) {
    q = (unsigned)(__uint2float_rn(x) * __builtin_amdgcn_rcpf(__uint2float_rn(f)));
    int rr = (int)(x - q * f);
    if (rr < 0) { rr += (int)f; --q; }
    if (rr >= (int)f) { rr -= (int)f; ++q; }
    r = (unsigned)rr;
}

// The encoder's step: the renormalised state x takes the symbol of frequency f and exclusive cumulative frequency c.
__device__ __forceinline__ unsigned rans_push(unsigned x, unsigned f, unsigned c) {
    unsigned q, r;
    divmod_small(x, f, q, r);
    return (q << kPB) + r + c;
}

// The decoder's step, before its renormalisation: the symbol whose slot range [c, c + f) holds the state's slot, and the state
// without it.  Tables in LDS: fc_l[sym] = f | c << 16, c_l[sym] = c with c_l[T] = 2^15, start[b] = the symbol whose range holds
// slot 16 b -- the search begins there and walks up (a bucket of 16 slots holds one symbol on average; empty ranges are skipped).
__device__ __forceinline__ unsigned rans_pop(unsigned &x, const uint16_t *start, const uint16_t *c_l, const uint32_t *fc_l) {
    const unsigned slot = x & ((1u << kPB) - 1u);
    unsigned sym = start[slot >> 4];                             // last symbol with c <= slot
    while (c_l[sym + 1] <= slot) ++sym;                          // c_l[T] = 2^15 > slot ends the walk below T
    const unsigned fc = fc_l[sym];
    x = (fc & 0xffffu) * (x >> kPB) + slot - (fc >> 16);
    return sym;
}

// The same step without the fc table: f = c[sym + 1] - c[sym], for a decoder that keeps several tables in LDS at once
// (vbq_rans_map.hip) and has no room for a third array per table.
__device__ __forceinline__ unsigned rans_pop(unsigned &x, const uint16_t *start, const uint16_t *c_l) {
    const unsigned slot = x & ((1u << kPB) - 1u);
    unsigned sym = start[slot >> 4];
    unsigned c1 = c_l[sym + 1];
    while (c1 <= slot) c1 = c_l[++sym + 1];
    const unsigned c0 = c_l[sym];
    x = (c1 - c0) * (x >> kPB) + slot - c0;
    return sym;
}

}  // namespace vbq
