// The wave-interleaved rANS coder (the compact latent file, vbq_amd/bitstream.py, magic "VBQc"; format: include/vbq.h,
// vbq_rans_il_encode_u16) as device functions over ONE part: the lane-to-symbol mapping, the ballot placement of a step's
// words, the decoder's two-register word window and the table staging.  vbq_rans_il.hip (the parts of one tensor) and
// vbq_rans_il_files.hip (the parts of many files) are callers that differ in where a part's geometry comes from; the format
// is defined here, once.
//
// A part is the symbols [a, b) of the S * n symbols of a tensor in stream-major order.  Symbol i of stream s lives at
// idx[s * stride + i] (stride = n: the streams lie back to back) and stream s is coded with the row freq + s * T.  A part may
// start and end inside a stream.  A run is a stretch of the part inside one stream: the tables of that stream are staged into
// LDS at the start of every run, and the lane states carry on from run to run.  One wave (a workgroup of 64) per part.
#pragma once
#include "vbq_rans_common.h"

namespace vbq {

constexpr int kLanes = 64;                                       // the lane count of the FORMAT (and of the workgroup)
constexpr int kStateWords = 2 * kLanes;

// Inclusive prefix sum over the 64 lanes in six DPP adds, no LDS: row_shr 1, 2, 4, 8 scan the rows of 16 lanes (a lane without
// a source adds 0), row_bcast:15 adds the total of row 0 / 2 to row 1 / 3, row_bcast:31 the total of the first 32 lanes to the
// last 32.  (A scan by __shfl_up is six LDS-permute round trips per 64 symbols, and the staging runs once per run.)
__device__ __forceinline__ unsigned wave_incl_scan(unsigned v) {
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 into rows 1 and 3
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 into rows 2 and 3
    return v;
}

// The tables of one stream into LDS, 64 symbols per round (coalesced reads, conflict-free LDS writes; the prefix sum of a round
// is one wave scan plus the carry of the rounds before):
//   fc_l[sym] = f | c << 16       c = exclusive cumulative frequency
// and for the decoder (kDecode)
//   c_l[sym]  = c, c_l[T] = 2^15
//   start[b]  = the symbol whose slot range [c, c + f) holds slot 16 b, by a direct fill of the ranges: a lane fills the range
//               of its own symbol when that is short (f <= 64: at most 5 buckets); a long range -- the one symbol of a near-dead
//               channel that holds nearly all the mass -- is filled by the 64 lanes together.
// Returns whether the row is valid (it sums to 2^15 and no entry is above 2^15 - 1).  For an invalid row the tables are
// garbage but every write stayed inside them; the caller does not decode with them.
template <bool kDecode>
__device__ __forceinline__ bool stage_tables_il(const uint16_t *__restrict__ freq, int T, uint32_t *fc_l, uint16_t *c_l,
                                                uint16_t *start) {
    const int lane = threadIdx.x;
    __syncthreads();                                             // the previous run's reads of the tables are done
    unsigned carry = 0;
    bool big = false;
    for (int base = 0; base < T; base += kLanes) {
        const int i = base + lane;
        const unsigned f = i < T ? (unsigned)freq[i] : 0u;
        const unsigned incl = wave_incl_scan(f);
        const unsigned run = carry + incl - f;
        if (i < T) {
            fc_l[i] = f | (run << 16);
            if (kDecode) c_l[i] = (uint16_t)run;
        }
        if (kDecode) {
            big |= f >= (1u << kPB);
            const unsigned lim = 1u << kPB;                      // an invalid row may run past 2^15: no bucket beyond the table
            const bool wide = f > 64u;
            if (!wide) {
                const unsigned end = run + f < lim ? run + f : lim;
                for (unsigned b = (run + 15u) >> 4; 16u * b < end; ++b) start[b] = (uint16_t)i;
            }
            unsigned long long m = __ballot(wide);
            while (m) {                                          // wave-uniform
                const int src = __ffsll((long long)m) - 1;
                m &= m - 1;
                const unsigned r0 = __shfl(run, src, 64), f0 = __shfl(f, src, 64);
                const unsigned end = r0 + f0 < lim ? r0 + f0 : lim;
                for (unsigned b = ((r0 + 15u) >> 4) + lane; 16u * b < end; b += kLanes) start[b] = (uint16_t)(base + src);
            }
        }
        carry += __shfl(incl, 63, 64);
    }
    const bool ok = carry == (1u << kPB) && !__any(big);
    if (kDecode && lane == 0) c_l[T] = (uint16_t)(1u << kPB);    // > every slot: ends the decoder's walk below T
    __syncthreads();
    return ok;
}

// The encoder over one part.  Runs last to first, steps last to first; in a step every active lane renormalises (emitting at
// most one word) and encodes its symbol.  The words of a step go to [wp - cnt, wp) in ascending lane order: a lane's place is
// the number of emitting lanes below it (a wave ballot).  kWrite = false counts only and gives *size_out the part's words;
// kWrite = true writes the part to payload[off, off + k0) backwards from its end, so that it begins exactly at off with the
// 128 state words -- the caller has checked that this range may be written and that k0 >= 128; k0 is the caller's own (the
// count of the kWrite = false pass): a word that would land below the state words is not written.  canon u16 [S][T] or null:
// symbol canon[s][idx] is coded instead of idx, by one pass over the staged table per run (map_segment_table).
template <bool kWrite>
__device__ __forceinline__ void il_encode_part(const uint16_t *__restrict__ idx, long stride, long n, long a, long b, int T,
                                               const uint16_t *__restrict__ freq, const uint16_t *__restrict__ canon,
                                               uint16_t *__restrict__ payload, long off, long k0,
                                               uint32_t *__restrict__ size_out, uint32_t *fc_l) {
    const int lane = threadIdx.x;
    const long lo = off + kStateWords;                           // the renormalisation words of the part: [lo, wp), written downwards
    long wp = off + k0;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned x = kRansL;
    unsigned count = 0;
    for (long s = (b - 1) / n; s >= a / n; --s) {                // stream of the run (wave-uniform)
        const long rs = s * n > a ? s * n : a;
        const long re = (s + 1) * n < b ? (s + 1) * n : b;
        const int len = (int)(re - rs);
        stage_tables_il<false>(freq + s * T, T, fc_l, nullptr, nullptr);
        if (canon) {
            map_segment_table(canon + s * T, T, fc_l);
            __syncthreads();
        }
        const uint16_t *src = idx + s * stride + (rs - s * n);
        int t = (len - 1) / kLanes;
        unsigned nxt = t * kLanes + lane < len ? (unsigned)src[t * kLanes + lane] : 0u;
        for (; t >= 0; --t) {
            const bool active = t * kLanes + lane < len;
            const unsigned sym = nxt;
            if (t > 0) nxt = src[(t - 1) * kLanes + lane];       // a full step: the next symbol is on its way while this one is coded
            const unsigned fc = fc_l[sym < (unsigned)T ? sym : 0u];   // (an index outside the table: memory-safe)
            const unsigned f = fc & 0xffffu, c = fc >> 16;
            const bool emit = active && x >= (f << (32 - kPB));
            const unsigned long long m = __ballot(emit);
            const int cnt = __popcll(m);
            if (kWrite) {
                wp -= cnt;
                const long at = wp + __popcll(m & below);
                if (emit && at >= lo) payload[at] = (uint16_t)(x & 0xffffu);
            }
            count += (unsigned)cnt;
            if (emit) x >>= 16;
            if (active) x = rans_push(x, f, c);
        }
    }
    if (kWrite) {
        uint16_t *st = payload + off;
        st[2 * lane] = (uint16_t)(x & 0xffffu);
        st[2 * lane + 1] = (uint16_t)(x >> 16);
    } else if (lane == 0) {
        *size_out = count + (unsigned)kStateWords;
    }
}

// The decoder over one part whose words in[0, k0) are UNTRUSTED; the caller has checked that this range may be read and that
// 128 <= k0.  Every read is in[j] with 0 <= j < k0; every symbol written is below T and lies at a position of the part.
// Returns the status bits it found: 2 the part ran out of words, 4 words left over or a final state other than 2^16, 8 an
// invalid frequency row.  With any of them the positions of the part hold garbage below T: the caller zeroes them.
//
// The words come through a two-register window: lane j holds words base + j (`cur`) and base + 64 + j (`nxt`) of the part, a
// lane takes its word from them by a shuffle, and the window moves on by 64 when `cur` is used up: one coalesced load per 64
// words instead of a dependent 2-byte load per lane and step.
__device__ __forceinline__ unsigned il_decode_part(const uint16_t *__restrict__ in, long k0, uint16_t *__restrict__ idx,
                                                   long stride, long n, long a, long b, int T,
                                                   const uint16_t *__restrict__ freq, uint32_t *fc_l, uint16_t *c_l,
                                                   uint16_t *start) {
    const int lane = threadIdx.x;
    unsigned bad = 0;
    unsigned x = (unsigned)in[2 * lane] | ((unsigned)in[2 * lane + 1] << 16);
    long base = kStateWords, rp = kStateWords;                   // window start and next unread word, relative to `in`
    unsigned cur = base + lane < k0 ? (unsigned)in[base + lane] : 0u;
    unsigned nxt = base + kLanes + lane < k0 ? (unsigned)in[base + kLanes + lane] : 0u;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (long s = a / n; s <= (b - 1) / n && !bad; ++s) {        // stream of the run (wave-uniform)
        const long rs = s * n > a ? s * n : a;
        const long re = (s + 1) * n < b ? (s + 1) * n : b;
        const int len = (int)(re - rs);
        if (!stage_tables_il<true>(freq + s * T, T, fc_l, c_l, start)) { bad |= 8u; break; }
        uint16_t *dst = idx + s * stride + (rs - s * n);
        for (int t = 0; t * kLanes < len; ++t) {
            const bool active = t * kLanes + lane < len;
            unsigned sym = 0;
            if (active) sym = rans_pop(x, start, c_l, fc_l);
            const bool need = active && x < kRansL;
            const unsigned long long m = __ballot(need);
            const int cnt = __popcll(m);
            if (rp + cnt > k0) { bad |= 2u; break; }             // wave-uniform: a valid part holds every word its steps take
            const int j = (int)(rp - base) + __popcll(m & below);   // 0 .. 127
            const unsigned w0 = __shfl(cur, j & 63, 64), w1 = __shfl(nxt, j & 63, 64);
            if (need) x = (x << 16) | (j < kLanes ? w0 : w1);
            rp += cnt;
            if (rp - base >= kLanes) {
                base += kLanes;
                cur = nxt;
                nxt = base + kLanes + lane < k0 ? (unsigned)in[base + kLanes + lane] : 0u;
            }
            if (active) dst[t * kLanes + lane] = (uint16_t)sym;
        }
    }
    if (!bad && (rp != k0 || __any(x != kRansL))) bad |= 4u;
    return bad;
}

// Zeros at every position of the part: what a rejected part decodes to.
__device__ __forceinline__ void il_zero_part(uint16_t *__restrict__ idx, long stride, long n, long a, long b) {
    const int lane = threadIdx.x;
    for (long s = a / n; s <= (b - 1) / n; ++s) {
        const long rs = s * n > a ? s * n : a;
        const long re = (s + 1) * n < b ? (s + 1) * n : b;
        uint16_t *dst = idx + s * stride + (rs - s * n);
        for (long i = lane; i < re - rs; i += kLanes) dst[i] = 0;
    }
}

}  // namespace vbq
