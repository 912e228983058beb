// Where the index planes of a launch lie, as the solve kernels' launchers ask (K1 and K1e, vbq_quantize_fast.hip).  Host code
// only and nothing from HIP, so that tests/host/index_planes_check.cpp can build it alone.
#pragma once
#include <stdint.h>

namespace vbq {

// L planes of u16 indices, plane l at out_idx + l * E elements, every store of a plane inside its E elements: true when the
// last byte of the last plane lies within 4 GB - 1 of out_idx.  Then one buffer descriptor over out_idx (its range field
// holds 2^32 - 1 bytes) reaches every store: a 32-bit byte offset inside the plane in a vector register, the plane's byte
// offset l * 2 E as the instruction's 32-bit scalar offset, their sum below 2^32.  Nothing to address (L or E below 1) is false.
inline bool index_planes_within_4gb(int64_t L, int64_t E) {
    if (L < 1 || E < 1) return false;
    if ((uint64_t)E > 0xffffffffull / 2ull) return false;     // one plane alone is too long (and 2 * E * L cannot wrap below)
    if ((uint64_t)L > 0xffffffffull) return false;
    return (uint64_t)L * (2ull * (uint64_t)E) <= 0xffffffffull;
}

}  // namespace vbq
