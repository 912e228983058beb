// What the batch kernels over lambda-map files share -- vbq_rans_map_files.hip (every segment of many files written or sized
// under each file's own palette) and vbq_rans_map_rates_files.hip (every file sized under every palette of a list): the walk
// of one lane over its segment, last symbol to first, with a class byte per symbol that picks the index plane the symbol is
// read from and the table it is coded with.  The callers differ in where a class's plane lies and in what a symbol does to
// the coder's state; the order of the symbols and the width of the loads are defined here, once.
#pragma once
#include "vbq_rans_common.h"

namespace vbq {

// Symbols [lo, hi) of one stream, hi - 1 first.  cl[i] is the class byte of symbol i; a byte >= P counts as class 0.
// plane_of(p) is the address of class p's plane of this stream: symbol i of class p is plane_of(p)[i].  put(sym, p) takes
// symbol sym of class p < P.  The tail down to an 8-byte boundary of the classes goes by narrow loads, then eight classes per
// 8-byte load -- and, when the eight agree and that class's plane is 16-byte aligned there, their symbols in one 16-byte load
// --, then the head: the same symbols in the same order whatever the alignment of the file.  Nothing outside cl[lo, hi) and
// plane_of(p)[lo, hi) is read.
template <class PlaneOf, class Put>
__device__ __forceinline__ void map_segment_walk(const uint8_t *cl, long lo, long hi, int P, PlaneOf plane_of, Put put) {
    auto cls_of = [&](unsigned v) -> unsigned { return v < (unsigned)P ? v : 0u; };   // (a class outside the palette: class 0)
    long i = hi;
    while (i > lo && reinterpret_cast<uintptr_t>(cl + i) % 8 != 0) {
        --i;
        const unsigned p = cls_of(cl[i]);
        put(plane_of(p)[i], p);
    }
    for (; i - 8 >= lo; i -= 8) {
        const uint2 cv = *reinterpret_cast<const uint2 *>(cl + i - 8);
        const unsigned c0 = cv.x & 0xffu;
        const unsigned p0 = cls_of(c0);
        const uint16_t *s8 = plane_of(p0) + i - 8;
        if (cv.x == c0 * 0x01010101u && cv.y == cv.x && reinterpret_cast<uintptr_t>(s8) % 16 == 0) {
            const uint4 v = *reinterpret_cast<const uint4 *>(s8);
            put(v.w >> 16, p0); put(v.w & 0xffffu, p0); put(v.z >> 16, p0); put(v.z & 0xffffu, p0);
            put(v.y >> 16, p0); put(v.y & 0xffffu, p0); put(v.x >> 16, p0); put(v.x & 0xffffu, p0);
        } else {
#pragma unroll
            for (int j = 7; j >= 0; --j) {
                const unsigned p = cls_of(((j < 4 ? cv.x : cv.y) >> (8 * (j & 3))) & 0xffu);
                put(plane_of(p)[i - 8 + j], p);
            }
        }
    }
    for (--i; i >= lo; --i) {
        const unsigned p = cls_of(cl[i]);
        put(plane_of(p)[i], p);
    }
}

}  // namespace vbq
