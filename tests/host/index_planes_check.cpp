// index_planes_within_4gb (vbq_amd/csrc/vbq_index_planes.h) at its boundary values, against its definition in wider
// arithmetic.  A stand-alone program: exit status 0 and nothing on stderr is a pass.
#include <stdint.h>
#include <stdio.h>

#include "vbq_index_planes.h"

static int failures = 0;

static void expect(int64_t L, int64_t E, bool want) {
    const bool got = vbq::index_planes_within_4gb(L, E);
    if (got != want) {
        fprintf(stderr, "index_planes_within_4gb(%lld, %lld) = %d, expected %d\n", (long long)L, (long long)E, (int)got, (int)want);
        ++failures;
    }
}

// the definition: the last byte of the last plane, 2 * E * L - 1, is at most 2^32 - 2 from out_idx
static bool definition(int64_t L, int64_t E) {
    if (L < 1 || E < 1) return false;
    const unsigned __int128 bytes = (unsigned __int128)(uint64_t)L * 2u * (uint64_t)E;
    return bytes <= (unsigned __int128)0xffffffffull;
}

int main() {
    const int64_t G4 = 1ll << 32;
    // one plane: 2 E <= 2^32 - 1
    expect(1, (G4 - 1) / 2, true);
    expect(1, (G4 - 1) / 2 + 1, false);
    expect(1, 1, true);
    // the headline shape and its neighbours: 32 planes of 36864 x 256 indices are 604 MB
    expect(32, 36864ll * 256, true);
    // 32 planes: E <= floor((2^32 - 1) / 64) = 2^26 - 1
    expect(32, (1ll << 26) - 1, true);
    expect(32, 1ll << 26, false);
    expect(16, (1ll << 27) - 1, true);
    expect(16, 1ll << 27, false);
    expect(3, 715827882, true);                               // 6 * 715827882 = 2^32 - 4
    expect(3, 715827883, false);                              // 2^32 + 2
    // nothing to address, and arguments whose product leaves 64 bits
    expect(0, 10, false);
    expect(10, 0, false);
    expect(-1, 10, false);
    expect(10, -1, false);
    expect(INT64_MAX, INT64_MAX, false);
    expect(INT64_MAX, 1, false);
    expect(1, INT64_MAX, false);
    expect(G4, 1, false);
    expect(G4 / 2, 1, false);
    expect(G4 / 2 - 1, 1, true);
    // a band around every boundary against the definition
    for (int64_t L = 1; L <= 33; ++L) {
        const int64_t edge = (G4 - 1) / (2 * L);
        for (int64_t d = -3; d <= 3; ++d) expect(L, edge + d, definition(L, edge + d));
    }
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    return failures ? 1 : 0;
}
