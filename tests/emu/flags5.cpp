// fixed4_flags_whole5 (f2q_device.h: the flag gather of a 20-base window that covers five whole quality rows, a byte-wise
// dot product per row) against fixed4_flags, the general gather, on the host.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <algorithm>
#include "../../2fast2q_amd/csrc/f2q_device.h"
using namespace f2q;

// rows: n x 5 x 4 words (five quality rows of a lane's four reads); st: window start, a multiple of 4.  Returns the number
// of reads whose two gathers differ.
extern "C" int fl5_check(const uint32_t *rows, uint32_t n, int st)
{
    const FixedGeom g = fixed_geom_at(st, 20, 30);
    int bad = 0;
    for (uint32_t i = 0; i < n; i++) {
        U4 q[5];
        for (int r = 0; r < 5; r++) { const uint32_t *w = rows + (size_t)i * 20 + 4 * r; q[r] = U4{w[0], w[1], w[2], w[3]}; }
        for (int j = 0; j < 4; j++) bad += fixed4_flags_whole5(q, j) != fixed4_flags(g, q, j);
    }
    return bad;
}
