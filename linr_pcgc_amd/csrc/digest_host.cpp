// linr_coords_digest_host: the geometry digest (csrc/digest_body.h) of rows in HOST memory as a plain loop - the twin of
// linr_coords_digest_segments (csrc/digest.hip) for one segment.  No GPU involved; compiles without the HIP headers
// (tools/digest_emul.cpp builds it on its own under the sanitizers).
#include "../../include/linr_hip.h"
#include "digest_body.h"

extern "C" uint64_t linr_coords_digest_host(const int32_t* coords_h, int64_t n, const int32_t* origin_h) {
    if (n < 0 || !coords_h) n = 0;
    const int32_t ox = origin_h ? origin_h[0] : 0, oy = origin_h ? origin_h[1] : 0, oz = origin_h ? origin_h[2] : 0;
    uint64_t sum = 0;
    for (int64_t i = 0; i < n; ++i) sum += dg_row(coords_h[3 * i], coords_h[3 * i + 1], coords_h[3 * i + 2], ox, oy, oz);
    return dg_finish(sum, (uint64_t)n);
}
