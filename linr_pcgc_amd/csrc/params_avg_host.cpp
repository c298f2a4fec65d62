// linr_params_average_host: one update of K exponential averages of a parameter vector in HOST memory as a plain loop - the twin of
// linr_params_average (csrc/params_avg.hip), and the definition of what the kernel computes.  No GPU involved; compiles without the
// HIP headers (tools/params_average_emul.cpp builds it on its own under the sanitizers).
#include "params_avg.h"
#include <cmath>

extern "C" int linr_params_average_host(const float* params_h, int64_t n, const float* weights_h, int32_t K, int64_t stride, float* avg_h) {
    int rc = linr_avg_check(n, weights_h, K, stride);
    if (rc) return rc < 0 ? rc : 0;
    if (!params_h || !avg_h) return LINR_EINVAL;
    for (int k = 0; k < K; ++k) {
        const float w = weights_h[k];
        float* a = avg_h + k * stride;
        for (int64_t i = 0; i < n; ++i) {
            const float d = params_h[i] - a[i];          // one fp32 rounding: it feeds the multiplicand of an explicit fma, which
            a[i] = std::fmaf(w, d, a[i]);                // no contraction setting can fuse it into
        }
    }
    return 0;
}
