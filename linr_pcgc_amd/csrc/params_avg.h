// What linr_params_average (csrc/params_avg.hip) and its host twin (csrc/params_avg_host.cpp) share: the argument checks both make
// alike.  Plain C++, no HIP header: the twin compiles on its own (tools/params_average_emul.cpp builds it under the sanitizers).
#pragma once
#include "../../include/linr_hip.h"

#define LINR_AVG_MAX 4          // rows of one call: linr_overfit_avg.weight has as many slots

// Everything the entry and its twin refuse alike (pointers and alignment apart).  0: go on; 1: n == 0, nothing to do.
static inline int linr_avg_check(int64_t n, const float* weights_h, int32_t K, int64_t stride) {
    if (n < 0 || K < 1 || K > LINR_AVG_MAX || !weights_h) return LINR_EINVAL;
    for (int k = 0; k < K; ++k)
        if (!(weights_h[k] > 0.0f && weights_h[k] <= 1.0f)) return LINR_EINVAL;          // outside (0, 1], or NaN
    if (stride < n || (stride & 3)) return LINR_EINVAL;
    return n == 0 ? 1 : 0;
}

#ifdef __HIPCC__
// the device entry's checks, pointers and alignment included (0: go on; 1: n == 0; < 0: refused), and the one launch behind them in
// profiler / poison class 12 (csrc/params_avg.hip); linr_overfit_gop_avg queues the same launch behind every step
__attribute__((visibility("hidden")))
int linr_params_average_check(const float* params, int64_t n, const float* weights_h, int32_t K, int64_t stride, const float* avg);
__attribute__((visibility("hidden")))
int linr_params_average_launch(const float* params, int64_t n, const float* weights_h, int32_t K, int64_t stride, float* avg, hipStream_t s);
#endif
