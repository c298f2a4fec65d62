// Averaged weights (opt-in; include/linr_hip.h: linr_params_average): K exponential averages of the flat parameter vector, each
// advanced by one update  avg[k][i] = fma(w_k, params[i] - avg[k][i], avg[k][i])  behind a training step.  The encoder may then code
// an average of the iterates instead of the last one (codec.search_average); csrc/params_avg_host.cpp is the same arithmetic as a
// plain loop and the definition of what is computed here.
//
// ONE launch for all K rows: a lane loads a float4 of the parameters once and walks the rows with it, 16-byte loads and stores, the
// 0..3 floats behind the last whole float4 element by element.  The vector is small (54,712 floats at scale_num 7: 54 workgroups), so
// the launch is latency, not bandwidth; the grid is capped and strides for larger vectors.  The weights travel as a kernel argument.
// No atomics, no reduction, nothing of the library's is read or kept: every element depends on itself alone.
#include "common.h"
#include "params_avg.h"
#include "prof.h"

namespace {

struct AvgWeights { float w[LINR_AVG_MAX]; };          // by value: 16 bytes of kernel argument

// the difference rounded to fp32 on its own, then one fused multiply-add: explicit, so that no contraction setting changes it
__device__ __forceinline__ float avg_step(float w, float p, float a) { return __fmaf_rn(w, __fsub_rn(p, a), a); }

// params 16-byte aligned, avg 16-byte aligned with stride % 4 == 0 (so every row is), stride >= n, K in 1..LINR_AVG_MAX, n >= 1
__global__ __launch_bounds__(LINR_BLOCK) void params_average_k(const float* __restrict__ params, int64_t n, AvgWeights wt, int K,
                                                               int64_t stride, float* __restrict__ avg) {
    const int64_t n4 = n >> 2;
    const int64_t t = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x, step = (int64_t)gridDim.x * LINR_BLOCK;
    const float4* p4 = reinterpret_cast<const float4*>(params);
    for (int64_t i = t; i < n4; i += step) {
        const float4 p = p4[i];
#pragma unroll
        for (int k = 0; k < LINR_AVG_MAX; ++k) {
            if (k < K) {                                 // uniform
                float4* a4 = reinterpret_cast<float4*>(avg + k * stride);
                float4 a = a4[i];
                const float w = wt.w[k];
                a.x = avg_step(w, p.x, a.x); a.y = avg_step(w, p.y, a.y); a.z = avg_step(w, p.z, a.z); a.w = avg_step(w, p.w, a.w);
                a4[i] = a;
            }
        }
    }
    const int64_t j = (n4 << 2) + t;                     // the tail: lanes 0..2 of the first workgroup
    if (j < n) {
        const float p = params[j];
#pragma unroll
        for (int k = 0; k < LINR_AVG_MAX; ++k)
            if (k < K) avg[k * stride + j] = avg_step(wt.w[k], p, avg[k * stride + j]);
    }
}

}  // namespace

int linr_params_average_check(const float* params, int64_t n, const float* weights_h, int32_t K, int64_t stride, const float* avg) {
    int rc = linr_avg_check(n, weights_h, K, stride);
    if (rc) return rc;
    if (!params || !avg) return LINR_EINVAL;
    if (!linr_aligned16(params) || !linr_aligned16(avg)) return LINR_EALIGN;
    return 0;
}

int linr_params_average_launch(const float* params, int64_t n, const float* weights_h, int32_t K, int64_t stride, float* avg, hipStream_t s) {
    AvgWeights wt;
    for (int k = 0; k < LINR_AVG_MAX; ++k) wt.w[k] = weights_h[k < K ? k : 0];
    // a float4 per lane; at most 2048 workgroups, which stride over what is left
    const int64_t b = ((n >> 2) + LINR_BLOCK - 1) / LINR_BLOCK;
    const unsigned grid = (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
    ProfScope ps(s, PK_MISC, 0);
    params_average_k<<<grid, LINR_BLOCK, 0, s>>>(params, n, wt, K, stride, avg);
    return linr_launch_rc();
}

extern "C" int linr_params_average(const float* params, int64_t n, const float* weights_h, int32_t K, int64_t stride, float* avg, void* stream) {
    int rc = linr_params_average_check(params, n, weights_h, K, stride, avg);
    if (rc) return rc < 0 ? rc : 0;
    return linr_params_average_launch(params, n, weights_h, K, stride, avg, (hipStream_t)stream);
}
