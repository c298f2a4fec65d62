// The weight quantiser of the model codec as element functions for host and device: quant_uniform2 (model_compression/
// model_size_est.py:72-91) and the de-quantisation the coded model is built with (encoder.py:101-103, decoder.py:87), in torch's fp32
// operation order - every operation ONE fp32 rounding.  Shared by linr_params_fake_quant / _host (csrc/fake_quant.hip), by the
// quantisation-aware train steps and by the executors that run from the uint8 codes (bf16_common.h: dequant_code), so that "the
// de-quantised model" is one expression everywhere.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// hipcc contracts a * b + c into an fma by default (-ffp-contract=fast-honor-pragmas), which changes the last bit where the sum
// cancels, so contraction is switched off in each function; the division is IEEE (correctly rounded is hipcc's default for fp32).

// recon = q / sym_max * ten_range + min_n
__host__ __device__ __forceinline__ float linr_fq_dequant(float q, float sym_max, float range, float minv) {
#pragma clang fp contract(off)
    const float t = q / sym_max;
    const float u = t * range;
    return u + minv;
}

// new_p = round((p - min_n) / ten_range * sym_max), round half to even; NaN for a NaN parameter
__host__ __device__ __forceinline__ float linr_fq_level(float p, float sym_max, float range, float minv) {
#pragma clang fp contract(off)
    const float d = p - minv;
    const float t = d / range;
    const float u = t * sym_max;
    return rintf(u);
}

// the integer code of a level: NaN -> 0, never outside [0, sym_max]
__host__ __device__ __forceinline__ uint16_t linr_fq_code(float level, float sym_max) {
    if (!(level >= 0.0f)) return 0;
    return (uint16_t)(level > sym_max ? sym_max : level);
}

// One parameter through the quantiser and back.  range == 0 (all parameters equal; quant_uniform2 itself yields NaN there):
// code 0 and the parameter itself.
__host__ __device__ __forceinline__ float linr_fq_element(float p, float sym_max, float range, float minv, uint16_t& code) {
    if (range == 0.0f) { code = 0; return p; }
    const float level = linr_fq_level(p, sym_max, range, minv);
    code = linr_fq_code(level, sym_max);
    return linr_fq_dequant(level, sym_max, range, minv);
}

// Minimum and maximum that do not depend on the order of the reduction: NaN never wins, and of two zeros the negative one is the
// smaller.  a is the running value (never NaN: it starts at +-INFINITY).
__host__ __device__ __forceinline__ float linr_fq_min(float a, float b) { return (b < a || (b == a && __builtin_signbit(b))) ? b : a; }
__host__ __device__ __forceinline__ float linr_fq_max(float a, float b) { return (b > a || (b == a && !__builtin_signbit(b))) ? b : a; }

// Candidate ranges (linr_params_fake_quant_ranges): a parameter clamped into [lo, hi]; a NaN passes through
#define LINR_FQ_MAX_RANGES 16
__host__ __device__ __forceinline__ float linr_fq_clamp(float p, float lo, float hi) { return p < lo ? lo : (p > hi ? hi : p); }

// mu of the model codec's Laplace model from the exact sum of the codes: torch.round(codes.mean()) in fp32 - the sum as one float
// (exact below 2^24, which 8-bit codes of up to 65,793 parameters are), one division, round half to even
__host__ __device__ __forceinline__ long long linr_fq_mean_level(unsigned long long sum_q, int64_t n) {
    return (long long)rintf((float)sum_q / (float)n);
}

// the one launch behind linr_params_fake_quant, after its argument checks (csrc/fake_quant.hip); the executors wrap it in their
// own profiler class
__attribute__((visibility("hidden")))
int linr_fake_quant_launch(const float* params, int64_t n, int32_t bitdepth, float* qparams, uint16_t* codes, float* minmax,
                           hipStream_t s);
// argument checks shared by the entry and the train steps
__attribute__((visibility("hidden")))
int linr_fake_quant_check(const float* params, int64_t n, int32_t bitdepth, const float* qparams, const uint16_t* codes);
