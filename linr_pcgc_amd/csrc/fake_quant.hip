// The model codec's weight quantiser on the device: qparams = dequant(quant_uniform2(params)) (model_compression/model_size_est.py:
// 72-91, encoder.py:101-103), bit for bit what the CPU codec computes in fp32 (csrc/fake_quant.h holds the arithmetic).  The
// quantisation-aware train steps (linr_net_train_step_qat, linr_net_train_step_bf16_qat) evaluate the network at its output.
//
// ONE launch of ONE workgroup of 1024 lanes: the global minimum and maximum stand between reading a parameter and quantising it, and
// a grid-wide reduction would cost a second launch or float atomics.  The parameter vector is small (54,712 floats = 214 KB at
// scale_num 7), so every lane keeps its share in registers between the two passes: 16-byte loads, a wave reduction by lane
// exchange, 16 wave results through LDS (written, barrier, read), then the quantise pass out of the registers - params is read once.
// A vector that does not fit (more than FQ_HELD floats) is read a second time in the same stride loop.  Minimum and maximum are
// exact, so the tree's shape does not matter.
#include "common.h"
#include "fake_quant.h"
#include "prof.h"

namespace {

constexpr int FQ_LANES = 1024;
constexpr int FQ_V4 = 16;                                   // float4 registers a lane may hold: 64 VGPRs of the 128 a 16-wave block has
constexpr int64_t FQ_HELD = (int64_t)FQ_LANES * FQ_V4 * 4;  // 65,536 floats

struct FqRange { float mn, mx; };

__device__ __forceinline__ void fq_see(FqRange& r, float x) { r.mn = linr_fq_min(r.mn, x); r.mx = linr_fq_max(r.mx, x); }
__device__ __forceinline__ void fq_see(FqRange& r, const float4& v) { fq_see(r, v.x); fq_see(r, v.y); fq_see(r, v.z); fq_see(r, v.w); }

__device__ __forceinline__ void fq_put(const float4& v, int64_t i4, float sym_max, float range, float minv, float4* __restrict__ q4,
                                       ushort4* __restrict__ c4) {
    uint16_t cx, cy, cz, cw;
    float4 o;
    o.x = linr_fq_element(v.x, sym_max, range, minv, cx);
    o.y = linr_fq_element(v.y, sym_max, range, minv, cy);
    o.z = linr_fq_element(v.z, sym_max, range, minv, cz);
    o.w = linr_fq_element(v.w, sym_max, range, minv, cw);
    q4[i4] = o;
    if (c4) c4[i4] = make_ushort4(cx, cy, cz, cw);
}

// params / qparams 16-byte aligned, codes 8-byte aligned or NULL; n >= 1
__global__ __launch_bounds__(FQ_LANES) void fake_quant_k(const float* params, int64_t n, float sym_max, float* qparams, uint16_t* codes,
                                                         float* __restrict__ minmax) {
    __shared__ float s_mn[FQ_LANES / LINR_WAVE], s_mx[FQ_LANES / LINR_WAVE];
    const int tid = threadIdx.x;
    const int64_t n4 = n >> 2;                              // whole float4s; the 0..3 floats behind them go to lanes 0..2
    const float4* p4 = reinterpret_cast<const float4*>(params);
    const bool held = n <= FQ_HELD;                         // uniform
    const int64_t tail_i = 4 * n4 + tid;
    const bool has_tail = tail_i < n;
    float4 v[FQ_V4];
    float tail = 0.0f;
    FqRange r = {INFINITY, -INFINITY};
    if (held) {
#pragma unroll
        for (int j = 0; j < FQ_V4; ++j) {
            const int64_t i4 = (int64_t)j * FQ_LANES + tid;
            if (i4 < n4) { v[j] = p4[i4]; fq_see(r, v[j]); }
        }
    } else {
        for (int64_t i4 = tid; i4 < n4; i4 += FQ_LANES) fq_see(r, p4[i4]);
    }
    if (has_tail) { tail = params[tail_i]; fq_see(r, tail); }
    // all 64 lanes of every wave are here
#pragma unroll
    for (int d = LINR_WAVE / 2; d >= 1; d >>= 1) {
        r.mn = linr_fq_min(r.mn, __shfl_xor(r.mn, d, LINR_WAVE));
        r.mx = linr_fq_max(r.mx, __shfl_xor(r.mx, d, LINR_WAVE));
    }
    if ((tid & (LINR_WAVE - 1)) == 0) { s_mn[tid / LINR_WAVE] = r.mn; s_mx[tid / LINR_WAVE] = r.mx; }
    __syncthreads();
    r.mn = s_mn[0]; r.mx = s_mx[0];
#pragma unroll
    for (int w = 1; w < FQ_LANES / LINR_WAVE; ++w) { r.mn = linr_fq_min(r.mn, s_mn[w]); r.mx = linr_fq_max(r.mx, s_mx[w]); }
    const float minv = r.mn;
    const float range = r.mx - r.mn;                        // ten_range = max_n - min_n, one fp32 rounding
    if (tid == 0 && minmax) { minmax[0] = r.mn; minmax[1] = r.mx; }
    float4* q4 = reinterpret_cast<float4*>(qparams);
    ushort4* c4 = reinterpret_cast<ushort4*>(codes);
    if (held) {
#pragma unroll
        for (int j = 0; j < FQ_V4; ++j) {
            const int64_t i4 = (int64_t)j * FQ_LANES + tid;
            if (i4 < n4) fq_put(v[j], i4, sym_max, range, minv, q4, c4);
        }
    } else {
        // every element is read and written by the same lane in both passes
        for (int64_t i4 = tid; i4 < n4; i4 += FQ_LANES) fq_put(p4[i4], i4, sym_max, range, minv, q4, c4);
    }
    if (has_tail) {
        uint16_t c;
        qparams[tail_i] = linr_fq_element(tail, sym_max, range, minv, c);
        if (codes) codes[tail_i] = c;
    }
}

}  // namespace

int linr_fake_quant_check(const float* params, int64_t n, int32_t bitdepth, const float* qparams, const uint16_t* codes) {
    if (n < 0 || bitdepth < 2 || bitdepth > 16) return LINR_EINVAL;
    if (n == 0) return 0;
    if (!params || !qparams) return LINR_EINVAL;
    if (!linr_aligned16(params) || !linr_aligned16(qparams) || (((uintptr_t)codes) & 7u)) return LINR_EALIGN;
    return 0;
}

int linr_fake_quant_launch(const float* params, int64_t n, int32_t bitdepth, float* qparams, uint16_t* codes, float* minmax,
                           hipStream_t s) {
    if (n == 0) return 0;
    fake_quant_k<<<1, FQ_LANES, 0, s>>>(params, n, (float)((1 << bitdepth) - 1), qparams, codes, minmax);
    return linr_launch_rc();
}

extern "C" int linr_params_fake_quant(const float* params, int64_t n, int32_t bitdepth, float* qparams, uint16_t* codes, float* minmax,
                                      void* stream) {
    int rc = linr_fake_quant_check(params, n, bitdepth, qparams, codes);
    if (rc) return rc;
    ProfScope ps((hipStream_t)stream, PK_MISC, 0);
    return linr_fake_quant_launch(params, n, bitdepth, qparams, codes, minmax, (hipStream_t)stream);
}

extern "C" int linr_params_fake_quant_host(const float* params, int64_t n, int32_t bitdepth, float* qparams, uint16_t* codes,
                                           float* minmax) {
    if (n < 0 || bitdepth < 2 || bitdepth > 16) return LINR_EINVAL;
    if (n == 0) return 0;
    if (!params || !qparams) return LINR_EINVAL;
    const float sym_max = (float)((1 << bitdepth) - 1);
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t i = 0; i < n; ++i) { mn = linr_fq_min(mn, params[i]); mx = linr_fq_max(mx, params[i]); }
    const float range = mx - mn;
    if (minmax) { minmax[0] = mn; minmax[1] = mx; }
    for (int64_t i = 0; i < n; ++i) {
        uint16_t c;
        qparams[i] = linr_fq_element(params[i], sym_max, range, mn, c);
        if (codes) codes[i] = c;
    }
    return 0;
}
