// The model codec's weight quantiser on the device: qparams = dequant(quant_uniform2(params)) (model_compression/model_size_est.py:
// 72-91, encoder.py:101-103), bit for bit what the CPU codec computes in fp32 (csrc/fake_quant.h holds the arithmetic).  The
// quantisation-aware train steps (linr_net_train_step, linr_net_train_step_bf16 with linr_step_args.qparams) evaluate the network at its output.
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

// ---- candidate ranges (linr_params_fake_quant_ranges) ---------------------------------------------------------------------------
// The encoder's range search quantises ONE parameter vector under K candidate ranges (lo, hi) in one launch: workgroup k clamps the
// parameters into candidate k's range and quantises them with it, into row k of [K][stride] outputs.  The ranges are given, so
// nothing stands between reading a parameter and quantising it; what needs the whole row is mu = rint(sum_q / n), which stands in
// front of sum |q - mu| - the second pass.  Up to FQ_HELD floats it runs out of registers: every lane keeps the CODES of its share
// (two registers per float4, so params is read once); a larger vector is read and quantised a second time in the same stride loop.
// All sums are integers: exact, whatever the order.
struct FqBounds { float lo[LINR_FQ_MAX_RANGES], hi[LINR_FQ_MAX_RANGES]; };      // by value: 128 bytes of kernel argument

struct FqCount { unsigned long long below, above, sum_q; };     // per lane

__device__ __forceinline__ float fq_clamped(float p, float lo, float hi, float sym_max, float range, uint16_t& c, FqCount& s) {
    s.below += p < lo;
    s.above += p > hi;
    const float o = linr_fq_element(linr_fq_clamp(p, lo, hi), sym_max, range, lo, c);
    s.sum_q += c;
    return o;
}

// -> the four codes, packed: what the second pass needs of a float4
__device__ __forceinline__ uint2 fq_put_clamped(const float4& v, int64_t i4, float lo, float hi, float sym_max, float range,
                                                float4* __restrict__ q4, ushort4* __restrict__ c4, FqCount& s) {
    uint16_t cx, cy, cz, cw;
    float4 o;
    o.x = fq_clamped(v.x, lo, hi, sym_max, range, cx, s);
    o.y = fq_clamped(v.y, lo, hi, sym_max, range, cy, s);
    o.z = fq_clamped(v.z, lo, hi, sym_max, range, cz, s);
    o.w = fq_clamped(v.w, lo, hi, sym_max, range, cw, s);
    q4[i4] = o;
    if (c4) c4[i4] = make_ushort4(cx, cy, cz, cw);
    return make_uint2((uint32_t)cx | ((uint32_t)cy << 16), (uint32_t)cz | ((uint32_t)cw << 16));
}

// |q - mu| (mu is an integer in [0, sym_max]): of a code, of four packed ones, of a parameter that is quantised once more
__device__ __forceinline__ uint32_t fq_dev(uint32_t c, int32_t mu) {
    const int32_t d = (int32_t)c - mu;
    return (uint32_t)(d < 0 ? -d : d);
}
__device__ __forceinline__ uint32_t fq_dev(const uint2& c, int32_t mu) {
    return fq_dev(c.x & 0xFFFFu, mu) + fq_dev(c.x >> 16, mu) + fq_dev(c.y & 0xFFFFu, mu) + fq_dev(c.y >> 16, mu);
}
__device__ __forceinline__ uint32_t fq_dev(float p, float lo, float hi, float sym_max, float range, int32_t mu) {
    uint16_t c;
    linr_fq_element(linr_fq_clamp(p, lo, hi), sym_max, range, lo, c);
    return fq_dev((uint32_t)c, mu);
}
__device__ __forceinline__ uint32_t fq_dev(const float4& v, float lo, float hi, float sym_max, float range, int32_t mu) {
    return fq_dev(v.x, lo, hi, sym_max, range, mu) + fq_dev(v.y, lo, hi, sym_max, range, mu) + fq_dev(v.z, lo, hi, sym_max, range, mu) +
           fq_dev(v.w, lo, hi, sym_max, range, mu);
}

// the sum of x over the workgroup, in every lane; slots: FQ_LANES / LINR_WAVE words of LDS that nothing else uses
__device__ __forceinline__ unsigned long long fq_block_sum(unsigned long long x, unsigned long long* slots) {
#pragma unroll
    for (int d = LINR_WAVE / 2; d >= 1; d >>= 1) x += __shfl_xor(x, d, LINR_WAVE);
    if ((threadIdx.x & (LINR_WAVE - 1)) == 0) slots[threadIdx.x / LINR_WAVE] = x;
    __syncthreads();
    x = slots[0];
#pragma unroll
    for (int w = 1; w < FQ_LANES / LINR_WAVE; ++w) x += slots[w];
    return x;
}

// grid = K, workgroup k = candidate k.  params 16-byte aligned; qparams 16-byte, codes 8-byte aligned (or NULL) with stride % 4 == 0, so
// that every row is; stats: int64 [K][4] or NULL; n >= 1
__global__ __launch_bounds__(FQ_LANES) void fake_quant_ranges_k(const float* params, int64_t n, float sym_max, FqBounds bounds, int64_t stride,
                                                                float* qparams, uint16_t* codes, long long* __restrict__ stats) {
    __shared__ unsigned long long s_sum[4][FQ_LANES / LINR_WAVE];
    const int tid = threadIdx.x;
    const int k = blockIdx.x;
    const float lo = bounds.lo[k], hi = bounds.hi[k];
    const float range = hi - lo;                            // one fp32 rounding, as ten_range
    const int64_t n4 = n >> 2;
    const float4* p4 = reinterpret_cast<const float4*>(params);
    float4* q4 = reinterpret_cast<float4*>(qparams + k * stride);
    ushort4* c4 = codes ? reinterpret_cast<ushort4*>(codes + k * stride) : nullptr;
    const bool held = n <= FQ_HELD;                         // uniform
    const int64_t tail_i = 4 * n4 + tid;
    const bool has_tail = tail_i < n;
    uint2 c[FQ_V4];                                         // the codes of this lane's float4s: half the registers of the parameters
    uint32_t tail_c = 0;
    FqCount s = {0, 0, 0};
    if (held) {
#pragma unroll
        for (int j = 0; j < FQ_V4; ++j) {
            const int64_t i4 = (int64_t)j * FQ_LANES + tid;
            if (i4 < n4) c[j] = fq_put_clamped(p4[i4], i4, lo, hi, sym_max, range, q4, c4, s);
        }
    } else {
        for (int64_t i4 = tid; i4 < n4; i4 += FQ_LANES) fq_put_clamped(p4[i4], i4, lo, hi, sym_max, range, q4, c4, s);
    }
    if (has_tail) {
        uint16_t ct;
        qparams[k * stride + tail_i] = fq_clamped(params[tail_i], lo, hi, sym_max, range, ct, s);
        if (codes) codes[k * stride + tail_i] = ct;
        tail_c = ct;
    }
    if (!stats) return;                                     // uniform
    // all 64 lanes of every wave are here
    const unsigned long long below = fq_block_sum(s.below, s_sum[0]);
    const unsigned long long above = fq_block_sum(s.above, s_sum[1]);
    const unsigned long long sum_q = fq_block_sum(s.sum_q, s_sum[2]);
    const int32_t mu = (int32_t)linr_fq_mean_level(sum_q, n);
    unsigned long long dev = 0;
    if (held) {
#pragma unroll
        for (int j = 0; j < FQ_V4; ++j) {
            const int64_t i4 = (int64_t)j * FQ_LANES + tid;
            if (i4 < n4) dev += fq_dev(c[j], mu);
        }
    } else {
        // every element is read by the lane that read it in the first pass
        for (int64_t i4 = tid; i4 < n4; i4 += FQ_LANES) dev += fq_dev(p4[i4], lo, hi, sym_max, range, mu);
    }
    if (has_tail) dev += fq_dev(tail_c, mu);
    dev = fq_block_sum(dev, s_sum[3]);
    if (tid < 4) stats[4 * k + tid] = (long long)(tid == 0 ? below : tid == 1 ? above : tid == 2 ? sum_q : dev);
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

// Everything the entry and its host twin refuse alike (pointers and alignment apart).  0: go on; 1: n == 0, nothing to do.
static int fq_ranges_check(int64_t n, int32_t bitdepth, const float* ranges_h, int32_t K, int64_t stride) {
    if (n < 0 || bitdepth < 2 || bitdepth > 16) return LINR_EINVAL;
    if (K < 1 || K > LINR_FQ_MAX_RANGES || !ranges_h) return LINR_EINVAL;
    if (stride < n || (stride & 3)) return LINR_EINVAL;
    for (int k = 0; k < K; ++k)
        if (!(ranges_h[2 * k] <= ranges_h[2 * k + 1])) return LINR_EINVAL;          // lo > hi, or a NaN bound
    return n == 0 ? 1 : 0;
}

extern "C" int linr_params_fake_quant_ranges(const float* params, int64_t n, int32_t bitdepth, const float* ranges_h, int32_t K,
                                             int64_t stride, float* qparams, uint16_t* codes, int64_t* stats, void* stream) {
    int rc = fq_ranges_check(n, bitdepth, ranges_h, K, stride);
    if (rc) return rc < 0 ? rc : 0;
    rc = linr_fake_quant_check(params, n, bitdepth, qparams, codes);
    if (rc) return rc;
    if (((uintptr_t)stats) & 7u) return LINR_EALIGN;
    FqBounds b;
    for (int k = 0; k < LINR_FQ_MAX_RANGES; ++k) {
        b.lo[k] = ranges_h[2 * (k < K ? k : 0)];
        b.hi[k] = ranges_h[2 * (k < K ? k : 0) + 1];
    }
    ProfScope ps((hipStream_t)stream, PK_MISC, 0);
    fake_quant_ranges_k<<<K, FQ_LANES, 0, (hipStream_t)stream>>>(params, n, (float)((1 << bitdepth) - 1), b, stride, qparams, codes,
                                                                 reinterpret_cast<long long*>(stats));
    return linr_launch_rc();
}

extern "C" int linr_params_fake_quant_ranges_host(const float* params, int64_t n, int32_t bitdepth, const float* ranges_h, int32_t K,
                                                  int64_t stride, float* qparams, uint16_t* codes, int64_t* stats) {
    int rc = fq_ranges_check(n, bitdepth, ranges_h, K, stride);
    if (rc) return rc < 0 ? rc : 0;
    if (!params || !qparams) return LINR_EINVAL;
    const float sym_max = (float)((1 << bitdepth) - 1);
    for (int k = 0; k < K; ++k) {
        const float lo = ranges_h[2 * k], hi = ranges_h[2 * k + 1];
        const float range = hi - lo;
        float* q = qparams + k * stride;
        uint16_t* c = codes ? codes + k * stride : nullptr;
        int64_t below = 0, above = 0, sum_q = 0, dev = 0;
        for (int64_t i = 0; i < n; ++i) {
            uint16_t code;
            below += params[i] < lo;
            above += params[i] > hi;
            q[i] = linr_fq_element(linr_fq_clamp(params[i], lo, hi), sym_max, range, lo, code);
            if (c) c[i] = code;
            sum_q += code;
        }
        if (!stats) continue;
        const int64_t mu = linr_fq_mean_level((unsigned long long)sum_q, n);
        for (int64_t i = 0; i < n; ++i) {
            uint16_t code;
            linr_fq_element(linr_fq_clamp(params[i], lo, hi), sym_max, range, lo, code);
            dev += code > mu ? code - mu : mu - code;
        }
        stats[4 * k] = below; stats[4 * k + 1] = above; stats[4 * k + 2] = sum_q; stats[4 * k + 3] = dev;
    }
    return 0;
}
