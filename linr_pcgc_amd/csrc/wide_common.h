// What the two cores of the wide 3x3x3 convolutions share (csrc/wide.hip: fp32 products on v_mfma_f32_4x4x1; csrc/wide_mul.hip: bf16
// products on v_mfma_f32_4x4x4_16b_bf16): the launch arguments, the row epilogue (residual, LINR_ACCUM, masks, ReLU and the pointwise
// side paths EPI 1..4, all fp32 on the unrounded values) and the launch geometry.  Not part of the C-ABI.
#pragma once
#include "common.h"
#include "conv_common.h"

#ifndef LINR_CONV_BLOCK
#define LINR_CONV_BLOCK 256
#endif
#define WC_MAXB 4
struct WcArgs {
    const float* in[WC_MAXB];      // gathered blocks (fwd: the input, bwd: the output gradient), each with its zero row at [-8, 0)
    const float* res[2];           // per produced block or nullptr
    const float* act[2];           // LINR_RELU_MASK: mask by act > 0
    float* out[2];                 // produced blocks
    const float* W;                // [27][cin][cout] (ME layout)
    const float* bias;             // fwd: [cout] or nullptr
    int cin, cout;                 // of the convolution (fwd: gathered = cin, produced = cout; bwd: the other way round)
    int gvalid;                    // gathered channels that exist (first convolutions of the outter blocks: cin = k < 8)
    int pb0;                       // first produced block of this launch
    unsigned flags;
    // pointwise side path of a wide Inception layer fused into the epilogue (models/resnet.py:55-60; template parameter EPI):
    //   EPI 1 (fwd conv0_0 C -> h): out2 = relu(own input row @ W10 + b10)                         (conv1_0 reads the centre tap's row)
    //   EPI 2 (fwd conv1_1 h -> h): out2 = (this kernel's output row) @ W12 + b12 + aux            (conv1_2 + the residual's upper half)
    //   EPI 3 (bwd tail conv):      out2 = ((produced upper half) @ W12^T) * (aux > 0)             (backward of conv1_2 and of M's ReLU)
    //   EPI 4 (bwd conv0_0):        produced += (aux own row) @ W10^T, in front of the mask        (backward-data of conv1_0; aux = gH1)
    // pw_W: [cin_pw][cout_pw] (ME layout), pw_b [cout_pw] or nullptr; pw_on: this launch runs the side path (EPI 3: the launch that
    // produces the upper half, whose first local block is pw_hi0)
    const float* pw_W; const float* pw_b;
    const float* pw_aux[2];
    float* pw_out[2];
    int pw_on, pw_hi0;
};

// rows (cin_pw) and columns (cout_pw) of the side path's weight matrix
template <int GB, int PB, int EPI> struct WcPw {
    static constexpr int PWI = EPI == 1 ? 8 * GB : EPI == 2 ? 8 * PB : EPI == 3 ? 4 * GB : EPI == 4 ? 16 * GB : 0;
    static constexpr int PWO = EPI == 1 ? 8 * PB : EPI == 2 ? 8 * PB : EPI == 3 ? 4 * GB : EPI == 4 ? 8 * GB : 0;
};

// the side path's weights (and bias, EPI 1 / 2) into LDS at wp, in front of the workgroup's barrier
template <int GB, int PB, int EPI>
__device__ __forceinline__ void wc_pw_stage(const WcArgs& a, float* wp) {
    constexpr int PWI = WcPw<GB, PB, EPI>::PWI, PWO = WcPw<GB, PB, EPI>::PWO;
    if constexpr (EPI != 0) {
        for (int e = threadIdx.x; e < PWI * PWO; e += LINR_CONV_BLOCK) wp[e] = a.pw_W[e];
        if (EPI <= 2) for (int e = threadIdx.x; e < PWO; e += LINR_CONV_BLOCK) wp[PWI * PWO + e] = a.pw_b ? a.pw_b[e] : 0.0f;
    }
}

// One live row behind the taps: acc = bias + the convolution's sum in fp32, 4 produced channels per accumulator.  wq: the side path's
// weights in LDS (wc_pw_stage), through a pointer that is per-lane in form.
template <int GB, int PB, int EPI>
__device__ __forceinline__ void wc_epilogue(const WcArgs& a, const f32x4 (&acc)[2 * PB], int64_t row, const float* wq) {
    constexpr int PWI = WcPw<GB, PB, EPI>::PWI, PWO = WcPw<GB, PB, EPI>::PWO;
    // epilogue order of the 8-wide kernels: + res, + old (LINR_ACCUM), [EPI 4: + the pointwise backward], * (act > 0)
    // (LINR_RELU_MASK), ReLU
    float o[PB][8];
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int j = 0; j < 4; ++j) o[pb][4 * h + j] = acc[2 * pb + h][j];
        if (a.res[pb]) {
            const float* r = a.res[pb] + row * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[pb][j] += r[j];
        }
        if (a.flags & LINR_ACCUM) {
            const float* op = a.out[pb] + row * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[pb][j] += op[j];
        }
    }
    if constexpr (EPI == 4) {
        // + gH1[row] @ W10^T: per produced channel ci the chain of linr_linear_wide's backward-data pass (gradient channels
        // ascending from 0), added to what the convolution, the residual's share and the old content gave
        float gh[8 * GB];
#pragma unroll
        for (int b = 0; b < GB; ++b) {
            const float4 t0 = *reinterpret_cast<const float4*>(a.pw_aux[b] + row * 8), t1 = *reinterpret_cast<const float4*>(a.pw_aux[b] + row * 8 + 4);
            gh[8 * b] = t0.x; gh[8 * b + 1] = t0.y; gh[8 * b + 2] = t0.z; gh[8 * b + 3] = t0.w;
            gh[8 * b + 4] = t1.x; gh[8 * b + 5] = t1.y; gh[8 * b + 6] = t1.z; gh[8 * b + 7] = t1.w;
        }
#pragma unroll
        for (int pb = 0; pb < PB; ++pb)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float* wrow = wq + (8 * (a.pb0 + pb) + j) * PWO;
                float t = 0.0f;
#pragma unroll
                for (int co = 0; co < PWO; ++co) t = fmaf(gh[co], wrow[co], t);
                o[pb][j] = t + o[pb][j];
            }
    }
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) {
        if (a.flags & LINR_RELU_MASK) {
            const float* m = a.act[pb] + row * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[pb][j] = m[j] > 0.0f ? o[pb][j] : 0.0f;
        }
        if (a.flags & LINR_RELU) {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[pb][j] = fmaxf(o[pb][j], 0.0f);
        }
        float* op = a.out[pb] + row * 8;
        *reinterpret_cast<float4*>(op) = make_float4(o[pb][0], o[pb][1], o[pb][2], o[pb][3]);
        *reinterpret_cast<float4*>(op + 4) = make_float4(o[pb][4], o[pb][5], o[pb][6], o[pb][7]);
    }
    if constexpr (EPI == 1) {
        // conv1_0 on the row itself: bias, then the input channels ascending (linr_linear_wide's chain), ReLU
        float xin[8 * GB];
#pragma unroll
        for (int b = 0; b < GB; ++b) {
            const float4 t0 = *reinterpret_cast<const float4*>(a.in[b] + row * 8), t1 = *reinterpret_cast<const float4*>(a.in[b] + row * 8 + 4);
            xin[8 * b] = t0.x; xin[8 * b + 1] = t0.y; xin[8 * b + 2] = t0.z; xin[8 * b + 3] = t0.w;
            xin[8 * b + 4] = t1.x; xin[8 * b + 5] = t1.y; xin[8 * b + 6] = t1.z; xin[8 * b + 7] = t1.w;
        }
        float y[PWO];
#pragma unroll
        for (int j = 0; j < PWO; ++j) y[j] = wq[PWI * PWO + j];
#pragma unroll
        for (int i = 0; i < PWI; ++i)
#pragma unroll
            for (int j = 0; j < PWO; ++j) y[j] = fmaf(xin[i], wq[i * PWO + j], y[j]);
#pragma unroll
        for (int b = 0; b < PB; ++b) {
            float* q = a.pw_out[b] + row * 8;
            *reinterpret_cast<float4*>(q) = make_float4(fmaxf(y[8 * b], 0.f), fmaxf(y[8 * b + 1], 0.f), fmaxf(y[8 * b + 2], 0.f), fmaxf(y[8 * b + 3], 0.f));
            *reinterpret_cast<float4*>(q + 4) = make_float4(fmaxf(y[8 * b + 4], 0.f), fmaxf(y[8 * b + 5], 0.f), fmaxf(y[8 * b + 6], 0.f), fmaxf(y[8 * b + 7], 0.f));
        }
    }
    if constexpr (EPI == 2) {
        // conv1_2 on this kernel's own output row M, + the residual's upper half
        float y[PWO];
#pragma unroll
        for (int j = 0; j < PWO; ++j) y[j] = wq[PWI * PWO + j];
#pragma unroll
        for (int i = 0; i < PWI; ++i)
#pragma unroll
            for (int j = 0; j < PWO; ++j) y[j] = fmaf(o[i / 8][i % 8], wq[i * PWO + j], y[j]);
#pragma unroll
        for (int b = 0; b < PB; ++b) {
            const float* r = a.pw_aux[b] + row * 8;
            float* q = a.pw_out[b] + row * 8;
            *reinterpret_cast<float4*>(q) = make_float4(y[8 * b] + r[0], y[8 * b + 1] + r[1], y[8 * b + 2] + r[2], y[8 * b + 3] + r[3]);
            *reinterpret_cast<float4*>(q + 4) = make_float4(y[8 * b + 4] + r[4], y[8 * b + 5] + r[5], y[8 * b + 6] + r[6], y[8 * b + 7] + r[7]);
        }
    }
    if constexpr (EPI == 3) {
        // gM = (gI[upper half] @ W12^T) * (M > 0): per channel ci of M the gradient channels ascending (the backward-data chain)
        if (a.pw_on) {          // uniform
            constexpr int NHB = PWI / 8;                         // blocks of the upper half = of M
            constexpr int HI0 = GB == 2 ? 1 : 0;                 // its first local block: C = 16: the launch makes blocks 0, 1; C = 32: 2, 3
#pragma unroll
            for (int b = 0; b < NHB; ++b) {
                const float* mrow = a.pw_aux[b] + row * 8;
                float g[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float* wrow = wq + (8 * b + j) * PWO;
                    float t = 0.0f;
#pragma unroll
                    for (int co = 0; co < PWO; ++co) t = fmaf(o[HI0 + co / 8][co % 8], wrow[co], t);
                    g[j] = mrow[j] > 0.0f ? t : 0.0f;
                }
                float* q = a.pw_out[b] + row * 8;
                *reinterpret_cast<float4*>(q) = make_float4(g[0], g[1], g[2], g[3]);
                *reinterpret_cast<float4*>(q + 4) = make_float4(g[4], g[5], g[6], g[7]);
            }
        }
    }
}

// the weight image is built once per workgroup, which then loops over row tiles (two workgroups per CU as in occ_conv7_k)
static inline int64_t wc_grid(int64_t n) {
    static const int cus = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1) v = 256;
        return v;
    }();
    const int64_t tiles = linr_grid(n, LINR_CONV_BLOCK);
    const int64_t want = (int64_t)cus * 2;
    const int64_t per = (tiles + want - 1) / want;
    return (tiles + per - 1) / per;
}

// ---- weight gradient: one workgroup row of the slab per (persistent block, input block) ------------------------------------------------
#define WW_PAIR 1736          // slab elements of a pair: [27][8][8] kernel block + 8 bias sums
#define WW_WAVES 4
#define WW_TAPS 28                    // 27 taps + the dump slot of the 7th gather's unused lane group
struct WwArgs {
    const float* in[WC_MAXB];         // the groups' input blocks (zero row at [-8, 0))
    const float* g[WC_MAXB][WC_MAXB]; // per group: the gradient blocks [n][8] (one convolution: the same for every group)
    int cw[WC_MAXB];                  // live channels of a group's input block
    int64_t slab_off[WC_MAXB];        // per group: where its NGB pairs start in a slab row (one convolution: bi * nbo * WW_PAIR)
    float* slab; int64_t block_stride;
};

// The end of a weight-gradient workgroup: acc[b][c][h][j] of lane (tap k, quad q) = gW[k][4 q + c][4 h + j] of gradient block b, bsum =
// the lane's partial column sum of its gradient element.  Folds the waves in order and writes the group's slab row.
template <int NGB>
__device__ __forceinline__ void ww_fold(const f32x4 (&acc)[NGB][4][2], const float (&bsum)[NGB], float* sacc, float (*sbias)[WW_WAVES][8],
                                        const WwArgs& a, int bi, int wave, int lane) {
    constexpr int NA = 32;                                  // accumulator floats per lane and gradient block
    // bias sums: lane l holds the partial column sum of channel gc over rows gu, gu + 8, ...: the 8 row phases by a fixed xor tree
#pragma unroll
    for (int b = 0; b < NGB; ++b) {
        float t = bsum[b];
#pragma unroll
        for (int m = 8; m < 64; m <<= 1) t += __shfl_xor(t, m, 64);
        if (lane < 8) sbias[b][wave][lane] = t;
    }
    const int cinv = a.cw[bi];
    const int per_k = cinv * 8, total = 27 * per_k;
    float* dst0 = a.slab + (int64_t)blockIdx.x * a.block_stride + a.slab_off[bi];
    static_for<NGB>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        __syncthreads();                       // the images (b = 0) or the previous block's fold are done with
        {
            float* mine = sacc + (wave * 64 + lane) * (NA + 1);
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int i = 0; i < 4; ++i) mine[(c * 2 + h) * 4 + i] = acc[b][c][h][i];
        }
        __syncthreads();
        float* dst = dst0 + (int64_t)b * WW_PAIR;
        const int tid = threadIdx.x;
        if (tid < 8) {
            float t = sbias[b][0][tid];
            for (int w = 1; w < WW_WAVES; ++w) t += sbias[b][w][tid];
            dst[1728 + tid] = t;
        }
        for (int e = tid; e < total; e += WW_WAVES * 64) {
            const int kq = e / per_k, r = e - kq * per_k;
            const int ci = r >> 3, co = r & 7;
            const int idx = (2 * kq + (ci >> 2)) * (NA + 1) + ((ci & 3) * 2 + (co >> 2)) * 4 + (co & 3);
            constexpr int W = 64 * (NA + 1);
            float t = sacc[idx];
#pragma unroll
            for (int w = 1; w < WW_WAVES; ++w) t += sacc[w * W + idx];
            dst[e] = t;
        }
    });
}

// the bf16-product cores (csrc/wide_mul.hip; flags & LINR_MUL_BF16): the dispatch of wconv_k / the launch of wwgrad_k with the same
// arguments and grids
int linr_wide_mul_conv(int bwd, int gb, int pb, int epi, const WcArgs& a, const int32_t* lo, const uint32_t* mask, int64_t ld, int64_t n,
                       hipStream_t s);
int linr_wide_mul_wgrad(int ngb, int nblk, int ngroups, const WwArgs& a, const int32_t* tile8t, int64_t n, hipStream_t s);
