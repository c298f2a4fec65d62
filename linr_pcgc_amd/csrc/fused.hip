// Forward and backward-data convolutions and the occupancy heads on the COMPRESSED kernel map (csrc/net.hip is the caller; the map is
// built by linr_kmap_compress, csrc/kmap.hip; the stand-alone weight gradients are in csrc/wgrad.hip).
//
// Compressed kernel map: the coordinate list is sorted x-major, so the up-to-three dz = -1,0,+1 neighbours of one
// (dx,dy) column are consecutive rows.  Per row: lo[q] = row of the first present neighbour of column q = (dx+1)+3(dy+1)
// (9 x int32) + a 27-bit presence mask = 40 B instead of 27 x int32 = 108 B.  The 36 MB table of a loot-like frame
// becomes 13.5 MB, i.e. one XCD's share (1.7 MB) stays L2-resident across the ~140 conv passes of a training step.
#include "common.h"
#include "conv_common.h"
#include "bwd_tail.h"
#include "head_bwd.h"

// ---- plain conv3 forward / backward-data on the compressed map, on the matrix cores --------------------------------------
// `in` must have the zero pad row at index -1.
//   BWD == false: acc[o] += x[i] * W[(k*GIN + i)*GOUT + o]
//   BWD == true : acc[o] += x[i] * W[(k*GOUT + o)*GIN + i]   (gathered rows come from the mirrored offset)
// v_mfma_f32_4x4x1_16b_f32 is 16 independent 4x4 outer products (K = 1); with CBSZ = 4 the A operand of block ABID is
// broadcast to all 16 blocks, so ONE instruction computes, for all 64 lanes at once,
//        acc[row(lane)][4*ABID + i] += W[ci][4*ABID + i] * x[row(lane)][ci]        i = 0..3
// i.e. 64 rows x 4 output channels x 1 input channel = 256 FMAs with NO padding (the 16-wide MFMA shapes waste half
// of their N dimension at Cout = 8).  The lane keeps the thread-per-row layout of spconv_gather_k (csrc/spconv.hip): B = the lane's
// gathered feature x[ci], D = the lane's 4 accumulators, A = the weight row held by lanes 0..GOUT-1 (read from an LDS
// copy of the whole [27][Cin][Cout] kernel).  K = 1 makes every instruction a single-rounding fmaf(x, w, acc), issued
// in the same order as spconv_gather_k (taps in LINR_TAP order, ci ascending) => bit-identical results, at the MFMA rate
// (measured 91-119 TFLOP/s for this stream vs 52-71 TFLOP/s for v_pk_fma_f32; tools/mfma_probe.hip, valu_probe.hip).
// Measured dead ends for this kernel (kept out of the tree): hand-pinned software pipelines
// (2-3 offsets ahead, or a whole dz-plane of gathers in flight) and wave-cooperative staging of each (dx,dy) column's
// contiguous neighbour range through LDS were all slower than the compiler's own interleaving below.
// occupancy head fused behind the prune convolution (models/upsample.py:153-160 + models/model_core.py:76-81):
// z = w2 . relu(W1 c + b1) + b2, p = sigmoid(z), bits partial of the block.  EPI == 1 selects it.
struct HeadArgs {
    const float* w1;      // [24][8]  inner_mlps.k.0.0.weight
    const float* b1;      // [24]
    const float* w2;      // [24]     inner_mlps.k.0.2.weight
    const float* b2;      // [1]
    const float* target;  // occupancy column (stride target_ld) or nullptr (decoder: probabilities only)
    int target_ld;
    float* p_out;         // [n]
    double* partial;      // [gridDim.x] block partial sums of nats, or nullptr
};

#ifndef LINR_CONV_BLOCK
#define LINR_CONV_BLOCK 256
#endif
template <int GIN, int GOUT, bool BWD, int LOADW, int EPI = 0>
__global__ __launch_bounds__(LINR_CONV_BLOCK) void cconv_mfma_k(const float* __restrict__ in, int in_ld,
                                                           const int32_t* __restrict__ lo, const uint32_t* __restrict__ mask,
                                                           int64_t ld, int64_t n, const float* __restrict__ W,
                                                           const float* __restrict__ bias, const float* __restrict__ res,
                                                           int res_ld, const float* __restrict__ act, int act_ld,
                                                           float* __restrict__ out, int out_ld, unsigned flags,
                                                           HeadArgs hd = HeadArgs(), PwArgs pw = PwArgs(), Grp gp = Grp()) {
    static_assert(GOUT == 4 || GOUT == 8, "output channels must fill 1 or 2 MFMA blocks");
    {   // group offsets (all zero for a plain launch)
        const int gi = blockIdx.y;
        in += gp.in[gi]; W += gp.w[gi]; out += gp.out[gi];
        if (bias) bias += gp.b[gi];
        if (res) res += gp.res[gi];
        if (act) act += gp.act[gi];
        if constexpr (EPI == 1) {
            hd.w1 += gp.e0[gi]; hd.b1 += gp.e1[gi]; hd.w2 += gp.e2[gi]; hd.b2 += gp.e3[gi];
            if (hd.target) hd.target += gp.e4[gi];
            hd.p_out += gp.e5[gi];
            if (hd.partial) hd.partial += gp.e6[gi];
        }
        if constexpr (EPI == 2) { pw.w += gp.e0[gi]; pw.b += gp.e1[gi]; }
        if constexpr (EPI == 3) { pw.w += gp.e0[gi]; pw.aux += gp.e1[gi]; pw.aux_out += gp.e2[gi]; }
        if constexpr (EPI == 4) { pw.w += gp.e0[gi]; pw.aux += gp.e1[gi]; }
    }
    // All weights of the convolution live in registers for the whole kernel: the A operand of the 16-block MFMA is taken
    // from block ABID (an immediate), so ONE VGPR carries 16 different weight 4-vectors - block b of register wv[g][i]
    // holds W(k = g*KPV + b/HB, input i, outputs 4*(b%HB) .. +3).  27 x Cin x Cout floats = at most 32 VGPRs, loaded once;
    // the loop below has no weight traffic at all (an LDS copy + 4 ds_reads and waits per offset cost ~8 us per launch).
    constexpr int HB = GOUT / 4;                 // output halves (MFMA blocks) per offset
    constexpr int KPV = 16 / HB;                 // offsets packed per register
    constexpr int NG = (27 + KPV - 1) / KPV;
    const int lane = threadIdx.x & 63;
    float wv[NG][GIN];
    {
        const int blk = lane >> 2, j = lane & 3;
        const int kl = blk / HB, co = 4 * (blk % HB) + j;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int k = g * KPV + kl;
#pragma unroll
            for (int i = 0; i < GIN; ++i)
                wv[g][i] = (k < 27) ? (BWD ? W[(k * GOUT + co) * GIN + i] : W[(k * GIN + i) * GOUT + co]) : 0.0f;
        }
    }
    const int64_t row_raw = (int64_t)blockIdx.x * LINR_CONV_BLOCK + threadIdx.x;
    const bool live = row_raw < n;
    const int64_t row = live ? row_raw : n - 1;          // every lane stays in the MFMAs (they ignore EXEC)
    const char* pad = reinterpret_cast<const char*>(in - in_ld);
    const uint32_t rowbytes = (uint32_t)in_ld * 4u;
    uint32_t off[27];
    decode_offsets<BWD>(lo, mask, ld, row, rowbytes, off);
    f32x4 acc[GOUT / 4];
#pragma unroll
    for (int h = 0; h < GOUT / 4; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[h][j] = (bias != nullptr) ? bias[4 * h + j] : 0.0f;
    constexpr int PF = 4;
    float x[PF + 1][LOADW];
    // Left to itself hipcc waits (vmcnt(0)) right after every 16-byte gather - 54 serial round trips per wave.  The loop
    // is therefore pipelined by hand: the load of offset k+PF is issued before the MFMAs of offset k and sched_barrier
    // keeps it there, so the compiler's own counted waits leave PF rows in flight.
#pragma unroll
    for (int u = 0; u < PF; ++u) RowLoadF<LOADW>::run(pad + off[LINR_TAP(u)], x[u]);
    __builtin_amdgcn_sched_barrier(0);
    static_for<27>([&](auto kc) {
        constexpr int kk = decltype(kc)::value;          // step; k = the tap it handles (common.h: LINR_TAP)
        constexpr int k = LINR_TAP(kk);
        constexpr int g = k / KPV, ab = (k % KPV) * HB;
        if constexpr (kk + PF < 27) RowLoadF<LOADW>::run(pad + off[LINR_TAP(kk + PF)], x[(kk + PF) % (PF + 1)]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < GIN; ++i) {
            acc[0] = __builtin_amdgcn_mfma_f32_4x4x1f32(wv[g][i], x[kk % (PF + 1)][i], acc[0], 4, ab, 0);
            if constexpr (GOUT == 8)
                acc[1] = __builtin_amdgcn_mfma_f32_4x4x1f32(wv[g][i], x[kk % (PF + 1)][i], acc[1], 4, ab + 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    });
    float a[GOUT];
#pragma unroll
    for (int h = 0; h < GOUT / 4; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) a[4 * h + j] = acc[h][j];
    if constexpr (EPI == 1) {
        // ---- fused occupancy head: the conv output row a[0..8) is C_k --------------------------------------------
        float* op = out + row * out_ld;
        if (live) {
            *reinterpret_cast<float4*>(op) = make_float4(a[0], a[1], a[2], a[3]);
            *reinterpret_cast<float4*>(op + 4) = make_float4(a[4], a[5], a[6], a[7]);
        }
        float z = hd.b2[0];
#pragma unroll
        for (int j = 0; j < 24; ++j) {
            float hj = hd.b1[j];
#pragma unroll
            for (int i = 0; i < 8; ++i) hj = fmaf(a[i], hd.w1[j * 8 + i], hj);
            z = fmaf(fmaxf(hj, 0.0f), hd.w2[j], z);
        }
        const float p = 1.0f / (1.0f + expf(-z));
        if (live) hd.p_out[row] = p;
        if (hd.partial != nullptr) {          // wave-uniform (kernel argument)
            __shared__ double sred[LINR_CONV_BLOCK / 64];
            double nats = 0.0;
            if (live) {
                const float t = hd.target[row * hd.target_ld];
                nats = (double)((t - 1.0f) * fmaxf(logf(1.0f - p), -100.0f) - t * fmaxf(logf(p), -100.0f));
            }
            // fixed shuffle tree inside the wave, then the waves in order => bit-reproducible
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) nats += __shfl_xor(nats, d, 64);
            if (lane == 0) sred[threadIdx.x >> 6] = nats;
            __syncthreads();
            if (threadIdx.x == 0) {
                double tot = sred[0];
                for (int w = 1; w < LINR_CONV_BLOCK / 64; ++w) tot += sred[w];
                hd.partial[blockIdx.x] = tot;
            }
        }
        return;
    } else {
    if (!live) return;
    // epilogue order: + res, + old (ACCUM), [+ own-row pointwise term], * mask, ReLU
    if (res != nullptr) {
        const float* r = res + row * res_ld;
#pragma unroll
        for (int o = 0; o < GOUT; ++o) a[o] += r[o];
    }
    float* op = out + row * out_ld;
    if (flags & LINR_ACCUM) {
#pragma unroll
        for (int o = 0; o < GOUT; ++o) a[o] += op[o];
    }
    if constexpr (EPI == 4) {          // gA += gH[row][4:8] @ W10^T     (W10 [8][4]: gin[i] = sum_o g[o] * W10[i][o])
        const float4 g4 = *reinterpret_cast<const float4*>(pw.aux + row * 8 + 4);
        const float g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float t = 0.0f;
#pragma unroll
            for (int o = 0; o < 4; ++o) t = fmaf(g[o], pw.w[i * 4 + o], t);
            a[i] += t;
        }
    }
    if constexpr (EPI == 3) {          // store gI, then gM = (gI[4:8] @ W12^T) * (M > 0)   (W12 [4][4])
        const float4 m4 = *reinterpret_cast<const float4*>(pw.aux + row * 4);
        const float mv[4] = {m4.x, m4.y, m4.z, m4.w};
        float gm[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float t = 0.0f;
#pragma unroll
            for (int o = 0; o < 4; ++o) t = fmaf(a[4 + o], pw.w[i * 4 + o], t);
            gm[i] = mv[i] > 0.0f ? t : 0.0f;
        }
        *reinterpret_cast<float4*>(pw.aux_out + row * 4) = make_float4(gm[0], gm[1], gm[2], gm[3]);
    }
    if constexpr (EPI == 2) {          // conv0_0 half: ReLU, store; conv1_0 half: relu(in[row] @ W10 + b10)
        const char* self = reinterpret_cast<const char*>(in) + (uint32_t)row * ((uint32_t)in_ld * 4u);
        float xc[8];
        RowLoadF<8>::run(self, xc);
        float h1[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) h1[o] = pw.b[o];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int o = 0; o < 4; ++o) h1[o] = fmaf(xc[i], pw.w[i * 4 + o], h1[o]);
        *reinterpret_cast<float4*>(op) = make_float4(fmaxf(a[0], 0.0f), fmaxf(a[1], 0.0f), fmaxf(a[2], 0.0f), fmaxf(a[3], 0.0f));
        *reinterpret_cast<float4*>(op + 4) = make_float4(fmaxf(h1[0], 0.0f), fmaxf(h1[1], 0.0f), fmaxf(h1[2], 0.0f), fmaxf(h1[3], 0.0f));
        return;
    }
    if (flags & LINR_RELU_MASK) {
        const float* m = act + row * act_ld;
#pragma unroll
        for (int o = 0; o < GOUT; ++o) a[o] = m[o] > 0.0f ? a[o] : 0.0f;
    }
    if (flags & LINR_RELU) {
#pragma unroll
        for (int o = 0; o < GOUT; ++o) a[o] = fmaxf(a[o], 0.0f);
    }
    if (out_ld % 4 == 0) {
#pragma unroll
        for (int v = 0; v < GOUT / 4; ++v)
            *reinterpret_cast<float4*>(op + 4 * v) = make_float4(a[4 * v], a[4 * v + 1], a[4 * v + 2], a[4 * v + 3]);
    } else {
#pragma unroll
        for (int o = 0; o < GOUT; ++o) op[o] = a[o];
    }
    }
}

extern "C" int linr_spconv_cmap(int32_t bwd, const float* in, int32_t in_ld, const int32_t* lo, const uint32_t* mask, int64_t ld,
                                int64_t n, const float* W, const float* bias, int32_t cin, int32_t cout, const float* res,
                                int32_t res_ld, const float* act, int32_t act_ld, float* out, int32_t out_ld, uint32_t flags,
                                void* stream) {
    if (n < 0 || ld < n || (in_ld != 4 && in_ld != 8)) return LINR_EINVAL;
    if (n == 0) return 0;
    if (!in || !lo || !mask || !W || !out) return LINR_EINVAL;
    if (!linr_aligned16(in) || !linr_aligned16(out)) return LINR_EALIGN;
    const int gin = bwd ? cout : cin, gout = bwd ? cin : cout;
    if (in_ld < gin || out_ld < gout || (gout != 4 && gout != 8)) return LINR_EINVAL;
    if ((flags & LINR_RELU_MASK) && (!act || act_ld < gout)) return LINR_EINVAL;
    if (res && res_ld < gout) return LINR_EINVAL;
    if (!linr_rows_fit32(n, 4 * in_ld)) return LINR_EINVAL;
    const ConvGroup g = {in, W, bias, res, act, out};
    return linr_cconv_launch(bwd != 0, {lo, mask, ld, n}, &g, 1, in_ld, cin, cout, res_ld, act_ld, out_ld, flags, (hipStream_t)stream);
}

// prune conv 8->8 + head of stage k in one launch; partial: [linr_grid(n,256)] doubles or nullptr
int linr_cconv_head_launch(LinrCmap m, const HeadFwdGroup* g, int ng, int target_ld, hipStream_t s) {
    if (ng < 1 || ng > LINR_MAXG) return LINR_EINVAL;
    if (m.n == 0) return 0;
    Grp gp = Grp();
    for (int i = 0; i < ng; ++i) {
        gp.in[i] = g[i].in - g[0].in; gp.w[i] = g[i].W - g[0].W; gp.b[i] = g[i].bias - g[0].bias; gp.out[i] = g[i].c_out - g[0].c_out;
        gp.e0[i] = g[i].w1 - g[0].w1; gp.e1[i] = g[i].b1 - g[0].b1; gp.e2[i] = g[i].w2 - g[0].w2; gp.e3[i] = g[i].b2 - g[0].b2;
        gp.e4[i] = g[i].target - g[0].target; gp.e5[i] = g[i].p_out - g[0].p_out; gp.e6[i] = g[i].partial - g[0].partial;
    }
    HeadArgs hd = {g[0].w1, g[0].b1, g[0].w2, g[0].b2, g[0].target, target_ld, g[0].p_out, g[0].partial};
    cconv_mfma_k<8, 8, false, 8, 1><<<dim3(linr_grid(m.n, LINR_CONV_BLOCK), ng), LINR_CONV_BLOCK, 0, s>>>(
        g[0].in, 8, m.lo, m.mask, m.ld, m.n, g[0].W, g[0].bias, nullptr, 0, nullptr, 0, g[0].c_out, 8, 0, hd, PwArgs(), gp);
    return linr_launch_rc();
}

// ---- the two 4->4 convolutions of the Inception block as ONE pass --------------------------------------------------------
// forward (models/resnet.py:56-57): in = H [n][8];  I[:,0:4] = conv(H[:,0:4]; W01) + b01 + A[:,0:4]
//                                   M = relu(conv(H[:,4:8]; W11) + b11);  I[:,4:8] = M @ W12 + b12 + A[:,4:8]
// backward: gH = [bwd(gI[:,0:4]; W01) | bwd(gM; W11)] * (H > 0), gathered at the mirrored offsets from two matrices.
// One 32-byte (or 2 x 16-byte) gather per neighbour serves both convolutions; lanes 0-3 hold W01's tap, lanes 4-7 W11's.
struct DualArgs {
    const float* in2; int in2_ld;      // bwd: second gathered matrix (gM, ld 4); fwd: unused
    const float* w01; const float* w11;
    const float* b01; const float* b11;
    const float* a_res;                // fwd: A [n][8] (residual)
    const float* w12; const float* b12;
    float* m_out;                      // fwd: M [n][4]
    const float* act;                  // bwd: H [n][8] for the ReLU mask
};

template <bool BWD>
__global__ __launch_bounds__(LINR_BLOCK) void cconv_dual44_k(const float* __restrict__ in, int in_ld,
                                                             const int32_t* __restrict__ lo, const uint32_t* __restrict__ mask,
                                                             int64_t ld, int64_t n, DualArgs d, float* __restrict__ out,
                                                             Grp gp = Grp()) {
    {   // group offsets: in, e0 = in2, w = w01, e1 = w11, b = b01, e2 = b11, res = a_res, e3 = w12, e4 = b12, e5 = m_out, act, out
        const int gi = blockIdx.y;
        in += gp.in[gi]; out += gp.out[gi];
        if (d.in2) d.in2 += gp.e0[gi];
        d.w01 += gp.w[gi]; d.w11 += gp.e1[gi];
        if (d.b01) d.b01 += gp.b[gi];
        if (d.b11) d.b11 += gp.e2[gi];
        if (d.a_res) d.a_res += gp.res[gi];
        if (d.w12) d.w12 += gp.e3[gi];
        if (d.b12) d.b12 += gp.e4[gi];
        if (d.m_out) d.m_out += gp.e5[gi];
        if (d.act) d.act += gp.act[gi];
    }
    // register-resident weights (see cconv_mfma_k): block b of wv[g][i] holds, for offset k = g*8 + b/2, the tap of
    // W01 (b even) or W11 (b odd) for input i and outputs 0..3
    const int lane = threadIdx.x & 63;
    float wv[4][4];
    {
        const int blk = lane >> 2, j = lane & 3;
        const int kl = blk >> 1;
        const float* Wsel = (blk & 1) ? d.w11 : d.w01;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int k = g * 8 + kl;
#pragma unroll
            for (int i = 0; i < 4; ++i) wv[g][i] = (k < 27) ? (BWD ? Wsel[(k * 4 + j) * 4 + i] : Wsel[(k * 4 + i) * 4 + j]) : 0.0f;
        }
    }
    const int64_t row_raw = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    const bool live = row_raw < n;
    const int64_t row = live ? row_raw : n - 1;
    uint32_t off[27];
    decode_offsets<BWD>(lo, mask, ld, row, 1u, off);                  // row index + 1 (0 = pad row); scaled per matrix below
    const char* pad0 = reinterpret_cast<const char*>(in - in_ld);
    // row pitches are 16 or 32 bytes: scale by wave-uniform shifts (v_mul_lo_u32 is quarter rate)
    const uint32_t rb0 = __builtin_amdgcn_readfirstlane(in_ld == 8 ? 5u : 4u);
    const char* pad1 = BWD ? reinterpret_cast<const char*>(d.in2 - d.in2_ld) : pad0 + 16;     // fwd: second half of the same row
    const uint32_t rb1 = BWD ? __builtin_amdgcn_readfirstlane(d.in2_ld == 8 ? 5u : 4u) : rb0;
    f32x4 acc0, acc1;
#pragma unroll
    for (int j = 0; j < 4; ++j) { acc0[j] = BWD ? 0.0f : d.b01[j]; acc1[j] = BWD ? 0.0f : d.b11[j]; }
    constexpr int PF = 3;                             // gathers run PF offsets ahead of the MFMAs (see cconv_mfma_k)
    float x0[PF + 1][4], x1[PF + 1][4];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        RowLoadF<4>::run(pad0 + (off[LINR_TAP(u)] << rb0), x0[u]);
        RowLoadF<4>::run(pad1 + (off[LINR_TAP(u)] << rb1), x1[u]);
    }
    __builtin_amdgcn_sched_barrier(0);
    static_for<27>([&](auto kc) {
        constexpr int kk = decltype(kc)::value;           // step; k = weight tap (decode_offsets already mirrored `off` for BWD)
        constexpr int k = LINR_TAP(kk);
        constexpr int g = k / 8, ab = (k % 8) * 2;
        if constexpr (kk + PF < 27) {
            RowLoadF<4>::run(pad0 + (off[LINR_TAP(kk + PF)] << rb0), x0[(kk + PF) % (PF + 1)]);
            RowLoadF<4>::run(pad1 + (off[LINR_TAP(kk + PF)] << rb1), x1[(kk + PF) % (PF + 1)]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(wv[g][i], x0[kk % (PF + 1)][i], acc0, 4, ab, 0);
            acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(wv[g][i], x1[kk % (PF + 1)][i], acc1, 4, ab + 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    });
    if (!live) return;
    float* op = out + row * 8;
    if (BWD) {
        const float4 h0 = *reinterpret_cast<const float4*>(d.act + row * 8);
        const float4 h1 = *reinterpret_cast<const float4*>(d.act + row * 8 + 4);
        *reinterpret_cast<float4*>(op) = make_float4(h0.x > 0.0f ? acc0[0] : 0.0f, h0.y > 0.0f ? acc0[1] : 0.0f,
                                                     h0.z > 0.0f ? acc0[2] : 0.0f, h0.w > 0.0f ? acc0[3] : 0.0f);
        *reinterpret_cast<float4*>(op + 4) = make_float4(h1.x > 0.0f ? acc1[0] : 0.0f, h1.y > 0.0f ? acc1[1] : 0.0f,
                                                         h1.z > 0.0f ? acc1[2] : 0.0f, h1.w > 0.0f ? acc1[3] : 0.0f);
    } else {
        const float4 a0 = *reinterpret_cast<const float4*>(d.a_res + row * 8);
        const float4 a1 = *reinterpret_cast<const float4*>(d.a_res + row * 8 + 4);
        const float m[4] = {fmaxf(acc1[0], 0.0f), fmaxf(acc1[1], 0.0f), fmaxf(acc1[2], 0.0f), fmaxf(acc1[3], 0.0f)};
        *reinterpret_cast<float4*>(d.m_out + row * 4) = make_float4(m[0], m[1], m[2], m[3]);
        float i1[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) i1[o] = d.b12[o];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int o = 0; o < 4; ++o) i1[o] = fmaf(m[i], d.w12[i * 4 + o], i1[o]);
        *reinterpret_cast<float4*>(op) = make_float4(acc0[0] + a0.x, acc0[1] + a0.y, acc0[2] + a0.z, acc0[3] + a0.w);
        *reinterpret_cast<float4*>(op + 4) = make_float4(i1[0] + a1.x, i1[1] + a1.y, i1[2] + a1.z, i1[3] + a1.w);
    }
}

int linr_dual44_fwd_launch(LinrCmap m, const Dual44FwdGroup* g, int ng, hipStream_t s) {
    if (ng < 1 || ng > LINR_MAXG) return LINR_EINVAL;
    if (m.n == 0) return 0;
    Grp gp = Grp();
    for (int i = 0; i < ng; ++i) {
        gp.in[i] = g[i].H - g[0].H; gp.w[i] = g[i].w01 - g[0].w01; gp.b[i] = g[i].b01 - g[0].b01; gp.e1[i] = g[i].w11 - g[0].w11;
        gp.e2[i] = g[i].b11 - g[0].b11; gp.res[i] = g[i].A - g[0].A; gp.e3[i] = g[i].w12 - g[0].w12; gp.e4[i] = g[i].b12 - g[0].b12;
        gp.e5[i] = g[i].M - g[0].M; gp.out[i] = g[i].I - g[0].I;
    }
    DualArgs d = {nullptr, 0, g[0].w01, g[0].w11, g[0].b01, g[0].b11, g[0].A, g[0].w12, g[0].b12, g[0].M, nullptr};
    cconv_dual44_k<false><<<dim3(linr_grid(m.n, LINR_BLOCK), ng), LINR_BLOCK, 0, s>>>(g[0].H, 8, m.lo, m.mask, m.ld, m.n, d, g[0].I, gp);
    return linr_launch_rc();
}

int linr_dual44_bwd_launch(LinrCmap m, const Dual44BwdGroup* g, int ng, hipStream_t s) {
    if (ng < 1 || ng > LINR_MAXG) return LINR_EINVAL;
    if (m.n == 0) return 0;
    Grp gp = Grp();
    for (int i = 0; i < ng; ++i) {
        gp.in[i] = g[i].gI - g[0].gI; gp.e0[i] = g[i].gM - g[0].gM; gp.w[i] = g[i].w01 - g[0].w01; gp.e1[i] = g[i].w11 - g[0].w11;
        gp.act[i] = g[i].H - g[0].H; gp.out[i] = g[i].gH - g[0].gH;
    }
    DualArgs d = {g[0].gM, 4, g[0].w01, g[0].w11, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, g[0].H};
    cconv_dual44_k<true><<<dim3(linr_grid(m.n, LINR_BLOCK), ng), LINR_BLOCK, 0, s>>>(g[0].gI, 8, m.lo, m.mask, m.ld, m.n, d, g[0].gH, gp);
    return linr_launch_rc();
}

// conv0_0 (8->4) + conv1_0 (1x1 8->4) forward with both ReLUs: H = [relu(conv3(A)) | relu(A @ W10 + b10)]
int linr_conv_pw_fwd_launch(LinrCmap m, const ConvPwGroup* g, int ng, hipStream_t s) {
    if (ng < 1 || ng > LINR_MAXG) return LINR_EINVAL;
    if (m.n == 0) return 0;
    Grp gp = Grp();
    for (int i = 0; i < ng; ++i) {
        gp.in[i] = g[i].A - g[0].A; gp.w[i] = g[i].w00 - g[0].w00; gp.b[i] = g[i].b00 - g[0].b00; gp.out[i] = g[i].H - g[0].H;
        gp.e0[i] = g[i].w10 - g[0].w10; gp.e1[i] = g[i].b10 - g[0].b10;
    }
    PwArgs pw = {g[0].w10, g[0].b10, nullptr, nullptr};
    cconv_mfma_k<8, 4, false, 8, 2><<<dim3(linr_grid(m.n, LINR_CONV_BLOCK), ng), LINR_CONV_BLOCK, 0, s>>>(
        g[0].A, 8, m.lo, m.mask, m.ld, m.n, g[0].w00, g[0].b00, nullptr, 0, nullptr, 0, g[0].H, 8, 0, HeadArgs(), pw, gp);
    return linr_launch_rc();
}

// backward of the block's tail conv: gI = bwd(gO; Wb) and gM = (gI[:,4:8] @ W12^T) * (M > 0)   (Conv88BwdGroup: g = gO, out = gI)
int linr_conv_bwd_gm_launch(LinrCmap m, const Conv88BwdGroup* g, int ng, hipStream_t s) {
    if (ng < 1 || ng > LINR_MAXG) return LINR_EINVAL;
    if (m.n == 0) return 0;
    Grp gp = Grp();
    for (int i = 0; i < ng; ++i) {
        gp.in[i] = g[i].g - g[0].g; gp.w[i] = g[i].W - g[0].W; gp.out[i] = g[i].out - g[0].out;
        gp.e0[i] = g[i].w12 - g[0].w12; gp.e1[i] = g[i].M - g[0].M; gp.e2[i] = g[i].gM - g[0].gM;
    }
    PwArgs pw = {g[0].w12, nullptr, g[0].M, g[0].gM};
    cconv_mfma_k<8, 8, true, 8, 3><<<dim3(linr_grid(m.n, LINR_CONV_BLOCK), ng), LINR_CONV_BLOCK, 0, s>>>(
        g[0].g, 8, m.lo, m.mask, m.ld, m.n, g[0].W, nullptr, nullptr, 0, nullptr, 0, g[0].out, 8, 0, HeadArgs(), pw, gp);
    return linr_launch_rc();
}

// gA = (bwd(gH[:,0:4]; W00) + gI (+ old gA: LINR_ACCUM) + gH[:,4:8] @ W10^T) (* (A > 0): LINR_RELU_MASK)
int linr_conv_bwd_ga_launch(LinrCmap m, const Conv84BwdGroup* g, int ng, unsigned flags, hipStream_t s) {
    if (ng < 1 || ng > LINR_MAXG) return LINR_EINVAL;
    if (m.n == 0) return 0;
    if ((flags & LINR_RELU_MASK) && !g[0].A) return LINR_EINVAL;
    Grp gp = Grp();
    for (int i = 0; i < ng; ++i) {
        gp.in[i] = g[i].gH - g[0].gH; gp.w[i] = g[i].w00 - g[0].w00; gp.res[i] = g[i].gI - g[0].gI; gp.act[i] = g[i].A - g[0].A;
        gp.out[i] = g[i].gA - g[0].gA; gp.e0[i] = g[i].w10 - g[0].w10; gp.e1[i] = g[i].gH - g[0].gH;
    }
    PwArgs pw = {g[0].w10, nullptr, g[0].gH, nullptr};
    cconv_mfma_k<4, 8, true, 4, 4><<<dim3(linr_grid(m.n, LINR_CONV_BLOCK), ng), LINR_CONV_BLOCK, 0, s>>>(
        g[0].gH, 8, m.lo, m.mask, m.ld, m.n, g[0].w00, nullptr, g[0].gI, 8, g[0].A, 8, g[0].gA, 8, flags & (LINR_RELU_MASK | LINR_ACCUM),
        HeadArgs(), pw, gp);
    return linr_launch_rc();
}

// ---- first convolutions of the 7 outter blocks: one gather, 56 outputs -----------------------------------------------------
// Block b (1..7) starts with conv3(occ[:, :b] -> 8) + ReLU on the SAME occupancy rows (models/upsample.py:206-214), so the
// grouped forward gathers each neighbour's 8 occupancy floats once and feeds all 7 kernels: per offset 28 (block, input
// channel) pairs x 2 output quads = 56 MFMA blocks instead of 7 x 16 with zero-extended kernels, and 1/7 of the gathers.
// The weights sit in LDS as the A-operand image wl[k][v][lane]: block (lane >> 2) of register v is combo 16 v + block,
// combo c <-> pair p = c / 2 (block g = tri^-1(p), channel ci = p - g (g + 1) / 2), quad h = c % 2.  Per output the chain is
// bias, then taps in LINR_TAP order, ci ascending fmaf - the chain of cconv_mfma_k on that block alone, so the decoder's
// block-by-block forward gives the same bits.
struct Occ7Args { int64_t w[7], b[7], out[7]; };       // parameter offsets (kernel, bias) and output element offsets per block

__host__ __device__ constexpr int occ7_g(int p) { return p < 1 ? 0 : p < 3 ? 1 : p < 6 ? 2 : p < 10 ? 3 : p < 15 ? 4 : p < 21 ? 5 : 6; }

__global__ __launch_bounds__(LINR_CONV_BLOCK) void occ_conv7_k(const float* __restrict__ occ, const int32_t* __restrict__ lo,
                                                               const uint32_t* __restrict__ mask, int64_t ld, int64_t n,
                                                               const float* __restrict__ P, Occ7Args a,
                                                               float* __restrict__ out) {
    __shared__ float wl[27 * 4 * 64];
    {   // the weight image: a thread's 27 loads all in flight, then the LDS stores (as a rolled loop every element waited for two
        // dependent loads - the block's parameter offset out of the argument struct, then the weight: 54 round trips to the L2 in
        // front of the first tile).  Element e = threadIdx.x + 256 i: the combo (e & 255) >> 2 and j = e & 3 do not depend on i.
        const int c = (int)(threadIdx.x >> 2), j = (int)(threadIdx.x & 3);
        const int pr = c >> 1, h = c & 1, g = occ7_g(pr), ci = pr - g * (g + 1) / 2;
        int64_t wg = a.w[0];
#pragma unroll
        for (int q = 1; q < 7; ++q) wg = (g == q) ? a.w[q] : wg;          // constant indices: scalar loads + selects
        const float* src = P + wg + ci * 8 + 4 * h + j;
        const int kstride = (g + 1) * 8;
        float wv[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) wv[k] = c < 56 ? src[k * kstride] : 0.0f;
#pragma unroll
        for (int k = 0; k < 27; ++k) wl[k * 256 + threadIdx.x] = wv[k];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const char* pad = reinterpret_cast<const char*>(occ - 8);
    // the 27 KB weight image is built once per workgroup: the launch gives every workgroup several row tiles (linr_occ_conv7_launch)
    const int64_t tiles = (n + LINR_CONV_BLOCK - 1) / LINR_CONV_BLOCK;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row_raw = tile * LINR_CONV_BLOCK + threadIdx.x;
    const bool live = row_raw < n;
    const int64_t row = live ? row_raw : n - 1;          // every lane stays in the MFMAs (they ignore EXEC)
    uint32_t off[27];
    decode_offsets<false>(lo, mask, ld, row, 32u, off);
    f32x4 acc[7][2];
#pragma unroll
    for (int g = 0; g < 7; ++g)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[g][h][j] = P[a.b[g] + 4 * h + j];
    constexpr int PF = 3;
    float x[PF + 1][8];
    float wr[2][4];
#pragma unroll
    for (int u = 0; u < PF; ++u) RowLoadF<8>::run(pad + off[LINR_TAP(u)], x[u]);
#pragma unroll
    for (int v = 0; v < 4; ++v) wr[0][v] = wl[(LINR_TAP(0) * 4 + v) * 64 + lane];
    __builtin_amdgcn_sched_barrier(0);
    static_for<27>([&](auto kc) {
        constexpr int kk = decltype(kc)::value;            // step; tap LINR_TAP(kk)
        if constexpr (kk + PF < 27) RowLoadF<8>::run(pad + off[LINR_TAP(kk + PF)], x[(kk + PF) % (PF + 1)]);
        if constexpr (kk + 1 < 27) {
#pragma unroll
            for (int v = 0; v < 4; ++v) wr[(kk + 1) & 1][v] = wl[(LINR_TAP(kk + 1) * 4 + v) * 64 + lane];
        }
        __builtin_amdgcn_sched_barrier(0);
        // input channel outermost: consecutive MFMAs write different accumulators (no back-to-back dependent issue), and
        // every output still sees its channels in ascending order
        static_for<7>([&](auto cic) {
            constexpr int ci = decltype(cic)::value;
            static_for<7 - ci>([&](auto gc) {
                constexpr int g = ci + decltype(gc)::value;
                static_for<2>([&](auto hc) {
                    constexpr int h = decltype(hc)::value;
                    constexpr int c = 2 * (g * (g + 1) / 2 + ci) + h;
                    acc[g][h] = __builtin_amdgcn_mfma_f32_4x4x1f32(wr[kk & 1][c / 16], x[kk % (PF + 1)][ci], acc[g][h], 4, c % 16, 0);
                });
            });
        });
        __builtin_amdgcn_sched_barrier(0);
    });
    if (live) {
#pragma unroll
        for (int g = 0; g < 7; ++g) {
            float* op = out + a.out[g] + row * 8;
            *reinterpret_cast<float4*>(op) = make_float4(fmaxf(acc[g][0][0], 0.0f), fmaxf(acc[g][0][1], 0.0f),
                                                         fmaxf(acc[g][0][2], 0.0f), fmaxf(acc[g][0][3], 0.0f));
            *reinterpret_cast<float4*>(op + 4) = make_float4(fmaxf(acc[g][1][0], 0.0f), fmaxf(acc[g][1][1], 0.0f),
                                                             fmaxf(acc[g][1][2], 0.0f), fmaxf(acc[g][1][3], 0.0f));
        }
    }
    }
}

// occ: arena copy of the occupancy [n][8] with the zero pad row in front; w_off / b_off: parameter offsets of the 7 first
// convolutions (kernel [27][b][8] of block b) ; out + out_off[g]: A matrix of block g + 1
int linr_occ_conv7_launch(const float* occ, LinrCmap m, const float* P, const int64_t* w_off, const int64_t* b_off, float* out,
                          const int64_t* out_off, hipStream_t s) {
    const int64_t n = m.n;
    if (n == 0) return 0;
    Occ7Args a;
    for (int g = 0; g < 7; ++g) { a.w[g] = w_off[g]; a.b[g] = b_off[g]; a.out[g] = out_off[g]; }
    // MFMA-bound (1512 per 64 rows): two workgroups per CU keep the matrix cores fed, and each amortises its weight image over
    // tiles / grid row tiles (same-box A/B at 337 k rows, ms/step: one tile per workgroup 1.732, three workgroups per CU 1.725,
    // two 1.716, one 1.720)
    constexpr int per_cu = 2;
    static const int cus = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1) v = 256;
        return v;
    }();
    const int64_t tiles = linr_grid(n, LINR_CONV_BLOCK);
    const int64_t want = (int64_t)cus * per_cu;
    const int64_t per = (tiles + want - 1) / want;                 // tiles per workgroup
    const int64_t grid = (tiles + per - 1) / per;
    occ_conv7_k<<<(unsigned)grid, LINR_CONV_BLOCK, 0, s>>>(occ, m.lo, m.mask, m.ld, n, P, a, out);
    return linr_launch_rc();
}

// ---- fused backward of the occupancy head ------------------------------------------------------------------------------
// csrc/head_bwd.h holds the arithmetic (shared with the bf16 training executor); here: fp32 rows in and out, grouped launches.
struct HeadBwdArgs {
    const float* c;  const float* p;  const float* target; int target_ld;
    const float* w1; const float* b1; const float* w2;
    float gscale;                     // d loss / d nats
    float* gc;                        // [n][8]
    float* big; int64_t block_stride; int64_t off_w1, off_b1, off_w2, off_b2;
    int active;
};

__global__ __launch_bounds__(HB_WAVES * 64, 2) void head_bwd_k(HeadBwdArgs A, int64_t n, Grp gp = Grp()) {
    __shared__ float lds[HB_LDS_FLOATS];
    // group offsets: in = c, e0 = p, e1 = target, w = w1, b = b1, e2 = w2, out = gc, e3..e6 = slab offsets of w1, b1, w2, b2
    const int gi = blockIdx.y;
    const float* C = A.c + gp.in[gi];
    float* GC = A.gc + gp.out[gi];
    HbParams h;
    h.p = A.p + gp.e0[gi]; h.target = A.target + gp.e1[gi]; h.target_ld = A.target_ld;
    h.w1 = A.w1 + gp.w[gi]; h.b1 = A.b1 + gp.b[gi]; h.w2 = A.w2 + gp.e2[gi];
    h.gscale = A.gscale; h.n = n;
    h.dst = A.big + (int64_t)blockIdx.x * A.block_stride;
    h.off_w1 = A.off_w1 + gp.e3[gi]; h.off_b1 = A.off_b1 + gp.e4[gi]; h.off_w2 = A.off_w2 + gp.e5[gi]; h.off_b2 = A.off_b2 + gp.e6[gi];
    h.active = A.active;
    head_bwd_body<HbRaw32>(h,
        [&](int64_t row) { return HbRaw32{*reinterpret_cast<const f32x4*>(C + row * 8), *reinterpret_cast<const f32x4*>(C + row * 8 + 4)}; },
        [](const HbRaw32& r, float (&c)[8]) {
            c[0] = r.a[0]; c[1] = r.a[1]; c[2] = r.a[2]; c[3] = r.a[3]; c[4] = r.b[0]; c[5] = r.b[1]; c[6] = r.b[2]; c[7] = r.b[3];
        },
        [&](int64_t row, const float (&g)[8]) {
            *reinterpret_cast<float4*>(GC + row * 8) = make_float4(g[0], g[1], g[2], g[3]);
            *reinterpret_cast<float4*>(GC + row * 8 + 4) = make_float4(g[4], g[5], g[6], g[7]);
        }, lds);
}

static int hb_cus() {
    static const int v = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
        return n;
    }();
    return v;
}

// rows_written == nullptr: slab rows 0 .. nblocks - 1 are all written (rows beyond the active blocks get zeros); otherwise only the
// active blocks' rows are written and *rows_written tells the caller how many (its reduction must stop there)
int linr_head_bwd_launch(const HeadBwdGroup* g, int ng, int target_ld, float gscale, int64_t n, float* big, int64_t block_stride,
                         int nblocks, int* rows_written, hipStream_t s) {
    if (rows_written) *rows_written = 0;
    if (ng < 1 || ng > LINR_MAXG) return LINR_EINVAL;
    if (n == 0) return 0;
    Grp gp = Grp();
    for (int i = 0; i < ng; ++i) {
        gp.in[i] = g[i].c - g[0].c; gp.e0[i] = g[i].p - g[0].p; gp.e1[i] = g[i].target - g[0].target; gp.w[i] = g[i].w1 - g[0].w1;
        gp.b[i] = g[i].b1 - g[0].b1; gp.e2[i] = g[i].w2 - g[0].w2; gp.out[i] = g[i].gc - g[0].gc;
        gp.e3[i] = g[i].w1_off - g[0].w1_off; gp.e4[i] = g[i].b1_off - g[0].b1_off; gp.e5[i] = g[i].w2_off - g[0].w2_off;
        gp.e6[i] = g[i].b2_off - g[0].b2_off;
    }
    const int active = hb_blocks(n, ng, hb_cus(), nblocks);
    HeadBwdArgs A = {g[0].c, g[0].p, g[0].target, target_ld, g[0].w1, g[0].b1, g[0].w2, gscale, g[0].gc, big, block_stride,
                     g[0].w1_off, g[0].b1_off, g[0].w2_off, g[0].b2_off, active};
    head_bwd_k<<<dim3(rows_written ? active : nblocks, ng), HB_WAVES * 64, 0, s>>>(A, n, gp);
    if (rows_written) *rows_written = active;
    return linr_launch_rc();
}

// executor entry: all matrices are arena matrices (16-byte aligned rows, ld in {4, 8}, pad row present).  The kernel writes 4 or
// 8 channels, so the backward-data of an outter block's first conv into 1..3 or 5..7 occupancy channels is refused (nothing needs it).
int linr_cconv_launch(bool bwd, LinrCmap m, const ConvGroup* g, int ng, int in_ld, int cin, int cout, int res_ld, int act_ld,
                      int out_ld, unsigned flags, hipStream_t s) {
    if (ng < 1 || ng > LINR_MAXG) return LINR_EINVAL;
    if (m.n == 0) return 0;
    Grp gp = Grp();
    for (int i = 0; i < ng; ++i) {
        gp.in[i] = g[i].in - g[0].in; gp.w[i] = g[i].W - g[0].W; gp.b[i] = g[i].bias - g[0].bias; gp.res[i] = g[i].res - g[0].res;
        gp.act[i] = g[i].act - g[0].act; gp.out[i] = g[i].out - g[0].out;
    }
    const dim3 grid(linr_grid(m.n, LINR_CONV_BLOCK), ng);
#define GO(GI, GO_, B)                                                                                                  \
    do {                                                                                                                \
        cconv_mfma_k<GI, GO_, B, ((GI + 3) / 4 * 4)><<<grid, LINR_CONV_BLOCK, 0, s>>>(                                  \
            g[0].in, in_ld, m.lo, m.mask, m.ld, m.n, g[0].W, g[0].bias, g[0].res, res_ld, g[0].act, act_ld, g[0].out, out_ld, flags, \
            HeadArgs(), PwArgs(), gp);                                                                                  \
        return linr_launch_rc();                                                                                        \
    } while (0)
#define FWD(CI, CO) if (!bwd && cin == CI && cout == CO) GO(CI, CO, false);
#define BWD(CI, CO) if (bwd && cin == CI && cout == CO) GO(CO, CI, true);
    FWD(8, 8) FWD(8, 4) FWD(4, 4) FWD(1, 8) FWD(2, 8) FWD(3, 8) FWD(4, 8) FWD(5, 8) FWD(6, 8) FWD(7, 8)
    BWD(8, 8) BWD(8, 4) BWD(4, 4) BWD(4, 8)
#undef BWD
#undef FWD
#undef GO
    return LINR_EINVAL;
}


// ---- the executor's fused layers as stand-alone ops (include/linr_hip.h) ---------------------------------------------------
static bool cmap_ok(const void* in, const int32_t* lo, const uint32_t* mask, int64_t ld, int64_t n) {
    return in && lo && mask && ld >= n;
}
#define HEAD_PARAMS 241            // inner_mlps.k.0: 0.weight [24][8], 0.bias [24], 2.weight [1][24], 2.bias [1]

extern "C" size_t linr_head_workspace_bytes(int64_t n) {
    if (n < 0) return 0;
    const size_t fwd = (size_t)linr_grid(n, LINR_CONV_BLOCK) * sizeof(double);
    const size_t bwd = (size_t)LINR_WG_BLOCKS * HEAD_PARAMS * sizeof(float);
    return (fwd > bwd ? fwd : bwd) + 64;
}

extern "C" int linr_head_fwd(const float* prior, const int32_t* lo, const uint32_t* mask, int64_t ld, int64_t n,
                             const float* Wp, const float* bp, const float* w1, const float* b1, const float* w2,
                             const float* b2, const float* target, int32_t target_ld, float* c_out, float* p_out,
                             double* bits_acc, void* ws, size_t ws_bytes, void* stream) {
    if (n < 0) return LINR_EINVAL;
    if (n == 0) return 0;
    if (!cmap_ok(prior, lo, mask, ld, n) || !Wp || !bp || !w1 || !b1 || !w2 || !b2 || !c_out || !p_out) return LINR_EINVAL;
    if (bits_acc && (!target || target_ld < 1 || !ws)) return LINR_EINVAL;
    if (!linr_aligned16(prior) || !linr_aligned16(c_out)) return LINR_EALIGN;
    if (!linr_rows_fit32(n)) return LINR_EINVAL;
    double* part = nullptr;
    if (bits_acc) {
        if (ws_bytes < linr_head_workspace_bytes(n)) return LINR_ENOSPC;
        if (((uintptr_t)ws) & 7u) return LINR_EALIGN;
        part = (double*)ws;
    }
    const HeadFwdGroup g = {prior, Wp, bp, c_out, w1, b1, w2, b2, target, p_out, part};
    int rc = linr_cconv_head_launch({lo, mask, ld, n}, &g, 1, target_ld, (hipStream_t)stream);
    if (rc) return rc;
    if (bits_acc) return linr_bits_finish_launch(part, (int)linr_grid(n, LINR_CONV_BLOCK), bits_acc, (hipStream_t)stream);
    return 0;
}

extern "C" int linr_head_bwd(const float* c, const float* p, const float* target, int32_t target_ld, const float* w1,
                             const float* b1, const float* w2, float gscale, float* gc, int64_t n, float* ghead, void* ws,
                             size_t ws_bytes, void* stream) {
    if (n < 0 || target_ld < 1) return LINR_EINVAL;
    if (!ghead) return LINR_EINVAL;
    if (n == 0) return linr_hip_rc(hipMemsetAsync(ghead, 0, HEAD_PARAMS * sizeof(float), (hipStream_t)stream));
    if (!c || !p || !target || !w1 || !b1 || !w2 || !gc || !ws) return LINR_EINVAL;
    if (ws_bytes < linr_head_workspace_bytes(n)) return LINR_ENOSPC;
    if (!linr_aligned16(c) || !linr_aligned16(gc) || !linr_aligned16(ws)) return LINR_EALIGN;
    float* slab = (float*)ws;
    // gscale multiplies BITS (like linr_bce_bits_bwd); the kernel works in nats: d bits / d nats = 1 / ln 2
    const HeadBwdGroup g = {c, p, target, w1, b1, w2, gc, 0, 192, 216, 240};
    int rc = linr_head_bwd_launch(&g, 1, target_ld, gscale * 1.4426950408889634f, n, slab, HEAD_PARAMS, LINR_WG_BLOCKS, nullptr,
                                  (hipStream_t)stream);
    if (rc) return rc;
    return linr_slab_reduce_launch(slab, LINR_WG_BLOCKS, HEAD_PARAMS, ghead, (hipStream_t)stream);
}

static bool inc_ok(const linr_inception_params* q) {
    return q && q->w00 && q->b00 && q->w01 && q->b01 && q->w10 && q->b10 && q->w11 && q->b11 && q->w12 && q->b12;
}

extern "C" int linr_inception_fwd(const float* x, const int32_t* lo, const uint32_t* mask, int64_t ld, int64_t n,
                                  const linr_inception_params* q, float* H, float* M, float* I, void* stream) {
    if (n < 0) return LINR_EINVAL;
    if (n == 0) return 0;
    if (!cmap_ok(x, lo, mask, ld, n) || !inc_ok(q) || !H || !M || !I) return LINR_EINVAL;
    if (!linr_aligned16(x) || !linr_aligned16(H) || !linr_aligned16(M) || !linr_aligned16(I)) return LINR_EALIGN;
    if (!linr_rows_fit32(n)) return LINR_EINVAL;
    const LinrCmap m = {lo, mask, ld, n};
    const ConvPwGroup g0 = {x, q->w00, q->b00, q->w10, q->b10, H};
    int rc = linr_conv_pw_fwd_launch(m, &g0, 1, (hipStream_t)stream);
    if (rc) return rc;
    const Dual44FwdGroup g1 = {H, q->w01, q->b01, q->w11, q->b11, x, q->w12, q->b12, M, I};
    return linr_dual44_fwd_launch(m, &g1, 1, (hipStream_t)stream);
}

extern "C" int linr_inception_bwd_data(const float* gI, const float* x, const float* H, const float* M, const int32_t* lo,
                                       const uint32_t* mask, int64_t ld, int64_t n, const linr_inception_params* q, float* gM,
                                       float* gH, float* gX, uint32_t flags, void* stream) {
    if (n < 0) return LINR_EINVAL;
    if (n == 0) return 0;
    if (!cmap_ok(gI, lo, mask, ld, n) || !inc_ok(q) || !H || !M || !gM || !gH || !gX) return LINR_EINVAL;
    if ((flags & LINR_RELU_MASK) && !x) return LINR_EINVAL;
    if (flags & ~(LINR_RELU_MASK | LINR_ACCUM)) return LINR_EINVAL;
    if (!linr_aligned16(gI) || !linr_aligned16(gM) || !linr_aligned16(gH) || !linr_aligned16(gX) || !linr_aligned16(H) ||
        !linr_aligned16(M)) return LINR_EALIGN;
    if (!linr_rows_fit32(n)) return LINR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    // I[:,4:8] = M @ W12 + b12 + x[:,4:8], M = relu(.)  =>  gM = (gI[:,4:8] @ W12^T) * (M > 0)
    int rc = linr_linear_launch(gI + 4, 8, n, q->w12, 1, 4, nullptr, 4, 4, nullptr, 0, M, 4, gM, 4, LINR_RELU_MASK, s);
    if (rc) return rc;
    const LinrCmap m = {lo, mask, ld, n};
    const Dual44BwdGroup g0 = {gI, gM, H, q->w01, q->w11, gH, 0, 0, 0, 0};
    rc = linr_dual44_bwd_launch(m, &g0, 1, s);
    if (rc) return rc;
    const Conv84BwdGroup g1 = {gH, x, gI, q->w00, q->w10, gX, 0, 0, 0, 0};
    return linr_conv_bwd_ga_launch(m, &g1, 1, flags, s);
}

extern "C" int linr_occ_conv7(const float* occ, const int32_t* lo, const uint32_t* mask, int64_t ld, int64_t n,
                              const float* params, const int64_t* w_off_h, const int64_t* b_off_h, float* out,
                              const int64_t* out_off_h, void* stream) {
    if (n < 0) return LINR_EINVAL;
    if (n == 0) return 0;
    if (!cmap_ok(occ, lo, mask, ld, n) || !params || !w_off_h || !b_off_h || !out || !out_off_h) return LINR_EINVAL;
    if (!linr_aligned16(occ) || !linr_aligned16(out)) return LINR_EALIGN;
    for (int g = 0; g < 7; ++g)
        if (w_off_h[g] < 0 || b_off_h[g] < 0 || (out_off_h[g] & 3)) return LINR_EINVAL;
    if (!linr_rows_fit32(n)) return LINR_EINVAL;
    return linr_occ_conv7_launch(occ, {lo, mask, ld, n}, params, w_off_h, b_off_h, out, out_off_h, (hipStream_t)stream);
}
