// bf16-PRODUCT cores of the wide 3x3x3 convolutions (flags & LINR_MUL_BF16; train_precision 'bf16-mul'): the kernels of csrc/wide.hip with
// their multiplications on bf16 matrix instructions.  Everything in memory stays fp32 - activations, gradients, weights, the slab -
// and so does everything that is not a product of the convolution: bias, residual, LINR_ACCUM, masks, ReLU, the pointwise side paths
// (wc_epilogue) and the bias gradient.  An operand is rounded to bf16 (nearest even, v_cvt_pk_bf16_f32) in registers, right at the
// multiply; products of two bf16 values are exact in fp32 and every sum is fp32:
//   forward        out = bias + sum rb(x) rb(W)          backward-data  gx = sum rb(g) rb(W) at the mirrored taps
//   weight grad    gW  = sum_rows rb(x) rb(g)            bias grad      gb = sum g (no product: unrounded)
// wmconv_k: wconv_k's organisation (lane = output row, every input block gathered once per tap as fp32, the weights of a tap as an
// A-operand image in LDS, broadcast by CBSZ / ABID) on v_mfma_f32_4x4x4_16b_bf16: one instruction takes FOUR gathered channels into four
// produced ones, a quarter of wconv_k's instructions per tap; the image holds bf16 (half the LDS).
// wmwgrad_k: wwgrad_k's organisation (group = input block, one gather of its rows for all gradient blocks, the same slab) with the rows
// as K of v_mfma_f32_4x4x4_16b_bf16: four rows per instruction.
#include "common.h"
#include "conv_common.h"
#include "bf16_common.h"
#include "wide_common.h"
#include "prof.h"

template <int GB, int PB, bool BWD, int EPI = 0>
__global__ __launch_bounds__(LINR_CONV_BLOCK) void wmconv_k(WcArgs a, const int32_t* __restrict__ lo, const uint32_t* __restrict__ mask,
                                                           int64_t ld, int64_t n) {
    constexpr int NCQ = 2 * GB, NQ = 2 * PB;                 // gathered channel quads, produced channel quads
    constexpr int NC = NCQ * NQ, NVP = (NC + 15) / 16;       // weight blocks (4 gathered x 4 produced) per tap; A-operand registers pairs
    extern __shared__ uint2 wimg[];                          // [27][NVP][64 lanes]: lane 4 blk + j of pair v = block 16 v + blk, produced j
    {   // the weight image: all of a thread's (scattered, L2-resident) loads in flight at once, then the roundings and the LDS stores
        constexpr int TOT = 27 * NVP * 64, IT = (TOT + LINR_CONV_BLOCK - 1) / LINR_CONV_BLOCK;
        float wv[IT][4];
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int e = (int)threadIdx.x + LINR_CONV_BLOCK * i;
            const int ln = e % 64, v = (e / 64) % NVP, k = e / (NVP * 64);
            const int c = 16 * v + (ln >> 2), j = ln & 3;
            const int cq = c / NQ, oq = c % NQ, po = 8 * a.pb0 + 4 * oq + j;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int gi = 4 * cq + t;
                float val = 0.0f;
                if (e < TOT && c < NC && gi < a.gvalid)
                    val = BWD ? a.W[((int64_t)k * a.cin + po) * a.cout + gi] : a.W[((int64_t)k * a.cin + gi) * a.cout + po];
                wv[i][t] = val;
            }
        }
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int e = (int)threadIdx.x + LINR_CONV_BLOCK * i;
            if (e < TOT) wimg[e] = make_uint2(pack2(wv[i][0], wv[i][1]), pack2(wv[i][2], wv[i][3]));
        }
    }
    // the side path's weights behind the image (read back with uniform addresses: LDS broadcasts)
    float* wp = reinterpret_cast<float*>(wimg + 27 * NVP * 64);
    // read through a pointer that is per-lane in form: with a uniform one the compiler keeps the weights in SGPRs and spills hundreds
    const float* wq = wp + __builtin_amdgcn_mbcnt_lo(0u, 0u);
    wc_pw_stage<GB, PB, EPI>(a, wp);
    __syncthreads();
    // the produced channels' bias: once per workgroup (uniform loads), not once per tile
    float bz[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) bz[q][j] = (!BWD && a.bias) ? a.bias[8 * a.pb0 + 4 * q + j] : 0.0f;
    const int lane = threadIdx.x & 63;
    const char* pad[GB];
#pragma unroll
    for (int g = 0; g < GB; ++g) pad[g] = reinterpret_cast<const char*>(a.in[g] - 8);
    const uint2* wlane = wimg + lane;
    const int64_t tiles = (n + LINR_CONV_BLOCK - 1) / LINR_CONV_BLOCK;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row_raw = tile * LINR_CONV_BLOCK + threadIdx.x;
        const bool live = row_raw < n;
        const int64_t row = live ? row_raw : n - 1;          // every lane stays in the MFMAs (they ignore EXEC)
        uint32_t off[27];
        decode_offsets<BWD>(lo, mask, ld, row, 32u, off);
        f32x4 acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[q][j] = bz[q][j];
        constexpr int PF = GB >= 4 ? 1 : 2;
        f32x4 x[PF + 1][NCQ];
        s16x4 wr[2][NVP];
        auto gather = [&](int u, uint32_t o) {
#pragma unroll
            for (int g = 0; g < GB; ++g) {
                x[u][2 * g] = *reinterpret_cast<const f32x4*>(pad[g] + o);
                x[u][2 * g + 1] = *reinterpret_cast<const f32x4*>(pad[g] + o + 16);
            }
        };
        auto wread = [&](int u, int k) {
#pragma unroll
            for (int v = 0; v < NVP; ++v) wr[u][v] = __builtin_bit_cast(s16x4, wlane[(k * NVP + v) * 64]);
        };
#pragma unroll
        for (int u = 0; u < PF; ++u) gather(u, off[LINR_TAP(u)]);
        wread(0, LINR_TAP(0));
        __builtin_amdgcn_sched_barrier(0);
        static_for<27>([&](auto kc) {
            constexpr int kk = decltype(kc)::value;            // step; tap LINR_TAP(kk)
            if constexpr (kk + PF < 27) gather((kk + PF) % (PF + 1), off[LINR_TAP(kk + PF)]);
            if constexpr (kk + 1 < 27) wread((kk + 1) & 1, LINR_TAP(kk + 1));
            __builtin_amdgcn_sched_barrier(0);
            // gathered quad outermost: consecutive MFMAs write different accumulators, every output sees its channels ascending
            static_for<NCQ>([&](auto gc) {
                constexpr int cq = decltype(gc)::value;
                const f32x4 xv = x[kk % (PF + 1)][cq];
                const s16x4 xb = __builtin_bit_cast(s16x4, make_uint2(pack2(xv[0], xv[1]), pack2(xv[2], xv[3])));      // rb(x) at the multiply
                static_for<NQ>([&](auto qc) {
                    constexpr int oq = decltype(qc)::value;
                    constexpr int c = cq * NQ + oq;
                    acc[oq] = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(wr[kk & 1][c / 16], xb, acc[oq], 4, c % 16, 0);
                });
            });
            __builtin_amdgcn_sched_barrier(0);
        });
        if (!live) continue;
        wc_epilogue<GB, PB, EPI>(a, acc, row, wq);
    }
}

template <int GB, int PB, bool BWD, int EPI = 0>
static int wm_launch(const WcArgs& a, const int32_t* lo, const uint32_t* mask, int64_t ld, int64_t n, hipStream_t s) {
    constexpr int PWI = WcPw<GB, PB, EPI>::PWI, PWO = WcPw<GB, PB, EPI>::PWO;
    constexpr int NVP = (4 * GB * PB + 15) / 16;
    constexpr size_t lds = (size_t)27 * NVP * 64 * 8 + ((size_t)PWI * PWO + PWO) * 4;
    wmconv_k<GB, PB, BWD, EPI><<<(unsigned)wc_grid(n), LINR_CONV_BLOCK, lds, s>>>(a, lo, mask, ld, n);
    return linr_launch_rc();
}

// the shapes of wc_dispatch (csrc/wide.hip), one for one
template <bool BWD>
static int wm_dispatch(int gb, int pb, int epi, const WcArgs& a, const int32_t* lo, const uint32_t* mask, int64_t ld, int64_t n, hipStream_t s) {
    if (epi == 0) {
        if (gb == 1 && pb == 1) return wm_launch<1, 1, BWD>(a, lo, mask, ld, n, s);
        if (gb == 1 && pb == 2) return wm_launch<1, 2, BWD>(a, lo, mask, ld, n, s);
        if (gb == 2 && pb == 1) return wm_launch<2, 1, BWD>(a, lo, mask, ld, n, s);
        if (gb == 2 && pb == 2) return wm_launch<2, 2, BWD>(a, lo, mask, ld, n, s);
        if (gb == 4 && pb == 1) return wm_launch<4, 1, BWD>(a, lo, mask, ld, n, s);
        if (gb == 4 && pb == 2) return wm_launch<4, 2, BWD>(a, lo, mask, ld, n, s);
        return LINR_EINVAL;
    }
    if constexpr (!BWD) {
        if (epi == 1 && gb == 2 && pb == 1) return wm_launch<2, 1, false, 1>(a, lo, mask, ld, n, s);
        if (epi == 1 && gb == 4 && pb == 2) return wm_launch<4, 2, false, 1>(a, lo, mask, ld, n, s);
        if (epi == 2 && gb == 1 && pb == 1) return wm_launch<1, 1, false, 2>(a, lo, mask, ld, n, s);
        if (epi == 2 && gb == 2 && pb == 2) return wm_launch<2, 2, false, 2>(a, lo, mask, ld, n, s);
    } else {
        if (epi == 3 && gb == 2 && pb == 2) return wm_launch<2, 2, true, 3>(a, lo, mask, ld, n, s);
        if (epi == 3 && gb == 4 && pb == 2) return wm_launch<4, 2, true, 3>(a, lo, mask, ld, n, s);
        if (epi == 4 && gb == 1 && pb == 2) return wm_launch<1, 2, true, 4>(a, lo, mask, ld, n, s);
        if (epi == 4 && gb == 2 && pb == 2) return wm_launch<2, 2, true, 4>(a, lo, mask, ld, n, s);
    }
    return LINR_EINVAL;
}

int linr_wide_mul_conv(int bwd, int gb, int pb, int epi, const WcArgs& a, const int32_t* lo, const uint32_t* mask, int64_t ld, int64_t n,
                       hipStream_t s) {
    return bwd ? wm_dispatch<true>(gb, pb, epi, a, lo, mask, ld, n, s) : wm_dispatch<false>(gb, pb, epi, a, lo, mask, ld, n, s);
}

// ---- weight gradient -------------------------------------------------------------------------------------------------------------------
// A wave's 8-row group: the gather lanes (tap of 4, row, quad) round their float4 to four bf16 and store it into the wave's image
// [tap][row][8 channels]; the gradient tile's lanes (row, channel) store theirs transposed, [channel][row].  The MFMA lanes (tap, quad)
// read their 8 rows x 4 channels back, regroup them to 4 channels x (rows 0..3 | rows 4..7) - the B operands, K = row - and the
// lanes 0..7 of the transposed tile are the A operands (block h = channels 4 h .. 4 h + 3): acc[b][c][h][j] += sum over 4 rows of
// g[row][4 h + j] x[tap][row][4 q + c], wwgrad_k's accumulators, so the fold and the slab are its own (ww_fold).
typedef uint4 __attribute__((may_alias)) uint4_alias;          // the transposed tile is stored as 16-bit elements and read as rows
#define WM_PITCH 144                  // bytes per tap in the bf16 image: 8 rows x 16 B + 16 B
template <int NGB>
__global__ __launch_bounds__(WW_WAVES * 64) void wmwgrad_k(WwArgs a, const int32_t* __restrict__ tile8t, int64_t n) {
    constexpr int NA = 32;                                  // accumulator floats per lane and gradient block
    constexpr int IMG_F4 = WW_TAPS * WM_PITCH / 16;
    constexpr int FOLD_F4 = 16 * (NA + 1);
    constexpr int SMEM_F4 = WW_WAVES * (IMG_F4 > FOLD_F4 ? IMG_F4 : FOLD_F4);
    __shared__ float4 smem[SMEM_F4];
    __shared__ float sbias[NGB][WW_WAVES][8];
    __shared__ uint4 sg[WW_WAVES][NGB][8];                  // per wave and gradient block: the tile as bf16 [channel][row]
    float* sacc = reinterpret_cast<float*>(smem);
    const int bi = blockIdx.y;
    const float* in = a.in[bi];
    const float* gsrc[NGB];
#pragma unroll
    for (int b = 0; b < NGB; ++b) gsrc[b] = a.g[bi][b];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = lane & 1, kk = lane >> 1, k = kk < 27 ? kk : 26;              // MFMA-side role: (tap, quad)
    const int gq = lane & 1, gu8 = (lane >> 1) & 7, gt = lane >> 4;             // gather-side role: (tap of 4, row of 8, quad)
    f32x4 acc[NGB][4][2];
#pragma unroll
    for (int b = 0; b < NGB; ++b)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int h = 0; h < 2; ++h) acc[b][c][h] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    int64_t per = (n + gridDim.x - 1) / gridDim.x;
    per = (per + 7) & ~(int64_t)7;
    const int64_t b0 = (int64_t)blockIdx.x * per;
    const int64_t b1 = (b0 + per < n) ? b0 + per : n;
    const char* ubase = reinterpret_cast<const char*>(in - 8);
    const uint32_t uoff = 32u + 16u * gq;
    const int gu = (lane >> 3) & 7, gc = lane & 7;           // the lane's element of an 8-row gradient tile
    const int32_t* tk = tile8t + (gt * 8 + gu8) * 8;
    char* img = reinterpret_cast<char*>(smem + wave * IMG_F4);
    uint32_t wofs[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const int p = 4 * j + gt;
        wofs[j] = (uint32_t)((p < 27 ? LINR_TAP(p) : 27) * WM_PITCH + gu8 * 16 + gq * 8);
    }
    const uint32_t rd0 = (uint32_t)(k * WM_PITCH + q * 8);
    bf16_t* gst[NGB];                                        // where the lane's gradient element goes; lanes 0..7 read a channel's 8 rows
    const uint4_alias* gld[NGB];
#pragma unroll
    for (int b = 0; b < NGB; ++b) {
        gst[b] = reinterpret_cast<bf16_t*>(&sg[wave][b][0]) + gc * 8 + gu;
        gld[b] = reinterpret_cast<const uint4_alias*>(&sg[wave][b][lane & 7]);
    }
    float bsum[NGB], gvn[NGB], gvc[NGB];
#pragma unroll
    for (int b = 0; b < NGB; ++b) bsum[b] = gvn[b] = gvc[b] = 0.0f;
    const int64_t g00 = b0 + 8 * wave;
    int4 ia = make_int4(-1, -1, -1, -1), ib = ia;
    float4 xg[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) xg[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (g00 < b1) {                        // wave-uniform; blocks behind the last row must not touch the tables at all
        const int4 a0 = *reinterpret_cast<const int4*>(tk + g00 * 32);
        const int4 c0 = *reinterpret_cast<const int4*>(tk + g00 * 32 + 4);
#pragma unroll
        for (int b = 0; b < NGB; ++b) gvc[b] = (g00 + gu < n) ? gsrc[b][(g00 + gu) * 8 + gc] : 0.0f;
        const int32_t i0[8] = {a0.x, a0.y, a0.z, a0.w, c0.x, c0.y, c0.z, c0.w};
#pragma unroll
        for (int j = 0; j < 7; ++j) xg[j] = *reinterpret_cast<const float4*>(ubase + (((uint32_t)i0[j] << 5) + uoff));
        const int64_t g1r = g00 + 8 * WW_WAVES;           // spare all -1 groups behind the last row group: no bounds check
        ia = *reinterpret_cast<const int4*>(tk + g1r * 32);
        ib = *reinterpret_cast<const int4*>(tk + g1r * 32 + 4);
#pragma unroll
        for (int b = 0; b < NGB; ++b) gvn[b] = (g1r + gu < n) ? gsrc[b][(g1r + gu) * 8 + gc] : 0.0f;
    }
    // rows 4 .. 7 of the previous group (zeros in front of the first: they add +0): they run while this group's reads are in flight
    s16x4 xo[4], gao[NGB];
#pragma unroll
    for (int c = 0; c < 4; ++c) xo[c] = (s16x4){0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < NGB; ++b) gao[b] = (s16x4){0, 0, 0, 0};
    auto mfmas = [&](const s16x4 (&ga)[NGB], const s16x4 (&xb)[4]) {
        static_for<NGB>([&](auto bc) {
            constexpr int b = decltype(bc)::value;
            static_for<4>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                acc[b][c][0] = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(ga[b], xb[c], acc[b][c][0], 4, 0, 0);
                acc[b][c][1] = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(ga[b], xb[c], acc[b][c][1], 4, 1, 0);
            });
        });
    };
    for (int64_t g0r = g00; g0r < b1; g0r += 8 * WW_WAVES) {
#pragma unroll
        for (int j = 0; j < 7; ++j)          // rb(x) as the rows enter the image
            *reinterpret_cast<uint2*>(img + wofs[j]) = make_uint2(pack2(xg[j].x, xg[j].y), pack2(xg[j].z, xg[j].w));
        float gv[NGB];
#pragma unroll
        for (int b = 0; b < NGB; ++b) {
            gv[b] = gvc[b];
            *gst[b] = f2bf(gv[b]);             // rb(g); the bias sums below take the fp32 value
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            const int32_t idn[8] = {ia.x, ia.y, ia.z, ia.w, ib.x, ib.y, ib.z, ib.w};
#pragma unroll
            for (int j = 0; j < 7; ++j) xg[j] = *reinterpret_cast<const float4*>(ubase + (((uint32_t)idn[j] << 5) + uoff));
            const int64_t g2r = g0r + 16 * WW_WAVES;
            ia = *reinterpret_cast<const int4*>(tk + g2r * 32);
            ib = *reinterpret_cast<const int4*>(tk + g2r * 32 + 4);
#pragma unroll
            for (int b = 0; b < NGB; ++b) {
                gvc[b] = gvn[b];
                gvn[b] = (g2r + gu < n) ? gsrc[b][(g2r + gu) * 8 + gc] : 0.0f;
            }
        }
        uint2 x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = *reinterpret_cast<const uint2*>(img + rd0 + (uint32_t)(u * 16));
        s16x4 galo[NGB], gahi[NGB];
#pragma unroll
        for (int b = 0; b < NGB; ++b) {
            const uint4 t = *gld[b];
            galo[b] = __builtin_bit_cast(s16x4, make_uint2(t.x, t.y));
            gahi[b] = __builtin_bit_cast(s16x4, make_uint2(t.z, t.w));
            bsum[b] += gv[b];
        }
        mfmas(gao, xo);
        // 8 rows x (c0 c1 | c2 c3) -> per channel (rows 0..3 | rows 4..7)
        s16x4 xlo[4];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const uint2 r0 = x[4 * hf], r1 = x[4 * hf + 1], r2 = x[4 * hf + 2], r3 = x[4 * hf + 3];
            const uint2 t[4] = {make_uint2((r0.x & 0xffffu) | (r1.x << 16), (r2.x & 0xffffu) | (r3.x << 16)),
                                make_uint2((r0.x >> 16) | (r1.x & 0xffff0000u), (r2.x >> 16) | (r3.x & 0xffff0000u)),
                                make_uint2((r0.y & 0xffffu) | (r1.y << 16), (r2.y & 0xffffu) | (r3.y << 16)),
                                make_uint2((r0.y >> 16) | (r1.y & 0xffff0000u), (r2.y >> 16) | (r3.y & 0xffff0000u))};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (hf == 0) xlo[c] = __builtin_bit_cast(s16x4, t[c]);
                else xo[c] = __builtin_bit_cast(s16x4, t[c]);
            }
        }
        mfmas(galo, xlo);
#pragma unroll
        for (int b = 0; b < NGB; ++b) gao[b] = gahi[b];
    }
    mfmas(gao, xo);                        // the last group's rows 4 .. 7
    ww_fold<NGB>(acc, bsum, sacc, sbias, a, bi, wave, lane);
}

int linr_wide_mul_wgrad(int ngb, int nblk, int ngroups, const WwArgs& a, const int32_t* tile8t, int64_t n, hipStream_t s) {
    const dim3 grid(nblk, ngroups);
    if (ngb == 1) wmwgrad_k<1><<<grid, WW_WAVES * 64, 0, s>>>(a, tile8t, n);
    else if (ngb == 2) wmwgrad_k<2><<<grid, WW_WAVES * 64, 0, s>>>(a, tile8t, n);
    else if (ngb == 4) wmwgrad_k<4><<<grid, WW_WAVES * 64, 0, s>>>(a, tile8t, n);
    else return LINR_EINVAL;
    return linr_launch_rc();
}
