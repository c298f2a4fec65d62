// Stand-alone weight gradients of the 3x3x3 convolutions on the matrix cores: what the two-kernel schedule (LINR_FUSED_BWD=0),
// block_layers > 1 and the wide executor launch where the fused backward (csrc/fused_bwd.hip) does not apply, and the bitwise
// reference of its partial sums.
#include "common.h"
#include "conv_common.h"

#define WG_WAVES 4          // waves per block of the MFMA weight-gradient kernels (same-box A/B: 2 -> 2.765, 4 -> 2.574, 8 -> 2.596 ms/step)
static_assert(LINR_TILE8T_SPARE == 3 * WG_WAVES, "spconv_wgrad_t_k prefetches two strides of WG_WAVES groups ahead");

// ---- backward-weight on the matrix cores -------------------------------------------------------------------------------------
// gW[k][ci][co] = sum_r x[nbr[k][r]][ci] * g[r][co].  Same wave-per-row-group organisation as spconv_wgrad_k (lane = one
// (offset k, channel quad q) pair, 16-byte gather of that quad for 8 rows at a time, persistent accumulators), but the
// 4 x COUT outer product per lane and row runs as v_mfma_f32_4x4x1_16b_f32 with the A operand broadcast from one block:
//     D[i] on lane l += A(lane 4*abid + i) * B(lane l)          (CBSZ = 4: one block feeds all 16; CBSZ = 3: one per half)
// B = component c of the lane's own gathered quad, A = the output gradient: a wave loads the g rows of its 8-row group
// with ONE coalesced dword load (lane l holds g[row l / COUT][l % COUT]), so block 2u + h (COUT 8) or u (COUT 4) already
// holds g[row u][4h .. 4h+3] and ABID selects it - no per-row gradient loads, no shuffles.  Register i of accumulator
// (c, h) on a lane is gW[k][4q + c][4h + i] of the lane's own pair.  DUAL (the two 4->4 convs of an Inception block):
// lanes 0..31 are conv 0, lanes 32..63 conv 1, each half loads its own gradient matrix and CBSZ = 3 keeps them apart.
// The bias gradient is the column sum of the same gradient tiles (each lane adds up the element it loads; a fixed shuffle
// tree and the waves in order finish it) - no per-row selects in the loop: VALU instructions run on the same FMA units as
// the f32 MFMAs, so every one of them is paid for.  K = 1 keeps exact fp32 FMAs in row order.
struct WgradSrc {
    const float* in; int in_ld;           // gathered matrix (quad q at column 4q)
    const float* g0; int g0_ld;           // output gradient (DUAL: of conv 0)
    const float* g1; int g1_ld;           // DUAL: output gradient of conv 1
};
struct WgradDual { int64_t w_off1, b_off1; };

// IDX: how a lane reads its neighbour indices from nbr[27][ld] - 0: scalar loads, 1: 16-byte loads (table 16-byte aligned, ld % 4 == 0).
// This is the direct-gather form: the fallback for frames without the transposed tiled table and the bitwise reference of
// spconv_wgrad_t_k below.
template <int XQ, int COUT, bool DUAL, int IDX>
__global__ __launch_bounds__(WG_WAVES * 64) void spconv_wgrad_mfma_k(WgradSrc S, const int32_t* __restrict__ nbr, int64_t nbr_ld,
                                                                    int64_t n, LinrWgradDst d, WgradDual dd, Grp gp = Grp()) {
    static_assert(!DUAL || (XQ == 2 && COUT == 4), "dual mode = two 4->4 convolutions");
    {   // group offsets: in, res = g0, act = g1, w/b = slab offsets of conv 0, e0/e1 = of conv 1, e2 = cin_valid override
        const int gi = blockIdx.y;
        S.in += gp.in[gi]; S.g0 += gp.res[gi];
        if (S.g1) S.g1 += gp.act[gi];
        d.w_off += gp.w[gi]; d.b_off += gp.b[gi];
        dd.w_off1 += gp.e0[gi]; dd.b_off1 += gp.e1[gi];
        if (gp.e2[gi] > 0) d.cin_valid = (int)gp.e2[gi];
    }
    constexpr int HB = COUT / 4;
    constexpr int NA = 4 * HB * 4;
    constexpr int CBSZ = DUAL ? 3 : 4;
    __shared__ float sacc[64 * (NA + 1)];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = DUAL ? (lane >> 5) : (XQ == 2 ? (lane & 1) : 0);
    const int kk = DUAL ? (lane & 31) : (XQ == 2 ? (lane >> 1) : lane);          // >= 27: idle lanes
    const bool live = kk < 27;
    const int k = live ? kk : 26;
    f32x4 acc[4][HB];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int h = 0; h < HB; ++h) acc[c][h] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    int64_t per = (n + gridDim.x - 1) / gridDim.x;
    per = (per + 7) & ~(int64_t)7;
    const int64_t b0 = (int64_t)blockIdx.x * per;
    const int64_t b1 = (b0 + per < n) ? b0 + per : n;
    const int32_t* nk = nbr + (int64_t)k * nbr_ld;
    const char* pad = reinterpret_cast<const char*>(S.in - S.in_ld) + 16 * q;
    const uint32_t rsh = __builtin_amdgcn_readfirstlane(S.in_ld == 8 ? 5u : 4u);      // 32- or 16-byte rows: a uniform shift, not a multiply
    // this lane's element of the 8-row gradient tile: row gu, channel gc of matrix gsel
    const float* gsel = (DUAL && q) ? S.g1 : S.g0;
    const int gld = (DUAL && q) ? S.g1_ld : S.g0_ld;
    const int gl = DUAL ? (lane & 31) : lane;
    const int gu = (gl / COUT) & 7, gc = gl % COUT;
    const int ncomp = __builtin_amdgcn_readfirstlane(d.cin_valid);      // live components per quad (>= 4: all)
    float bsum = 0.0f;
    for (int64_t g0r = b0 + 8 * wave; g0r < b1; g0r += 8 * WG_WAVES) {
        int32_t idx[8];
        if (IDX >= 1 && g0r + 8 <= n) {
            const int4 a = *reinterpret_cast<const int4*>(nk + g0r);
            const int4 b = *reinterpret_cast<const int4*>(nk + g0r + 4);
            idx[0] = a.x; idx[1] = a.y; idx[2] = a.z; idx[3] = a.w;
            idx[4] = b.x; idx[5] = b.y; idx[6] = b.z; idx[7] = b.w;
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) idx[u] = (g0r + u < n) ? nk[g0r + u] : -1;
        }
        const float gv = (g0r + gu < n) ? gsel[(g0r + gu) * gld + gc] : 0.0f;
        float4 x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            x[u] = *reinterpret_cast<const float4*>(pad + ((uint32_t)(idx[u] + 1) << rsh));
        }
        bsum += gv;                      // bias gradient: column sums of the gradient rows (lanes beyond the 27 offsets
                                         // gather offset 26's rows again; their products are never written)
        static_for<8>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            static_for<HB>([&](auto hc) {
                constexpr int h = decltype(hc)::value;
                constexpr int ab = u * HB + h;           // the block holding g[row u][4h .. 4h+3]
                // first convs of the outter blocks (cin_valid = 1..7): component c of a quad is input channel >= c, so it
                // is dead in BOTH quads once c >= cin_valid (wave-uniform: cin_valid is a kernel argument)
                acc[0][h] = __builtin_amdgcn_mfma_f32_4x4x1f32(gv, x[u].x, acc[0][h], CBSZ, ab, 0);
                if (DUAL || ncomp > 1) acc[1][h] = __builtin_amdgcn_mfma_f32_4x4x1f32(gv, x[u].y, acc[1][h], CBSZ, ab, 0);
                if (DUAL || ncomp > 2) acc[2][h] = __builtin_amdgcn_mfma_f32_4x4x1f32(gv, x[u].z, acc[2][h], CBSZ, ab, 0);
                if (DUAL || ncomp > 3) acc[3][h] = __builtin_amdgcn_mfma_f32_4x4x1f32(gv, x[u].w, acc[3][h], CBSZ, ab, 0);
            });
        });
    }
    // fold waves in wave order (fixed => reproducible)
    float* mine = sacc + lane * (NA + 1);
    for (int w = 0; w < WG_WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int h = 0; h < HB; ++h)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int e = (c * HB + h) * 4 + i;
                        mine[e] = (w == 0) ? acc[c][h][i] : mine[e] + acc[c][h][i];
                    }
        }
        __syncthreads();
    }
    // bias gradient: lane l holds the partial column sum of channel gc over rows gu, gu + 8, ...: add the 8 row phases with
    // a fixed xor tree, then the waves in order
    __shared__ float sbias[WG_WAVES][16];
    {
        float t = bsum;
#pragma unroll
        for (int m = COUT; m < 8 * COUT; m <<= 1) t += __shfl_xor(t, m, 64);
        const int slot = DUAL ? ((lane >> 5) * 4 + (lane & 3)) : (lane % COUT);          // lanes 0..COUT-1 (and 32..35 for DUAL)
        if ((lane & 31) < COUT && (DUAL || lane < 32)) sbias[wave][slot] = t;
        __syncthreads();
    }
    // register i of accumulator (c, h) on lane (kk, q)  <->  input channel 4q + c, output channel 4h + i of offset kk.  The
    // folded sums sit in LDS (sacc[lane][slot]); ALL threads copy them out in DESTINATION order, so the block's slab row is
    // written with coalesced dword stores (one lane-per-accumulator store per element would be 1,728 scattered 4-byte writes)
    {
        float* dst = d.base + (int64_t)blockIdx.x * d.block_stride;
        const int tid = threadIdx.x;
        if (tid < (DUAL ? 8 : COUT)) {
            float t = sbias[0][tid];
            for (int w = 1; w < WG_WAVES; ++w) t += sbias[w][tid];
            if (DUAL) dst[(tid < 4 ? d.b_off : dd.b_off1) + (tid & 3)] = t;
            else dst[d.b_off + tid] = t;
        }
        if constexpr (DUAL) {
            for (int e = tid; e < 2 * 432; e += WG_WAVES * 64) {
                const int t = e / 432, r = e - 432 * t;
                const int kq = r >> 4, slot = r & 15;                 // slot = ci * 4 + co (HB = 1)
                dst[(t ? dd.w_off1 : d.w_off) + r] = sacc[(32 * t + kq) * (NA + 1) + slot];
            }
        } else {
            const int cinv = d.cin_valid;
            const int per_k = cinv * COUT, total = 27 * per_k;
            for (int e = tid; e < total; e += WG_WAVES * 64) {
                const int kq = e / per_k, r = e - kq * per_k;
                const int ci = r / COUT, co = r - ci * COUT;
                const int ln = (XQ == 2) ? 2 * kq + (ci >> 2) : kq;
                const int slot = ((ci & 3) * HB + (co >> 2)) * 4 + (co & 3);
                dst[d.w_off + e] = sacc[ln * (NA + 1) + slot];
            }
        }
    }
}

// ---- weight gradients with COALESCED gathers and an LDS transpose --------------------------------------------------------------
// All weight-gradient kernels above take ~20 us per row pass whatever their MFMA count (8->8: 64 MFMAs per group, 8->4 and the
// dual 4->4: 32): they are bound by the L1 return path.  With lane = (tap, channel quad) a gather instruction delivers 54
// 16-byte pieces from ~20 different cache lines - about 55 % of the rate the convolutions reach with lane = row on the same
// bytes.  Here the gather of an 8-row group is laid out the convolutions' way - lane = (tap t of 4, row u of 8, quad q): one
// instruction fetches 4 taps x 8 CONSECUTIVE rows, i.e. four 256-byte runs - into a wave-private tap-major LDS image
// [tap][row][quad] with a tap pitch of 8 x 32 + 32 bytes, and every (tap, quad) lane reads its eight rows back with
// ds_read_b128: the pitch makes the 16-byte slot index (2 tap + quad + 2 row) mod 16 = (lane + 2 row) mod 16, distinct inside each of
// the hardware's 16-lane groups; the writes are 128 contiguous bytes per 8 lanes.  (SQ_LDS_BANK_CONFLICT still reads 3.4e5 cycles
// per launch, profiles/r02_pmc_wgrad_variants.txt: a few per cent of the LDS cycles, not attributed - the fold epilogue's
// stride-(NA + 1) accesses are the candidate, the row loop's accesses are conflict-free by construction.)  No block barrier (LDS operations of one wave
// execute in order).  Indices come from a second tiled table (linr_kmap_tile8t: [group][tap of 4][row][tap group j] so that a
// lane's seven indices are 32 contiguous bytes).  Pipeline: while the MFMAs of group t run, the gathers of group t+1 and the
// indices of group t+2 are in flight.  Same groups, same order, same MFMAs => same partial sums, bit for bit.
#define TW_PITCH 288                  // bytes per tap in the LDS image: 8 rows x 32 B + 32 B
#define TW_TAPS 28                    // 27 taps + one dump slot for the unused lane group of the 7th gather
template <int COUT, bool DUAL>
__global__ __launch_bounds__(WG_WAVES * 64) void spconv_wgrad_t_k(WgradSrc S, const int32_t* __restrict__ tile8t, int64_t n,
                                                                 LinrWgradDst d, WgradDual dd, Grp gp = Grp()) {
    static_assert(!DUAL || COUT == 4, "dual mode = two 4->4 convolutions");
    {
        const int gi = blockIdx.y;
        S.in += gp.in[gi]; S.g0 += gp.res[gi];
        if (S.g1) S.g1 += gp.act[gi];
        d.w_off += gp.w[gi]; d.b_off += gp.b[gi];
        dd.w_off1 += gp.e0[gi]; dd.b_off1 += gp.e1[gi];
        if (gp.e2[gi] > 0) d.cin_valid = (int)gp.e2[gi];
    }
    constexpr int HB = COUT / 4;
    constexpr int NA = 4 * HB * 4;
    constexpr int CBSZ = DUAL ? 3 : 4;
    // one LDS buffer: the four wave-private images during the row loop, the fold scratch afterwards (32 KB per block: four
    // blocks per CU)
    constexpr int IMG_F4 = TW_TAPS * TW_PITCH / 16;
    constexpr int FOLD_F4 = 16 * (NA + 1);                 // one wave's accumulators: 64 lanes x (NA + 1) floats
    constexpr int SMEM_F4 = WG_WAVES * (IMG_F4 > FOLD_F4 ? IMG_F4 : FOLD_F4);
    __shared__ float4 smem[SMEM_F4];
    float* sacc = reinterpret_cast<float*>(smem);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // MFMA-side role of the lane: (tap kk, quad q) as in spconv_wgrad_mfma_k
    const int q = DUAL ? (lane >> 5) : (lane & 1);
    const int kk = DUAL ? (lane & 31) : (lane >> 1);
    const int k = kk < 27 ? kk : 26;
    // gather-side role: (tap t of the instruction's 4, row u, quad gq)
    const int gq = lane & 1, gu8 = (lane >> 1) & 7, gt = lane >> 4;
    f32x4 acc[4][HB];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int h = 0; h < HB; ++h) acc[c][h] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    int64_t per = (n + gridDim.x - 1) / gridDim.x;
    per = (per + 7) & ~(int64_t)7;
    const int64_t b0 = (int64_t)blockIdx.x * per;
    const int64_t b1 = (b0 + per < n) ? b0 + per : n;
    // gathers in saddr form: uniform base (the zero pad row) + a 32-bit lane offset ((index + 1) * 32 + 16 quad)
    const char* ubase = reinterpret_cast<const char*>(S.in - 8);
    const uint32_t uoff = 32u + 16u * gq;
    const float* gsel = (DUAL && q) ? S.g1 : S.g0;
    const int gld = (DUAL && q) ? S.g1_ld : S.g0_ld;
    const int gl = DUAL ? (lane & 31) : lane;
    const int gu = (gl / COUT) & 7, gc = gl % COUT;
    // the lane's 8 indices (7 used) of a group: tile8t[group][gt][gu8][0..7]
    const int32_t* tk = tile8t + (gt * 8 + gu8) * 8;
    char* img = reinterpret_cast<char*>(smem + wave * IMG_F4);
    // write position of gather j: the tap at position 4 j + gt of the slab-major sequence (position 27 = the dump slot); read
    // position of MFMA row u: tap k
    uint32_t wofs[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const int p = 4 * j + gt;
        wofs[j] = (uint32_t)((p < 27 ? LINR_TAP(p) : 27) * TW_PITCH + gu8 * 32 + gq * 16);
    }
    const uint32_t rd0 = (uint32_t)(k * TW_PITCH + q * 16);
    float bsum = 0.0f;
    const int64_t g00 = b0 + 8 * wave;
    int4 ia = make_int4(-1, -1, -1, -1), ib = ia;
    float gvn = 0.0f, gvc = 0.0f;
    float4 xg[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) xg[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (g00 < b1) {                        // wave-uniform; blocks behind the last row must not touch the tables at all
        const int4 a0 = *reinterpret_cast<const int4*>(tk + g00 * 32);
        const int4 c0 = *reinterpret_cast<const int4*>(tk + g00 * 32 + 4);
        gvc = (g00 + gu < n) ? gsel[(g00 + gu) * gld + gc] : 0.0f;
        const int32_t i0[8] = {a0.x, a0.y, a0.z, a0.w, c0.x, c0.y, c0.z, c0.w};
#pragma unroll
        for (int j = 0; j < 7; ++j) xg[j] = *reinterpret_cast<const float4*>(ubase + (((uint32_t)i0[j] << 5) + uoff));
        const int64_t g1r = g00 + 8 * WG_WAVES;           // spare all -1 groups behind the last row group: no bounds check
        ia = *reinterpret_cast<const int4*>(tk + g1r * 32);
        ib = *reinterpret_cast<const int4*>(tk + g1r * 32 + 4);
        gvn = (g1r + gu < n) ? gsel[(g1r + gu) * gld + gc] : 0.0f;
    }
    for (int64_t g0r = g00; g0r < b1; g0r += 8 * WG_WAVES) {
        // (a) the gathered pieces of this group (requested one iteration ago) -> LDS image, tap-major
#pragma unroll
        for (int j = 0; j < 7; ++j) *reinterpret_cast<float4*>(img + wofs[j]) = xg[j];
        __builtin_amdgcn_sched_barrier(0);      // writes first: hoisting the next gathers above them costs 14 register-pair copies
        const float gv = gvc;
        // (b) next group's gathers (its indices arrived during the last MFMAs) and the indices of the group after it
        {
            const int32_t idn[8] = {ia.x, ia.y, ia.z, ia.w, ib.x, ib.y, ib.z, ib.w};
#pragma unroll
            for (int j = 0; j < 7; ++j) xg[j] = *reinterpret_cast<const float4*>(ubase + (((uint32_t)idn[j] << 5) + uoff));
            gvc = gvn;
            const int64_t g2r = g0r + 16 * WG_WAVES;
            ia = *reinterpret_cast<const int4*>(tk + g2r * 32);
            ib = *reinterpret_cast<const int4*>(tk + g2r * 32 + 4);
            gvn = (g2r + gu < n) ? gsel[(g2r + gu) * gld + gc] : 0.0f;
        }
        // (c) transposed read: this lane's (tap, quad) for the 8 rows of the group
        float4 x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = *reinterpret_cast<const float4*>(img + rd0 + (uint32_t)(u * 32));
        bsum += gv;
        static_for<8>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            static_for<HB>([&](auto hc) {
                constexpr int h = decltype(hc)::value;
                constexpr int ab = u * HB + h;
                // all four components unconditionally: the cin_valid skip of spconv_wgrad_mfma_k (scalar branches between the
                // MFMAs) costs this kernel more than the dead MFMAs of the three narrow first convs do (2.213 vs 2.227 ms/step);
                // accumulators of input channels >= cin_valid are never written out
                acc[0][h] = __builtin_amdgcn_mfma_f32_4x4x1f32(gv, x[u].x, acc[0][h], CBSZ, ab, 0);
                acc[1][h] = __builtin_amdgcn_mfma_f32_4x4x1f32(gv, x[u].y, acc[1][h], CBSZ, ab, 0);
                acc[2][h] = __builtin_amdgcn_mfma_f32_4x4x1f32(gv, x[u].z, acc[2][h], CBSZ, ab, 0);
                acc[3][h] = __builtin_amdgcn_mfma_f32_4x4x1f32(gv, x[u].w, acc[3][h], CBSZ, ab, 0);
            });
        });
    }
    __syncthreads();
    // Every wave parks its accumulators in its own LDS slice; the copy-out below adds the four slices in wave order
    // (((w0 + w1) + w2) + w3: the association of the former wave-by-wave fold, so the bits do not change) - one barrier instead
    // of four and no read-modify-write passes.
    {
        float* mine = sacc + (wave * 64 + lane) * (NA + 1);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int h = 0; h < HB; ++h)
#pragma unroll
                for (int i = 0; i < 4; ++i) mine[(c * HB + h) * 4 + i] = acc[c][h][i];
    }
    __shared__ float sbias[WG_WAVES][16];
    {
        float t = bsum;
#pragma unroll
        for (int m = COUT; m < 8 * COUT; m <<= 1) t += __shfl_xor(t, m, 64);
        const int slot = DUAL ? ((lane >> 5) * 4 + (lane & 3)) : (lane % COUT);
        if ((lane & 31) < COUT && (DUAL || lane < 32)) sbias[wave][slot] = t;
        __syncthreads();
    }
    {
        auto fold4 = [&](int e) {
            constexpr int W = 64 * (NA + 1);
            float t = sacc[e];
#pragma unroll
            for (int w = 1; w < WG_WAVES; ++w) t += sacc[w * W + e];
            return t;
        };
        float* dst = d.base + (int64_t)blockIdx.x * d.block_stride;
        const int tid = threadIdx.x;
        if (tid < (DUAL ? 8 : COUT)) {
            float t = sbias[0][tid];
            for (int w = 1; w < WG_WAVES; ++w) t += sbias[w][tid];
            if (DUAL) dst[(tid < 4 ? d.b_off : dd.b_off1) + (tid & 3)] = t;
            else dst[d.b_off + tid] = t;
        }
        if constexpr (DUAL) {
            for (int e = tid; e < 2 * 432; e += WG_WAVES * 64) {
                const int t = e / 432, r = e - 432 * t;
                dst[(t ? dd.w_off1 : d.w_off) + r] = fold4((32 * t + (r >> 4)) * (NA + 1) + (r & 15));
            }
        } else {
            const int cinv = d.cin_valid;
            if (cinv == 8) {          // all but the first convs of the outter blocks: constant divisors (a runtime division costs ~20 VALU ops)
                for (int e = tid; e < 27 * 8 * COUT; e += WG_WAVES * 64) {
                    const int kq = e / (8 * COUT), r = e % (8 * COUT);
                    const int ci = r / COUT, co = r % COUT;
                    dst[d.w_off + e] = fold4((2 * kq + (ci >> 2)) * (NA + 1) + ((ci & 3) * HB + (co >> 2)) * 4 + (co & 3));
                }
            } else {
                const int per_k = cinv * COUT, total = 27 * per_k;
                for (int e = tid; e < total; e += WG_WAVES * 64) {
                    const int kq = e / per_k, r = e - kq * per_k;
                    const int ci = r / COUT, co = r - ci * COUT;
                    dst[d.w_off + e] = fold4((2 * kq + (ci >> 2)) * (NA + 1) + ((ci & 3) * HB + (co >> 2)) * 4 + (co & 3));
                }
            }
        }
    }
}

int linr_conv3_wgrad_mfma(const WgradGroup* g, int ng, int in_ld, int gout_ld, const int32_t* nbr, int64_t nbr_ld, int64_t n,
                          const int32_t* tile8t, int cin, int cout, float* big, int64_t block_stride, int nblocks, hipStream_t s) {
    if (ng < 1 || ng > LINR_MAXG) return LINR_EINVAL;
    if (in_ld != 8 && in_ld != 4) return LINR_EINVAL;  // the kernels address gathered rows by a shift: 32- or 16-byte rows
    const int idx = (nbr_ld % 4 == 0 && linr_aligned16(nbr)) ? 1 : 0;
    Grp gp = Grp();
    for (int i = 0; i < ng; ++i) {
        gp.in[i] = g[i].in - g[0].in; gp.res[i] = g[i].gout - g[0].gout; gp.w[i] = g[i].w_off - g[0].w_off;
        gp.b[i] = g[i].b_off - g[0].b_off; gp.e2[i] = g[i].cin_live;
    }
    const float* in = g[0].in;
    const dim3 grid(nblocks, ng);
    WgradSrc S = {in, in_ld, g[0].gout, gout_ld, nullptr, 0};
    LinrWgradDst d = {big, block_stride, g[0].w_off, g[0].b_off, cin};
    WgradDual dd = {0, 0};
    // coalesced gathers + LDS transpose: 32-byte rows, the transposed tiled table
    if (tile8t && in_ld == 8 && cin <= 8 && (cout == 8 || (cout == 4 && cin == 8)) && linr_aligned16(in) && linr_aligned16(tile8t)) {
        if (cout == 8) spconv_wgrad_t_k<8, false><<<grid, WG_WAVES * 64, 0, s>>>(S, tile8t, n, d, dd, gp);
        else spconv_wgrad_t_k<4, false><<<grid, WG_WAVES * 64, 0, s>>>(S, tile8t, n, d, dd, gp);
        return linr_launch_rc();
    }
#define GO(XQ, CO)                                                                                                           \
    do {                                                                                                                     \
        if (idx == 1) spconv_wgrad_mfma_k<XQ, CO, false, 1><<<grid, WG_WAVES * 64, 0, s>>>(S, nbr, nbr_ld, n, d, dd, gp);   \
        else spconv_wgrad_mfma_k<XQ, CO, false, 0><<<grid, WG_WAVES * 64, 0, s>>>(S, nbr, nbr_ld, n, d, dd, gp);            \
        return linr_launch_rc();                                                                                             \
    } while (0)
    if (cin == 8 && cout == 8) GO(2, 8);
    if (cin == 8 && cout == 4) GO(2, 4);
    if (cin == 4 && cout == 4) GO(1, 4);
    if (cin < 8 && cout == 8 && in_ld >= 8) GO(2, 8);
#undef GO
    return LINR_EINVAL;
}

// both 4->4 convolutions of an Inception block: in = H [n][8]; conv 0 reads H[:,0:4] with gradient g0, conv 1 H[:,4:8] with g1
int linr_conv3_wgrad_dual44(const Dual44BwdGroup* g, int ng, int gI_ld, int gM_ld, const int32_t* nbr, int64_t nbr_ld, int64_t n,
                            const int32_t* tile8t, float* big, int64_t block_stride, int nblocks, hipStream_t s) {
    if (ng < 1 || ng > LINR_MAXG) return LINR_EINVAL;
    const int idx = (nbr_ld % 4 == 0 && linr_aligned16(nbr)) ? 1 : 0;
    Grp gp = Grp();
    for (int i = 0; i < ng; ++i) {
        gp.in[i] = g[i].H - g[0].H; gp.res[i] = g[i].gI - g[0].gI; gp.act[i] = g[i].gM - g[0].gM;
        gp.w[i] = g[i].w01_off - g[0].w01_off; gp.b[i] = g[i].b01_off - g[0].b01_off;
        gp.e0[i] = g[i].w11_off - g[0].w11_off; gp.e1[i] = g[i].b11_off - g[0].b11_off;
    }
    const float* H = g[0].H;
    const dim3 grid(nblocks, ng);
    WgradSrc S = {H, 8, g[0].gI, gI_ld, g[0].gM, gM_ld};
    LinrWgradDst d = {big, block_stride, g[0].w01_off, g[0].b01_off, 4};
    WgradDual dd = {g[0].w11_off, g[0].b11_off};
    if (tile8t && linr_aligned16(H) && linr_aligned16(tile8t)) {
        spconv_wgrad_t_k<4, true><<<grid, WG_WAVES * 64, 0, s>>>(S, tile8t, n, d, dd, gp);
        return linr_launch_rc();
    }
    if (idx == 1) spconv_wgrad_mfma_k<2, 4, true, 1><<<grid, WG_WAVES * 64, 0, s>>>(S, nbr, nbr_ld, n, d, dd, gp);
    else spconv_wgrad_mfma_k<2, 4, true, 0><<<grid, WG_WAVES * 64, 0, s>>>(S, nbr, nbr_ld, n, d, dd, gp);
    return linr_launch_rc();
}

// The executor's backward-weight kernel through its own entry: per-block partial sums of
//   gW[k][ci][co] = sum_r in[nbr_k(r)][ci] gout[r][co],  gb[co] = sum_r gout[r][co]
// into slab[b * (27 cin + 1) cout + (k cin + ci) cout + co] (bias row last), b < LINR_WG_BLOCKS (512); the caller sums the
// 512 partials in ascending order (the executor does so for all parameters at once in wgrad_reduce_k).
extern "C" int64_t linr_spconv_wgrad_cmap_blocks(void) { return LINR_WG_BLOCKS; }

extern "C" int linr_spconv_wgrad_cmap(const float* in, int32_t in_ld, const float* gout, int32_t gout_ld, const int32_t* nbr,
                                      const int32_t* tile8t, int64_t ld, int64_t n, int32_t cin, int32_t cout, float* slab,
                                      void* stream) {
    if (n < 0 || ld < n || in_ld != 8 || gout_ld < cout) return LINR_EINVAL;
    if (n == 0) return 0;
    if (!in || !gout || !nbr || !slab) return LINR_EINVAL;
    if (!linr_aligned16(in)) return LINR_EALIGN;
    if (!((cin == 8 && (cout == 8 || cout == 4)) || (cin < 8 && cin >= 1 && cout == 8))) return LINR_EINVAL;
    if (!linr_rows_fit32(n)) return LINR_EINVAL;
    const int64_t elems = (int64_t)(27 * cin + 1) * cout;
    if (tile8t && !linr_aligned16(tile8t)) return LINR_EALIGN;
    const WgradGroup g = {in, gout, 0, (int64_t)27 * cin * cout, 0};
    return linr_conv3_wgrad_mfma(&g, 1, in_ld, gout_ld, nbr, ld, n, tile8t, cin, cout, slab, elems, LINR_WG_BLOCKS, (hipStream_t)stream);
}

extern "C" int linr_spconv_wgrad_dual44(const float* H, const float* g0, int32_t g0_ld, const float* g1, int32_t g1_ld,
                                        const int32_t* nbr, const int32_t* tile8t, int64_t ld, int64_t n, float* slab, void* stream) {
    if (n < 0 || ld < n || g0_ld < 4 || g1_ld < 4) return LINR_EINVAL;
    if (n == 0) return 0;
    if (!H || !g0 || !g1 || !nbr || !slab) return LINR_EINVAL;
    if (!linr_aligned16(H)) return LINR_EALIGN;
    if (!linr_rows_fit32(n)) return LINR_EINVAL;
    // per block: [W01 432 | b01 4 | W11 432 | b11 4]
    const Dual44BwdGroup g = {g0, g1, H, nullptr, nullptr, nullptr, 0, 432, 436, 868};
    return linr_conv3_wgrad_dual44(&g, 1, g0_ld, g1_ld, nbr, ld, n, tile8t, slab, 872, LINR_WG_BLOCKS, (hipStream_t)stream);
}
