// What every backward pass ends with, for the fp32 executor (csrc/net.hip) and the bf16 training executor (csrc/train_bf16.hip) alike:
// the backward of the scale context, the fixed-order reduction of the per-block partial weight gradients [nb][n_params] into the
// gradient of the call, the scale-embedding gradients derived from the reduced sums, and torch.optim.Adam's step over the flat
// parameter buffer - with the stand-alone op entries of the same kernels (include/linr_hip.h: linr_sce_bwd*, linr_axpy).
#include "bwd_tail.h"
#include "conv_common.h"
#include "prof.h"
#include "sce.h"
#include <math.h>
#include <stdlib.h>

#define TRY(e) do { int rc_ = (e); if (rc_) return rc_; } while (0)

// Persistent blocks per weight-gradient launch (multiples of 32: wgrad_reduce_k's association).  Every block ends with a fold
// over its waves and writes one slab row per parameter, and the final reduction reads nb x n_params floats: fixed costs that
// grow with nb, while the grouped launches (8 groups since block_in joined them) bring nb x 8 blocks anyway.  Measured,
// ms/step with the joined schedule: 337 k rows (loot10): 512 -> 2.291, 384 -> 2.277, 256 -> 2.271, 192 -> 2.305, 160 -> 2.293,
// 128 -> 2.285; 373 k rows (andrew10): 512 -> 2.626, 256 -> 2.614, 160 -> 2.656; 54 k rows (sphere8): 384 -> 0.566, 256 -> 0.533,
// 192 -> 0.532, 128 -> 0.506, 96 -> 0.509, 64 -> 0.531 (profiles/r02_ab_wg_blocks.txt).  The block count decides how the partial
// sums associate, i.e. the rounding of the gradients; nothing else depends on it (tests: test_block_count_changes_only_the_rounding).
int linr_wg_blocks_for(int64_t rows) {
    static const int forced = getenv("LINR_WG_BLOCKS") ? atoi(getenv("LINR_WG_BLOCKS")) : 0;
    if (forced >= 32 && forced <= LINR_WG_BLOCKS && forced % 32 == 0) return forced;
    return rows >= 100000 ? 256 : 128;
}

// ghid[r] = (W2^T gx0[r]) * (hid[r] > 0)     (linear_k<8,16> with the ReLU mask, weights of r's scale)
__global__ __launch_bounds__(LINR_BLOCK) void sce_bwd_k(const float* __restrict__ P, SceArgs a, int64_t n,
                                                        const float* __restrict__ gx0, const float* __restrict__ hid,
                                                        float* __restrict__ ghid) {
    int s;
    const int64_t r = sce_row_of(a, (int)blockIdx.x, s);
    if (r < 0) return;
    const float* W2 = P + a.w2[s];
    const float4 g0 = *reinterpret_cast<const float4*>(gx0 + r * 8);
    const float4 g1 = *reinterpret_cast<const float4*>(gx0 + r * 8 + 4);
    const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    float acc[16];
#pragma unroll
    for (int o = 0; o < 16; ++o) acc[o] = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int o = 0; o < 16; ++o) acc[o] = fmaf(g[i], W2[i * 16 + o], acc[o]);
    const float4* hp = reinterpret_cast<const float4*>(hid + r * 16);
    float4* op = reinterpret_cast<float4*>(ghid + r * 16);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const float4 h = hp[v];
        op[v] = make_float4(h.x > 0.0f ? acc[4 * v] : 0.0f, h.y > 0.0f ? acc[4 * v + 1] : 0.0f,
                            h.z > 0.0f ? acc[4 * v + 2] : 0.0f, h.w > 0.0f ? acc[4 * v + 3] : 0.0f);
    }
}

// The whole backward of the scale context in ONE launch (grid: slab rows x scales): per row ghid = (W2^T gx0) * (hid > 0) with the
// scale's weights from the scalar cache (the fmaf chain of sce_bwd_k), and all four parameter gradients as X^T G products with the
// rows as the K dimension of v_mfma_f32_16x16x4_f32 (xtg_wgrad_k's scheme):
//   gW1[m][i] = sum_r ghid[r][m] * [emb | offset_feat | 1][r][i]   (column 15 = the bias gradient gb1),
//   gW2[o][i] = sum_r gx0[r][o] * hid[r][i],   gb2[o] = sum_r gx0[r][o]  (per-lane sums, fixed shuffle tree)
// Each wave passes its 64 rows through a wave-private LDS tile [row][ghid 16 | x 16 | gx0 8 | hid 16] to turn "lane = row" into
// the fragment layout.  Neither ghid nor the MLP input is written to memory (round 2/3: a 64 B/row matrix each, read back by two
// pointwise weight-gradient launches).  One slab row per workgroup and scale, the four waves folded in order.
#define SB_LD 57
#ifndef SB_LAB
#define SB_LAB 0            // lab builds (tools/lab_build.sh bwd_tail <tag> -DSB_LAB=mask): 1 no X^T G loop, 2 no LDS tile writes, 4 no gh / h arithmetic, 8 one tile per wave only
#endif
#define SB_WAVES 4          // (8 waves per workgroup = one workgroup per CU: 63.6 instead of 50.3 us per step for the two scale-context kernels)
__global__ __launch_bounds__(SB_WAVES * 64) void sce_bwd_all_k(const float* __restrict__ P, const float* __restrict__ off, SceArgs a,
                                                            const float* __restrict__ gx0, const float* __restrict__ hid,
                                                            float* __restrict__ big, int64_t block_stride) {
    __shared__ float sT[SB_WAVES * 64 * SB_LD];
    __shared__ float sfold[64 * 9];
    __shared__ float sb2[SB_WAVES * 8];
    int s = 0;                                                 // scale of this workgroup: uniform
    for (int i = 1; i < a.n_scales; ++i) s += ((int)blockIdx.x >= a.wg_off[i]) ? 1 : 0;
    const int sb = (int)blockIdx.x - a.wg_off[s], nsb = a.wg_off[s + 1] - a.wg_off[s];          // slab row, rows of this scale
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int mm = lane & 15, rr = lane >> 4;
    const float* emb = P + a.emb[s];
    const float* W2 = P + a.w2[s];
    const int64_t r0 = a.row_off[s], n = a.row_off[s + 1] - r0;
    int64_t per = (n + nsb - 1) / nsb;
    per = (per + 15) & ~(int64_t)15;
    const int64_t b0 = (int64_t)sb * per;
    const int64_t b1 = (b0 + per < n) ? b0 + per : n;
    float* T = sT + wave * 64 * SB_LD;
    // gh = g W2 on v_mfma_f32_4x4x1 with the weight 4-vector broadcast (CBSZ = 4), K = 1 - each instruction is one fmaf per output, output
    // gradients ascending from 0 like the loop it replaces (same bits): the 128 weights are TWO registers per lane (combo 4 i + oq ->
    // W2[i][4 oq + j], block (lane >> 2) of register v is combo 16 v + block) where rounds 2-5 pinned them into 128 vector registers
    // per lane (one workgroup per CU; now two, LDS-bound).  Worth ~1 us of the kernel's 21-22 (profiles/r06_sce_lab.txt).
    float wG[2];
    {
        const int blk = lane >> 2, j4 = lane & 3;
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int cb = 16 * v + blk;
            wG[v] = W2[(cb >> 2) * 16 + 4 * (cb & 3) + j4];
        }
    }
    // sce_fwd_k's weight image of the first layer (csrc/sce.h: combo 4 i + hq -> W1[4 hq + j][i], 60 + hq -> b1[4 hq + j])
    float wA[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (hid == nullptr) {
        const float* W1 = P + a.w1[s];
        const float* b1p = P + a.b1[s];
        const int blk = lane >> 2, j4 = lane & 3;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int cb = 16 * v + blk;
            wA[v] = cb < 60 ? W1[(4 * (cb & 3) + j4) * 15 + (cb >> 2)] : b1p[4 * (cb - 60) + j4];
        }
    }
    f32x4 acc1 = {0.0f, 0.0f, 0.0f, 0.0f}, acc2 = {0.0f, 0.0f, 0.0f, 0.0f};
    float bs[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bs[j] = 0.0f;
    // The inputs of a wave's NEXT tile are loaded while the current one is worked on (pinned by a scheduling barrier; rows behind the
    // range read its last row, masked by `live`).  The kernel's time is mostly fixed cost per workgroup - one tile per wave instead of
    // 3.75 still takes 17 of the 22 us (607 workgroups of 63 KB LDS on 512 slots: two rounds of prologue, tile, fold) - see
    // profiles/r06_sce_lab.txt.
    float4 ng0, ng1;
    float noff[7];
    auto fetch = [&](int64_t c0) {
        const int64_t row = c0 + lane;
        const int64_t r = r0 + (row < b1 ? row : b1 - 1);
        ng0 = *reinterpret_cast<const float4*>(gx0 + r * 8); ng1 = *reinterpret_cast<const float4*>(gx0 + r * 8 + 4);
#pragma unroll
        for (int i = 0; i < 7; ++i) noff[i] = off[r * 7 + i];
    };
    if (b0 + 64 * wave < b1) fetch(b0 + 64 * wave);
    for (int64_t c0 = b0 + 64 * wave; c0 < b1; c0 += 64 * SB_WAVES) {
        const int64_t row = c0 + lane;
        const bool live = row < b1;
        const int64_t r = r0 + (live ? row : b1 - 1);
        const float g[8] = {ng0.x, ng0.y, ng0.z, ng0.w, ng1.x, ng1.y, ng1.z, ng1.w};
        float x[16];
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = emb[i];
#pragma unroll
        for (int i = 0; i < 7; ++i) x[8 + i] = noff[i];
        x[15] = 1.0f;                                          // the bias gradient's pseudo input
        fetch(c0 + 64 * SB_WAVES);
        __builtin_amdgcn_sched_barrier(0);
        float h[16];
        if constexpr ((SB_LAB & 4) != 0) {
#pragma unroll
            for (int o = 0; o < 16; ++o) h[o] = x[o];
        } else
        if (hid != nullptr) {                                  // (uniform) the op-level entry hands the forward's hidden layer in
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float4 t = *reinterpret_cast<const float4*>(hid + r * 16 + 4 * v);
                h[4 * v] = t.x; h[4 * v + 1] = t.y; h[4 * v + 2] = t.z; h[4 * v + 3] = t.w;
            }
        } else {
            // the executors do not keep the hidden layer (64 bytes per row written by the forward and read back here): it is recomputed
            // with sce_fwd_k's own instruction sequence - same bits - from inputs this kernel loads anyway
            f32x4 hq4[4];
            static_for<4>([&](auto hc) {
                constexpr int hq = decltype(hc)::value;
                hq4[hq] = __builtin_amdgcn_mfma_f32_4x4x1f32(wA[3], 1.0f, (f32x4){0.0f, 0.0f, 0.0f, 0.0f}, 4, 12 + hq, 0);
            });
            static_for<15>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                static_for<4>([&](auto hc) {
                    constexpr int hq = decltype(hc)::value;
                    constexpr int cb = 4 * i + hq;
                    hq4[hq] = __builtin_amdgcn_mfma_f32_4x4x1f32(wA[cb / 16], x[i], hq4[hq], 4, cb % 16, 0);
                });
            });
#pragma unroll
            for (int o = 0; o < 16; ++o) h[o] = fmaxf(hq4[o >> 2][o & 3], 0.0f);
        }
        float gh[16];
        if constexpr ((SB_LAB & 4) != 0) {
#pragma unroll
            for (int o = 0; o < 16; ++o) gh[o] = g[o & 7];
        } else {
            f32x4 ghq[4];
            static_for<4>([&](auto oc) {
                constexpr int oq = decltype(oc)::value;
                ghq[oq] = __builtin_amdgcn_mfma_f32_4x4x1f32(wG[0], g[0], (f32x4){0.0f, 0.0f, 0.0f, 0.0f}, 4, oq, 0);
            });
            static_for<7>([&](auto ic) {
                constexpr int i = decltype(ic)::value + 1;
                static_for<4>([&](auto oc) {
                    constexpr int oq = decltype(oc)::value;
                    constexpr int cb = 4 * i + oq;
                    ghq[oq] = __builtin_amdgcn_mfma_f32_4x4x1f32(wG[cb / 16], g[i], ghq[oq], 4, cb % 16, 0);
                });
            });
#pragma unroll
            for (int o = 0; o < 16; ++o) gh[o] = ghq[o >> 2][o & 3];
        }
        float* Tr = T + lane * SB_LD;
        if constexpr ((SB_LAB & 2) == 0) {
#pragma unroll
        for (int o = 0; o < 16; ++o) Tr[o] = (live && h[o] > 0.0f) ? gh[o] : 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) Tr[16 + i] = live ? x[i] : 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) Tr[32 + j] = live ? g[j] : 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) Tr[40 + i] = live ? h[i] : 0.0f;
        } else {
            float t = 0.0f;
#pragma unroll
            for (int o = 0; o < 16; ++o) t += gh[o] + h[o] + x[o];
            bs[0] += t;
        }
        if (live) {
#pragma unroll
            for (int j = 0; j < 8; ++j) bs[j] += g[j];
        }
        // wave-private tile: LDS operations of a wave execute in order, no barrier.  (Round 6 lab, profiles/r06_sce_lab.txt: the tile
        // transposed so that an operand is four 16-byte reads instead of sixteen 4-byte ones - same time, other summation order: not kept.)
        if constexpr ((SB_LAB & 1) == 0)
#pragma unroll 4
        for (int s4 = 0; s4 < 16; ++s4) {
            const float* Tq = T + (4 * s4 + rr) * SB_LD;
            const float a1 = Tq[mm], b1v = Tq[16 + mm];
            const float a2 = (mm < 8) ? Tq[32 + mm] : 0.0f, b2v = Tq[40 + mm];
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1v, acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, b2v, acc2, 0, 0, 0);
        }
        if constexpr ((SB_LAB & 8) != 0) break;
    }
    // fold the 4 waves in wave order, then one partial per destination element (C/D map: row = (lane >> 4) * 4 + reg, col = lane & 15)
    float* mine = sfold + lane * 9;
    for (int w = 0; w < SB_WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                mine[j] = (w == 0) ? acc1[j] : mine[j] + acc1[j];
                mine[4 + j] = (w == 0) ? acc2[j] : mine[4 + j] + acc2[j];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int dd = 32; dd > 0; dd >>= 1) bs[j] += __shfl_xor(bs[j], dd, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) sb2[wave * 8 + j] = bs[j];
    }
    __syncthreads();
    if (wave == 0) {
        float* dst = big + (int64_t)sb * block_stride;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = rr * 4 + j;
            if (mm < 15) dst[a.w1[s] + m * 15 + mm] = mine[j];
            else dst[a.b1[s] + m] = mine[j];
            if (m < 8) dst[a.w2[s] + m * 16 + mm] = mine[4 + j];
        }
        if (lane < 8) {
            float t = sb2[lane];
#pragma unroll
            for (int w = 1; w < SB_WAVES; ++w) t += sb2[8 * w + lane];
            dst[a.b2[s] + lane] = t;
        }
    }
}

// dst (+)= src over n floats
__global__ __launch_bounds__(LINR_BLOCK) void axpy_k(const float* __restrict__ src, int64_t n, float* __restrict__ dst,
                                                     int accumulate) {
    const int64_t i = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (i < n) dst[i] = accumulate ? dst[i] + src[i] : src[i];
}

extern "C" int linr_axpy(const float* src, int64_t n, float* dst, int32_t accumulate, void* stream) {
    if (n < 0) return LINR_EINVAL;
    if (n == 0) return 0;
    if (!src || !dst) return LINR_EINVAL;
    axpy_k<<<linr_grid(n, LINR_BLOCK), LINR_BLOCK, 0, (hipStream_t)stream>>>(src, n, dst, accumulate ? 1 : 0);
    return linr_launch_rc();
}

// gemb[i] = sum_m gb1[m] * W1[m][i]   (scale-embedding gradient through Linear(15,16); the embedding row is a
// constant input of every row of its scale, so its gradient is W1[:, :8]^T applied to the bias gradient)
struct EmbArgs { int64_t gb1[MAX_SCALES], w1[MAX_SCALES], gemb[MAX_SCALES]; };
__global__ void sce_emb_grad_all_k(const float* __restrict__ P, float* __restrict__ gsum, EmbArgs a) {
    const int t = threadIdx.x, g = blockIdx.x;
    if (t < 8) {
        const float* gb1 = gsum + a.gb1[g];
        const float* W1 = P + a.w1[g];
        float s = 0.0f;
        for (int m = 0; m < 16; ++m) s = fmaf(gb1[m], W1[m * 15 + t], s);
        gsum[a.gemb[g] + t] = s;
    }
}

// gsum[p] = sum_b big[b][p] in a fixed association (RED_SPLIT threads per parameter, each 8 interleaved partial sums over
// its quarter of the slab rows in ascending order, quarters added in order) => bit-reproducible.  One thread per
// parameter alone would be 214 blocks of latency-bound streaming on 256 CUs.
#define RED_SPLIT 4       // threads per parameter: each sums nblocks / RED_SPLIT slab rows
// Parameters nobody wrote partials for - the scale embedding (its gradient is derived from the reduced sums afterwards) and
// the context MLPs of scales the frame does not contain - lie in [0, prefix): `zr` lists those ranges and the reduction
// writes 0 for them WITHOUT reading the slab, which therefore needs no clearing pass (a 2-D memset of nb rows per step).
struct ZeroRanges { int n; int64_t prefix; int64_t b[MAX_SCALES + 1], e[MAX_SCALES + 1]; };
// Parameter ranges whose producer (a fused backward launch: one round of long-lived blocks, csrc/fused_bwd.hip) wrote only the
// first rows[i] rows of the slab: the reduction stops there instead of having the producer fill the other rows with zeros.
#define MAX_SHORT 48
struct ShortRanges { int n; int64_t b[MAX_SHORT], e[MAX_SHORT]; int rows[MAX_SHORT]; };
__global__ __launch_bounds__(LINR_BLOCK) void wgrad_reduce_k(const float* __restrict__ big, int nblocks, int64_t total,
                                                             float* __restrict__ gsum, ZeroRanges zr, ShortRanges sr) {
    __shared__ float part[RED_SPLIT][LINR_BLOCK / RED_SPLIT];
    const int lp = threadIdx.x % (LINR_BLOCK / RED_SPLIT), q = threadIdx.x / (LINR_BLOCK / RED_SPLIT);
    const int64_t p = (int64_t)blockIdx.x * (LINR_BLOCK / RED_SPLIT) + lp;
    float s = 0.0f;
    bool skip = false;
    if (p < zr.prefix)
        for (int i = 0; i < zr.n; ++i) skip = skip || (p >= zr.b[i] && p < zr.e[i]);
    if (p < total && !skip) {
        float a[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = 0.0f;
        const int per = nblocks / RED_SPLIT;                 // nblocks is a multiple of 8 * RED_SPLIT
        int rows = nblocks;
        for (int i = 0; i < sr.n; ++i)
            if (p >= sr.b[i] && p < sr.e[i]) rows = sr.rows[i];
        const int hi = (q + 1) * per < rows ? (q + 1) * per : rows;
        if (per == 64) {
            // the usual slab (256 rows): the thread's 64 loads are all in flight before the first add (the rolled loop waits
            // for memory eight times); same adds in the same order
            const float* src = big + (int64_t)(q * 64) * total + p;
            float v[64];
#pragma unroll
            for (int j = 0; j < 64; ++j) v[j] = (q * 64 + j < hi) ? src[(int64_t)j * total] : 0.0f;
#pragma unroll
            for (int j = 0; j < 64; ++j)
                if (q * 64 + j < hi) a[j & 7] += v[j];
        } else {
            for (int b = q * per; b < hi; b += 8) {
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (b + i < hi) a[i] += big[(int64_t)(b + i) * total + p];
            }
        }
        s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    }
    part[q][lp] = s;
    __syncthreads();
    if (q == 0 && p < total) gsum[p] = ((part[0][lp] + part[1][lp]) + part[2][lp]) + part[3][lp];
}

extern "C" int linr_sce_bwd(const float* params, const linr_frame* f, const float* gx0, const float* hid, float* ghid,
                            void* stream) {
    Layout L;
    TRY(linr_frame_layout(f, 0, L));
    if (f->rows == 0) return 0;
    if (!params || !gx0 || !hid || !ghid) return LINR_EINVAL;
    if (!linr_aligned16(gx0) || !linr_aligned16(hid) || !linr_aligned16(ghid)) return LINR_EALIGN;
    const SceArgs sa = sce_args(f, L);
    sce_bwd_k<<<sa.blk_off[sa.n_scales], LINR_BLOCK, 0, (hipStream_t)stream>>>(params, sa, f->rows, gx0, hid, ghid);
    return linr_launch_rc();
}

// What the scale context's backward needs per frame, for linr_sce_bwd_params and linr_bwd_tail_launch alike: sa with the slab rows of
// every scale (wg_off: one workgroup per 256 rows, at most nb; a scale with fewer leaves a short range, appended to sr), the ranges
// the reduction writes zeros for (zr: the scale embedding and the context MLPs of absent scales get no partials) and the
// embedding-gradient table of the ns row ranges that have rows.  sr starts with the caller's ranges sh[0 .. nsh) that hold fewer than
// nb rows.  false: two of the frame's row ranges belong to one scale.
struct SceBwdPlan { SceArgs sa; ZeroRanges zr; ShortRanges sr; EmbArgs ea; int ns; };
static void short_push(ShortRanges& sr, int64_t b, int64_t e, int rows) {
    if (sr.n >= MAX_SHORT) abort();          // cannot happen (struct Ctx: 41); a silent drop would read unwritten rows
    sr.b[sr.n] = b; sr.e[sr.n] = e; sr.rows[sr.n] = rows; ++sr.n;
}
static bool sce_bwd_plan(const linr_frame* f, const Layout& L, int nb, const LinrShortRange* sh, int nsh, SceBwdPlan& p) {
    p.sr.n = 0;
    for (int i = 0; i < nsh; ++i)
        if (sh[i].rows < nb) short_push(p.sr, sh[i].b, sh[i].e, sh[i].rows);
    const int64_t total = L.block_in.a_w;                 // the scale context's parameters lead the layout
    p.sa = sce_args(f, L);
    p.zr.n = 0; p.zr.prefix = total;
    p.zr.b[p.zr.n] = L.emb; p.zr.e[p.zr.n] = L.emb + (int64_t)L.S * 8; ++p.zr.n;
    p.ns = 0;
    bool present[MAX_SCALES] = {}, distinct = true;
    p.sa.wg_off[0] = 0;
    for (int j = 0; j < f->n_scales; ++j) {
        const int64_t nj = f->row_off_h[j + 1] - f->row_off_h[j];
        int64_t wg = nj > 0 ? (nj + LINR_BLOCK - 1) / LINR_BLOCK : 0;
        if (wg > nb) wg = nb;
        p.sa.wg_off[j + 1] = p.sa.wg_off[j] + (int)wg;
        if (wg == 0) continue;
        const int si = f->scale_idx_h[j];
        if (present[si]) distinct = false;
        present[si] = true;
        if (wg < nb) short_push(p.sr, L.m0_w[si], L.m2_b[si] + 8, (int)wg);
        p.ea.gb1[p.ns] = L.m0_b[si]; p.ea.w1[p.ns] = L.m0_w[si]; p.ea.gemb[p.ns] = L.emb + si * 8; ++p.ns;
    }
    for (int si = 0; si < L.S; ++si)
        if (!present[si]) {
            p.zr.b[p.zr.n] = L.m0_w[si];
            p.zr.e[p.zr.n] = si + 1 < L.S ? L.m0_w[si + 1] : total;
            ++p.zr.n;
        }
    return distinct;
}

// The whole backward of the scale context as one call (what linr_net_backward launches for it): the gradients of scale_emb and of
// every scale MLP of the frame into grads[0 .. linr_sce_param_count) - the scale context's parameters lead the flat layout whatever
// the width of the rest of the network - from gx0 [rows][8] and the hid [rows][16] that linr_sce_fwd kept.  The MLPs of scales the
// frame does not contain and their embedding rows get zeros.  slab: linr_sce_bwd_params_slab_bytes(model_scale_num) bytes.
#define SCE_SLAB_ROWS 256
extern "C" int64_t linr_sce_param_count(int32_t model_scale_num) {
    Layout L;
    return make_layout(L, model_scale_num, 1) ? L.block_in.a_w : (int64_t)LINR_EINVAL;
}
extern "C" size_t linr_sce_bwd_params_slab_bytes(int32_t model_scale_num) {
    const int64_t t = linr_sce_param_count(model_scale_num);
    return t > 0 ? (size_t)SCE_SLAB_ROWS * (size_t)t * sizeof(float) : 0;
}
extern "C" int linr_sce_bwd_params(const float* params, const linr_frame* f, const float* gx0, const float* hid, float* slab,
                                   size_t slab_bytes, float* grads, void* stream) {
    Layout L;
    TRY(linr_frame_layout(f, 0, L));
    if (!params || !gx0 || !hid || !slab || !grads) return LINR_EINVAL;
    if (f->rows > 0 && !f->offset_feat) return LINR_EINVAL;
    if (!linr_aligned16(gx0) || !linr_aligned16(hid)) return LINR_EALIGN;
    const int64_t total = L.block_in.a_w;
    if (slab_bytes < (size_t)SCE_SLAB_ROWS * (size_t)total * sizeof(float)) return LINR_ENOSPC;
    hipStream_t s = (hipStream_t)stream;
    const int nb = SCE_SLAB_ROWS;
    SceBwdPlan pl;
    if (!sce_bwd_plan(f, L, nb, nullptr, 0, pl)) return LINR_EINVAL;      // two row ranges of one scale would share slab rows
    if (pl.ns > 0) sce_bwd_all_k<<<pl.sa.wg_off[f->n_scales], SB_WAVES * 64, 0, s>>>(params, f->offset_feat, pl.sa, gx0, hid, slab, total);
    wgrad_reduce_k<<<linr_grid(total, LINR_BLOCK / RED_SPLIT), LINR_BLOCK, 0, s>>>(slab, nb, total, grads, pl.zr, pl.sr);
    if (pl.ns > 0) sce_emb_grad_all_k<<<pl.ns, LINR_WAVE, 0, s>>>(params, grads, pl.ea);
    return linr_launch_rc();
}

// fixed-order sum of the [nblocks][total] partial slab (shared with the op-level entries of csrc/fused.hip)
int linr_slab_reduce_launch(const float* big, int nblocks, int64_t total, float* gsum, hipStream_t s) {
    if (total <= 0) return 0;
    ZeroRanges zr;
    zr.n = 0; zr.prefix = 0;
    ShortRanges sr;
    sr.n = 0;
    wgrad_reduce_k<<<linr_grid(total, LINR_BLOCK / RED_SPLIT), LINR_BLOCK, 0, s>>>(big, nblocks, total, gsum, zr, sr);
    return linr_launch_rc();
}

// The tail of every backward pass (fp32 executor: csrc/net.hip, backward_core; bf16 training executor: csrc/train_bf16.hip): the scale
// context's backward from gx0 [rows][8] fp32 and the hid [rows][16] of its forward (NULL: recomputed) (ghid and all four parameter gradients of every
// scale's context MLP in one launch), the fixed-order reduction of the [nb][total] slab `big` into gsum - `sh` lists the parameter
// ranges whose producers wrote fewer than nb slab rows - and the scale-embedding gradients derived from the reduced sums.
int linr_bwd_tail_launch(const linr_frame* f, const Layout& L, const float* P, const float* gx0, const float* hid, float* big,
                         float* gsum, int nb, const LinrShortRange* sh, int nsh, hipStream_t stream) {
    SceBwdPlan pl;
    (void)sce_bwd_plan(f, L, nb, sh, nsh, pl);
    if (pl.ns >= 1) {          // ghid and all four parameter gradients of every scale's context MLP in one launch
        ProfScope ps(stream, PK_SCE, 1);
        sce_bwd_all_k<<<pl.sa.wg_off[f->n_scales], SB_WAVES * 64, 0, stream>>>(P, f->offset_feat, pl.sa, gx0, hid, big, L.total);
    }
    // one pass sums every parameter's per-block partials in fixed order
    ProfScope ps_tail(stream, PK_MISC, 0);
    wgrad_reduce_k<<<linr_grid(L.total, LINR_BLOCK / RED_SPLIT), LINR_BLOCK, 0, stream>>>(big, nb, L.total, gsum, pl.zr, pl.sr);
    if (pl.ns > 0) sce_emb_grad_all_k<<<pl.ns, LINR_WAVE, 0, stream>>>(P, gsum, pl.ea);
    return linr_launch_rc();
}

// torch.optim.Adam's step over the flat parameter buffer of `total` floats with the per-scale step counters of the scale-context MLPs,
// which lead the flat order at every width (shared with csrc/train_bf16.hip and csrc/wide_train.hip): bias corrections in double, like
// torch.optim.Adam's Python scalars
int linr_adam_step_launch(const Layout& L, int64_t total, float* params, const float* gsum, const linr_step_args& a, hipStream_t s) {
    const int64_t* scale_steps_h = a.scale_steps_h;
    LinrAdamRanges rg;
    rg.count = 0; rg.begin = L.m0_w[0]; rg.len = L.S > 1 ? L.m0_w[1] - L.m0_w[0] : L.block_in.a_w - L.m0_w[0];
    if (scale_steps_h) {
        rg.count = L.S;
        // scale_steps_h[s] = updates applied to the context MLP of scale s INCLUDING this one; 0 = it has never had a gradient and
        // is skipped (torch.optim.Adam skips .grad None; torch 1.13's zero_grad() leaves zeros afterwards, so a started scale is
        // updated on every step - with the zero gradient the reduction writes for a scale this frame lacks)
        for (int sc = 0; sc < L.S; ++sc) {
            const int64_t t = scale_steps_h[sc];
            rg.active[sc] = t >= 1 ? 1 : 0;
            rg.step_size[sc] = t >= 1 ? (float)(a.lr / (1.0 - pow(a.beta1, (double)t))) : 0.0f;
            rg.bc2_sqrt[sc] = t >= 1 ? (float)sqrt(1.0 - pow(a.beta2, (double)t)) : 1.0f;
        }
    }
    return linr_adam_launch(params, gsum, a.exp_avg, a.exp_avg_sq, total, a.lr / (1.0 - pow(a.beta1, (double)a.step)),
                            sqrt(1.0 - pow(a.beta2, (double)a.step)), a.beta1, a.beta2, a.eps, a.weight_decay,
                            scale_steps_h ? &rg : nullptr, s);
}
