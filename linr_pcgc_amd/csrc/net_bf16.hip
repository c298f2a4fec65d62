// bf16 / uint8-weight inference executor (BASELINE config[4]: "bf16 SparseConv + int8 weight pack").
//
// The codec never runs the trained fp32 weights: encoder.py:101-103 codes the geometry with the DE-QUANTISED model
// (Model_Estimate.compress_model -> new_model), i.e. with w = q / 255 * (max - min) + min for the uint8 codes q of
// quant_uniform2 (model_compression/model_size_est.py:72-91) - exactly what the decoder rebuilds from model.bin.  This
// executor takes those codes as the model: 54,712 bytes instead of 219 KB, de-quantised inside the kernels.
//   * feature matrices are bf16 [1 + rows][8] (16 B per row: half the gather bytes of the fp32 path, one dwordx4 per tap),
//     accumulation is fp32;
//   * every 3x3x3 convolution runs on v_mfma_f32_4x4x4_16b_bf16 with CBSZ = 4: the A operand (a 4 cout x 4 cin weight block,
//     de-quantised from the uint8 codes and rounded to bf16 once per kernel, register-resident) is broadcast from block ABID
//     to all 16 blocks, B = four input channels of the lane's gathered row, D = four output channels of the lane's row:
//     64 rows x 4 cout x 4 cin per instruction - a quarter of the fp32 path's MFMAs;
//   * biases, the pointwise convolutions (conv1_0, conv1_2), the scale-context MLP and the head MLP stay fp32 VALU math on
//     the de-quantised fp32 parameters (one tiny prologue kernel writes them to the arena);
//   * inference only (encode / decode / codec): no activations are kept for a backward pass.
// Encoder (all 8 stages, grouped launches) and decoder (stage by stage) run the same kernels with the same per-row
// instruction sequence, so their probabilities are bit-identical and the 16-bit CDF quantisation cannot diverge.
#include "bf16_common.h"
#include "prof.h"
#include <stdlib.h>

#define TRY(e) do { int rc_ = (e); if (rc_) return rc_; } while (0)

// (the scale context sce_bf16_k lives in bf16_common.h: the wide bf16 executor, csrc/wide_bf16.hip, runs it too)

// ---- arena --------------------------------------------------------------------------------------------------------------------
struct BArena {
    int64_t rows;
    char* base;
    int64_t cur;                     // bytes
    float* PF;                       // [n_params] de-quantised fp32 parameters
    double* part;                    // [8 * grid] block partials of the bits
    bf16_t *X0, *OCC, *A[8], *H[8], *I[8], *O[8], *Hx[MAX_BL - 1], *Ix[MAX_BL - 1];
    BPads pads;
    bf16_t* mats;                    // start of the bf16 matrices (pad offsets are relative to it)
};

static bf16_t* bmat(BArena& a) {
    bf16_t* p = a.base ? reinterpret_cast<bf16_t*>(a.base + a.cur) : nullptr;
    if (a.pads.n >= BPADS_MAX) abort();
    a.pads.off[a.pads.n] = (a.cur - (int64_t)(reinterpret_cast<char*>(a.mats) - a.base)) / 2;
    a.pads.w[a.pads.n++] = 8;
    a.cur += (a.rows + 1) * 16;
    return p ? p + 8 : nullptr;
}

static void make_barena(BArena& a, int64_t rows, char* base, int64_t n_params, int block_layers) {
    a.rows = rows; a.base = base; a.cur = 0; a.pads.n = 0;
    a.PF = reinterpret_cast<float*>(base);
    a.cur += ((n_params * 4 + 63) / 64) * 64;
    a.part = reinterpret_cast<double*>(base + a.cur);
    a.cur += (((int64_t)8 * linr_grid(rows, LINR_BLOCK) * 8 + 63) / 64) * 64;
    a.mats = reinterpret_cast<bf16_t*>(base + a.cur);
    a.X0 = bmat(a); a.OCC = bmat(a);
    for (int b = 0; b < 8; ++b) { a.A[b] = bmat(a); a.H[b] = bmat(a); a.I[b] = bmat(a); a.O[b] = bmat(a); }
    for (int l = 0; l + 1 < MAX_BL; ++l) {
        a.Hx[l] = a.Ix[l] = nullptr;
        if (l + 1 < block_layers) { a.Hx[l] = bmat(a); a.Ix[l] = bmat(a); }
    }
}

extern "C" size_t linr_net_bf16_arena_bytes(int64_t rows, int32_t block_layers) {
    if (rows < 0) return 0;
    if (block_layers < 1) block_layers = 1;
    if (block_layers > MAX_BL) return 0;
    Layout L;
    make_layout(L, MAX_SCALES, block_layers);
    BArena a;
    make_barena(a, rows, nullptr, L.total, block_layers);
    return (size_t)a.cur + 64;
}

// ---- executor ------------------------------------------------------------------------------------------------------------------
struct BCtx {
    const linr_frame* f;
    Layout L;
    BArena A;
    const uint8_t* codes;
    float minv, range;
    hipStream_t s;
    int64_t R;
};

static BArgs base_args(const BCtx& c) {
    BArgs a = BArgs();
    a.lo = c.f->nbr_lo; a.mask = c.f->nbr_mask; a.ld = c.f->nbr_ld; a.n = c.R;
    a.codes = c.codes; a.minv = c.minv; a.range = c.range; a.pf = c.A.PF;
    return a;
}

// the one launch of bconv_k<G::MODE>: g[0 .. ng) are the groups (bf16_common.h), x what bfill takes per launch
template <class G, class... X>
static int blaunch(const BCtx& c, const G* g, int ng, X... x) {
    BArgs a = base_args(c);
    TRY(bfill(a, g, ng, x...));
    linr_poison_hook(c.s, PK_BF16_INFER);
    bconv_k<G::MODE><<<dim3(linr_grid(c.R, LINR_BLOCK), ng), LINR_BLOCK, 0, c.s>>>(a);
    return linr_launch_rc();
}

__global__ __launch_bounds__(LINR_BLOCK) void badd_rows_k(const bf16_t* __restrict__ src, int64_t n, bf16_t* __restrict__ dst) {
    const int64_t r = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (r >= n) return;
    float a[8], b[8];
    unpack_row(*reinterpret_cast<const uint4*>(src + r * 8), a);
    unpack_row(*reinterpret_cast<const uint4*>(dst + r * 8), b);
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] += a[j];
    *reinterpret_cast<uint4*>(dst + r * 8) = pack_row(b);
}

// make_block for one block slot (upsample.py:88-97), single launch group
static int bblock(const BCtx& c, const BlockP& bp, const bf16_t* in, int slot, const bf16_t* res) {
    const BArena& a = c.A;
    const BConvGroup first = {in, a.A[slot], nullptr, bp.a_w, bp.a_b, bp.cin};
    TRY(blaunch(c, &first, 1, 1));
    const bf16_t* X = a.A[slot];
    bf16_t* Il = nullptr;
    for (int l = 0; l < bp.nl; ++l) {          // one Inception layer: X -> H -> I (two launches)
        bf16_t* H = l == 0 ? a.H[slot] : a.Hx[l - 1];
        bf16_t* I = l == 0 ? a.I[slot] : a.Ix[l - 1];
        const BPwGroup pw = bpw_group(bp.inc[l], X, H);
        TRY(blaunch(c, &pw, 1));
        const BDualGroup du = bdual_group(bp.inc[l], H, X, I, nullptr);
        TRY(blaunch(c, &du, 1));
        X = I; Il = I;
    }
    if (bp.nl > 1) badd_rows_k<<<linr_grid(c.R, LINR_BLOCK), LINR_BLOCK, 0, c.s>>>(a.A[slot], c.R, Il);     // resnet.py:160-161
    const BConvGroup last = {Il, a.O[slot], res, bp.b_w, bp.b_b, 8};
    return blaunch(c, &last, 1, 0);
}

static int bheads(const BCtx& c, int k0, int k1, float* probs_stage_major, double* part) {
    BHeadGroup h[8];
    for (int k = k0; k < k1; ++k) h[k - k0] = bhead_group(c.L, k, c.A.O[k], nullptr);
    return blaunch(c, h, k1 - k0, part ? c.f->occ : nullptr, probs_stage_major, part);
}

extern "C" int linr_net_forward_bf16(const linr_frame* f, const uint8_t* codes, float min_param, float max_param, void* arena,
                                     size_t arena_bytes, int32_t stage_begin, int32_t stage_end, float* probs, double* bits_acc,
                                     void* stream) {
    if (!codes || !arena || !probs) return LINR_EINVAL;
    BCtx c;
    TRY(linr_frame_layout(f, 0, c.L));
    if (stage_begin < 0 || stage_end > 8 || stage_begin >= stage_end) return LINR_EINVAL;
    if (f->rows == 0) return 0;
    if (!f->nbr_lo || !f->nbr_mask || !f->offset_feat || !f->occ || f->nbr_ld < f->rows) return LINR_EINVAL;   // compressed map only
    if (!linr_rows_fit32(f->rows)) return LINR_EINVAL;
    if (arena_bytes < linr_net_bf16_arena_bytes(f->rows, c.L.BL)) return LINR_ENOSPC;
    if (((uintptr_t)arena) & 63u) return LINR_EALIGN;
    c.f = f; c.codes = codes; c.minv = min_param; c.range = max_param - min_param;      // fp32 subtraction, like ten_range
    c.s = (hipStream_t)stream; c.R = f->rows;
    make_barena(c.A, f->rows, (char*)arena, c.L.total, c.L.BL);
    const BArena& a = c.A;
    const Layout& L = c.L;
    occ_bf16_k<<<linr_grid(c.R, LINR_BLOCK), LINR_BLOCK, 0, c.s>>>(f->occ, c.R, a.OCC);
    if (stage_begin == 0) {
        dequant_all_k<<<linr_grid(L.total, LINR_BLOCK), LINR_BLOCK, 0, c.s>>>(codes, L.total, c.range, c.minv, a.PF);
        zero_pads16_k<<<a.pads.n, 64, 0, c.s>>>(a.mats, a.pads);
        BSce sa;
        linr_sce_table(f, L, sa);
        linr_poison_hook(c.s, PK_BF16_INFER);
        sce_bf16_k<<<linr_grid(c.R, LINR_BLOCK), LINR_BLOCK, 0, c.s>>>(a.PF, f->offset_feat, sa, c.R, a.X0);
        TRY(bblock(c, L.block_in, a.X0, 0, nullptr));                                   // O[0] = x_glob
    }
    double* part = bits_acc ? a.part : nullptr;
    const int64_t nblk = linr_grid(c.R, LINR_BLOCK);
    if (stage_begin == 0 && stage_end == 8) {
        // teacher-forced: the 7 outter blocks and the 8 heads as grouped launches (same kernels, same per-row arithmetic as
        // the staged path below)
        BConvGroup first[7], last[7];
        BPwGroup pw[7];
        BDualGroup du[7];
        for (int g = 0; g < 7; ++g) {
            const BlockP& bp = L.outter[g];
            const int s = g + 1;
            first[g] = {a.OCC, a.A[s], nullptr, bp.a_w, bp.a_b, bp.cin};
            pw[g] = bpw_group(bp.inc[0], a.A[s], a.H[s]);
            du[g] = bdual_group(bp.inc[0], a.H[s], a.A[s], a.I[s], nullptr);
            last[g] = {a.I[s], a.O[s], a.O[0], bp.b_w, bp.b_b, 8};
        }
        TRY(blaunch(c, first, 7, 1));
        TRY(blaunch(c, pw, 7));
        TRY(blaunch(c, du, 7));
        TRY(blaunch(c, last, 7, 0));
        TRY(bheads(c, 0, 8, probs, part));
    } else {
        for (int k = stage_begin; k < stage_end; ++k) {
            if (k > 0) TRY(bblock(c, L.outter[k - 1], a.OCC, k, a.O[0]));
            TRY(bheads(c, k, k + 1, probs, part));
        }
    }
    if (bits_acc)
        TRY(linr_bits_finish_launch(a.part + (int64_t)stage_begin * nblk, (int)((stage_end - stage_begin) * nblk), bits_acc, c.s));
    return linr_launch_rc();
}
