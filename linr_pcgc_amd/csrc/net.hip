// Whole-network fp32 executor: scale-context MLP -> block_in -> 8 x (prune conv + head MLP + sigmoid/BCE, outter block)
// forward, and the hand-derived backward, as one stream-ordered launch sequence over a flat parameter buffer and a
// caller-owned activation arena.  Replaces LINR_PCGC_Model.logic_core/forward (models/model_core.py:38-81),
// CNP.forward (models/upsample.py:163-217), make_block (:88-97), InceptionResNet.forward (models/resnet.py:55-60)
// and the autograd graph main.py:315-316 differentiates.
//
// Arena: every activation / gradient matrix is [1 + rows][ld] with an all-zero row in FRONT (row index -1), so the
// sparse convolutions read absent neighbours from it (LINR_PAD_ROW) with no branch.
//
// Here: the parameter count, the arena, the per-frame context, the launch helpers and group builders, the forward and backward
// schedules and the linr_net_* entries.  The kernels live in csrc/fused.hip, csrc/fused_bwd.hip, csrc/occ_wgrad.hip, csrc/wgrad.hip,
// csrc/linear.hip and csrc/sce.h; what ends a backward pass (scale-context backward, slab reduction, Adam) in csrc/bwd_tail.hip; the
// timing / poison scope around every launch in csrc/prof.h.  axpy_k went with the tail: the two places here that add matrices (the
// extra skip of a deeper block_in, the gradient accumulation of linr_net_backward) call its entry linr_axpy, i.e. the same launch
// behind that entry's argument checks and launch status.
#include "common.h"
#include "conv_common.h"
#include "layout.h"
#include "sce.h"
#include "bwd_tail.h"
#include "prof.h"
#include "fake_quant.h"
#include <stdlib.h>

#define TRY(e) do { int rc_ = (e); if (rc_) return rc_; } while (0)

// ---- parameter layout (reference parameters() order) ------------------------------------------------------------
extern "C" int linr_abi_version(void) { return LINR_ABI_VERSION; }

extern "C" int64_t linr_param_count(int32_t scale_num, int32_t block_layers) {
    Layout L;
    return make_layout(L, scale_num, block_layers) ? L.total : (int64_t)LINR_EINVAL;
}

// ---- arena ------------------------------------------------------------------------------------------------------
struct Arena {
    int64_t rows;
    float* base;
    int64_t cur;                 // floats
    int64_t pad_off[200];        // float offset of every pad row
    int pad_w[200];
    int npad;
    // forward (saved for backward)
    float *X0, *OCC;
    float *A[8], *H[8], *M[8], *I[8], *O[8];
    float *Hx[MAX_BL - 1], *Mx[MAX_BL - 1], *Ix[MAX_BL - 1];        // Inception layers 1.. of block_in (block_layers > 1)
    float *gIx[MAX_BL - 1], *gMx[MAX_BL - 1], *gHx[MAX_BL - 1];
    float *C[8], *P[8];
    // backward scratch
    float *gXG, *gX0;
    float *gC[8], *gO[8], *gI[8], *gA[8], *gH[8], *gM[8];   // one set per stage / block (the grouped launches need them side by side)
    float* BIG;                  // [LINR_WG_BLOCKS][n_params] per-block partial weight gradients
    float* GSUM;                 // [n_params] their fixed-order sum (the gradient of this backward call)
    int64_t n_params;
    void* slab;
};

static float* arena_mat(Arena& a, int ld) {
    a.cur = (a.cur + 3) & ~(int64_t)3;                       // 16-byte alignment
    a.pad_off[a.npad] = a.cur; a.pad_w[a.npad] = ld; a.npad++;
    float* p = a.base ? a.base + a.cur + ld : nullptr;      // row 0 starts after the pad row
    a.cur += (a.rows + 1) * (int64_t)ld;
    return p;
}

static size_t slab_need(int64_t rows) {          // the 8 heads' per-block bits partials
    return (size_t)8 * linr_grid(rows, LINR_BLOCK) * sizeof(double) + 64;
}

static void make_arena(Arena& a, int64_t rows, float* base, int64_t n_params, int block_layers = 1) {
    a.rows = rows; a.base = base; a.cur = 0; a.npad = 0;
    a.X0 = arena_mat(a, 8); a.OCC = arena_mat(a, 8);
    for (int b = 0; b < 8; ++b) {
        a.A[b] = arena_mat(a, 8); a.H[b] = arena_mat(a, 8); a.M[b] = arena_mat(a, 4);
        a.I[b] = arena_mat(a, 8); a.O[b] = arena_mat(a, 8);
    }
    for (int k = 0; k < 8; ++k) {
        a.C[k] = arena_mat(a, 8); a.P[k] = arena_mat(a, 1);
    }
    a.gXG = arena_mat(a, 8); a.gX0 = arena_mat(a, 8);
    for (int i = 0; i < 8; ++i) {
        a.gC[i] = arena_mat(a, 8); a.gO[i] = arena_mat(a, 8); a.gI[i] = arena_mat(a, 8); a.gA[i] = arena_mat(a, 8);
        a.gH[i] = arena_mat(a, 8); a.gM[i] = arena_mat(a, 4);
    }
    for (int l = 0; l + 1 < MAX_BL; ++l) {
        a.Hx[l] = a.Mx[l] = a.Ix[l] = a.gIx[l] = a.gMx[l] = a.gHx[l] = nullptr;
        if (l + 1 < block_layers) {
            a.Hx[l] = arena_mat(a, 8); a.Mx[l] = arena_mat(a, 4); a.Ix[l] = arena_mat(a, 8);
            a.gIx[l] = arena_mat(a, 8); a.gMx[l] = arena_mat(a, 4); a.gHx[l] = arena_mat(a, 8);
        }
    }
    a.n_params = n_params;
    a.cur = (a.cur + 15) & ~(int64_t)15;
    a.GSUM = base ? base + a.cur : nullptr; a.cur += (n_params + 15) & ~(int64_t)15;
    a.BIG = base ? base + a.cur : nullptr; a.cur += (int64_t)LINR_WG_BLOCKS * n_params;
    a.cur = (a.cur + 15) & ~(int64_t)15;                     // 64-byte alignment for the slab (doubles inside)
    a.slab = base ? (void*)(base + a.cur) : nullptr;
    a.cur += (int64_t)((slab_need(rows) + 3) / 4);
}

extern "C" size_t linr_net_arena_bytes(int64_t rows, int32_t block_layers) {
    if (rows < 0) return 0;
    if (block_layers < 1) block_layers = 1;
    if (block_layers > MAX_BL) return 0;
    Arena a;
    Layout L;
    make_layout(L, MAX_SCALES, block_layers);                 // sized for the largest scale_num: one arena serves any model of this depth
    make_arena(a, rows, nullptr, L.total, block_layers);
    return (size_t)a.cur * sizeof(float) + 64;
}

struct Ctx : LinrShortList {
    const linr_frame* f;
    const float* P;
    Arena A;
    Layout L;
    hipStream_t s;           // the caller's stream
    int64_t R;
    int64_t nbr_ld;
};

// index source of the conv kernels: the compressed map (the full neighbour table is 5 % slower also after the shift
// addressing of round 2: 2.565 vs 2.438 ms/step, profiles/r02_ab_conv_table.txt)
static LinrCmap cmap(const Ctx& c) { return {c.f->nbr_lo, c.f->nbr_mask, c.nbr_ld, c.R}; }

// block_in joins the grouped launches of the outter blocks when it has their shape (one Inception layer)
static bool join_block_in(const Ctx& c) { return c.L.block_in.nl == 1; }

// backward-data and weight gradient of the 8->8 convolutions from ONE gather (csrc/fused_bwd.hip); LINR_FUSED_BWD=0 restores the
// two-kernel schedule (same input gradients bit for bit, weight gradients in another summation order)
static bool fused_bwd(const Ctx& c) {
    static const int v = getenv("LINR_FUSED_BWD") ? atoi(getenv("LINR_FUSED_BWD")) : 1;
    // (the fused kernels have no 64-bit path into the compressed map: larger maps take the two-kernel path)
    return v != 0 && linr_cmap_fits32(c.nbr_ld);
}

static int conv3(Ctx& c, bool bwd, const float* in, int in_ld, const float* W, const float* bias, int cin, int cout,
                 const float* res, int res_ld, const float* act, int act_ld, float* out, int out_ld, unsigned flags) {
    ProfScope ps(c.s, bwd ? PK_BWD_DATA : PK_CONV88, 1);
    const ConvGroup g = {in, W, bias, res, act, out};
    return linr_cconv_launch(bwd, cmap(c), &g, 1, in_ld, cin, cout, res_ld, act_ld, out_ld, flags, c.s);
}

// transposed tiled table of the stand-alone weight-gradient kernels (csrc/wgrad.hip: spconv_wgrad_t_k), or NULL: indices from nbr
static const int32_t* wg_t8t(const Ctx& c) { return c.f->nbr8t; }
static int conv3_wgrad(Ctx& c, const float* in, int in_ld, const float* gout, int gout_ld, int cin, int cout,
                       int64_t w_off, int64_t b_off) {
    ProfScope ps(c.s, PK_WGRAD, 1);
    const WgradGroup g = {in, gout, w_off, b_off, 0};
    return linr_conv3_wgrad_mfma(&g, 1, in_ld, gout_ld, c.f->nbr, c.nbr_ld, c.R, wg_t8t(c), cin, cout, c.A.BIG, c.L.total, c.nb, c.s);
}

static int linear(Ctx& c, const float* in, int in_ld, int64_t n, const float* W, int ws_ci, int ws_co, const float* bias,
                  int cin, int cout, const float* res, int res_ld, const float* act, int act_ld, float* out, int out_ld,
                  unsigned flags) {
    return linr_linear_launch(in, in_ld, n, W, ws_ci, ws_co, bias, cin, cout, res, res_ld, act, act_ld, out, out_ld, flags,
                              c.s);
}

static int linear_wgrad(Ctx& c, const float* in, int in_ld, const float* gout, int gout_ld, int64_t n, int cin, int cout,
                        int64_t w_off, int ws_ci, int ws_co, int64_t b_off) {
    ProfScope ps(c.s, PK_LIN_WGRAD, 1);
    const WgradGroup g = {in, gout, w_off, b_off, 0};
    return linr_linear_wgrad_partial(&g, 1, in_ld, gout_ld, n, cin, cout, c.A.BIG, c.L.total, ws_ci, ws_co, c.nb, c.s);
}

// Per-layer matrices of block slot b (0 = block_in, 1..7 = outter blocks): layer 0 uses the slot's own H/M/I, the extra
// Inception layers of block_in (block_layers > 1, models/resnet.py:156-162) the Hx/Mx/Ix sets.
struct LayerBufs { float *H, *M, *I, *gI, *gM, *gH; };
static LayerBufs layer_bufs(Arena& a, int b, int l) {
    if (l == 0) return {a.H[b], a.M[b], a.I[b], a.gI[b], a.gM[b], a.gH[b]};
    return {a.Hx[l - 1], a.Mx[l - 1], a.Ix[l - 1], a.gIx[l - 1], a.gMx[l - 1], a.gHx[l - 1]};
}

// Block of slot b (layout.h: slot_block), and the launchers' per-group operands (common.h) of its pieces: Inception layer q with input X and matrices t;
// the block's tail conv with output gradient gO behind that layer; head k.  The grouped launches fill one array element per slot
// with these, the staged / per-block paths launch a single one.
static ConvPwGroup pw_fwd_group(const float* P, const IncP& q, const float* X, const LayerBufs& t) {
    return {X, P + q.c00_w, P + q.c00_b, P + q.c10_w, P + q.c10_b, t.H};
}
static Dual44FwdGroup dual_fwd_group(const float* P, const IncP& q, const float* X, const LayerBufs& t) {
    return {t.H, P + q.c01_w, P + q.c01_b, P + q.c11_w, P + q.c11_b, X, P + q.c12_w, P + q.c12_b, t.M, t.I};
}
static Conv88BwdGroup tail_bwd_group(const float* P, const BlockP& bp, const IncP& q, const float* gO, const LayerBufs& t) {
    return {gO, t.I, P + bp.b_w, t.gI, bp.b_w, bp.b_b, P + q.c12_w, t.M, t.gM, q.c12_w, q.c12_b};
}
static Dual44BwdGroup dual_bwd_group(const float* P, const IncP& q, const LayerBufs& t) {
    return {t.gI, t.gM, t.H, P + q.c01_w, P + q.c11_w, t.gH, q.c01_w, q.c01_b, q.c11_w, q.c11_b};
}
static Conv84BwdGroup c00_bwd_group(const float* P, const IncP& q, const float* A, const LayerBufs& t, float* gA) {
    return {t.gH, A, t.gI, P + q.c00_w, P + q.c10_w, gA, q.c00_w, q.c00_b, q.c10_w, q.c10_b};
}
static HeadFwdGroup head_fwd_group(Ctx& c, int k, bool bits) {          // bits: BCE partials into the arena slab, linr_grid(R, 256) per head
    const Arena& a = c.A;
    const Layout& L = c.L;
    double* part = bits ? (double*)a.slab + (int64_t)k * linr_grid(c.R, LINR_BLOCK) : nullptr;
    return {a.O[k], c.P + L.pr_w[k], c.P + L.pr_b[k], a.C[k], c.P + L.h0_w[k], c.P + L.h0_b[k], c.P + L.h2_w[k], c.P + L.h2_b[k],
            a.OCC + k, a.P[k], part};
}
// the two-kernel schedule reads the same operands through the stand-alone launchers
static WgradGroup wgrad_of(const Conv88BwdGroup& g) { return {g.xin, g.g, g.w_off, g.b_off, 0}; }
static ConvGroup bwd_data_of(const Conv88BwdGroup& g) { return {g.g, g.W, nullptr, nullptr, nullptr, g.out}; }

// make_block (models/upsample.py:88-97): conv3(cin->8)+ReLU -> ResNetBlock(nl x Inception, extra skip if nl > 1) ->
// conv3(8->8) (+ res)
static int block_fwd(Ctx& c, const BlockP& bp, const float* in, int in_ld, int b, const float* res) {
    Arena& a = c.A;
    const float* P = c.P;
    TRY(conv3(c, false, in, in_ld, P + bp.a_w, P + bp.a_b, bp.cin, 8, nullptr, 0, nullptr, 0, a.A[b], 8, LINR_RELU));
    const float* X = a.A[b];                          // input of the current Inception layer
    for (int l = 0; l < bp.nl; ++l) {
        const IncP& q = bp.inc[l];
        const LayerBufs t = layer_bufs(a, b, l);
        // Inception layer in two launches (csrc/fused.hip): [conv0_0 | conv1_0 centre tap] -> H, then the two 4->4 convs
        // as one pass with conv1_2 and the residual in the epilogue -> M, I
        const ConvPwGroup g0 = pw_fwd_group(P, q, X, t);
        TRY(linr_conv_pw_fwd_launch(cmap(c), &g0, 1, c.s));
        const Dual44FwdGroup g1 = dual_fwd_group(P, q, X, t);
        TRY(linr_dual44_fwd_launch(cmap(c), &g1, 1, c.s));
        X = t.I;
    }
    float* Il = layer_bufs(a, b, bp.nl - 1).I;
    if (bp.nl > 1)           // ResNetBlock.forward: out += x when it chains more than one layer (resnet.py:160-161)
        TRY(linr_axpy(a.A[b], c.R * 8, Il, 1, c.s));
    TRY(conv3(c, false, Il, 8, P + bp.b_w, P + bp.b_b, 8, 8, res, 8, nullptr, 0, a.O[b], 8, 0));
    return 0;
}

// gO: gradient w.r.t. the block output [R,8].  gin != nullptr: also produce the input gradient (block_in only).
static int block_bwd(Ctx& c, const BlockP& bp, const float* in, int in_ld, int b, const float* gO, float* gin) {
    Arena& a = c.A;
    const float* P = c.P;
    const int nl = bp.nl;
    const LayerBufs last = layer_bufs(a, b, nl - 1);
    // O = conv3(I_last; b)
    TRY(conv3_wgrad(c, last.I, 8, gO, 8, 8, 8, bp.b_w, bp.b_b));
    for (int l = nl - 1; l >= 0; --l) {
        const IncP& q = bp.inc[l];
        const LayerBufs t = layer_bufs(a, b, l);
        const float* X = l == 0 ? a.A[b] : layer_bufs(a, b, l - 1).I;         // the layer's input
        float* gX = l == 0 ? a.gA[b] : layer_bufs(a, b, l - 1).gI;           // where its input gradient goes
        // gI of this layer: from the block's tail conv (last layer) or written by layer l+1 as its input gradient
        // I[:,4:8] = M @ c12 + b12 + X[:,4:8]  =>  gM = (gI[:,4:8] @ W12^T) * (M > 0)
        if (l == nl - 1) {   // gI = bwd(gO; Wb) with gM in the epilogue (csrc/fused.hip)
            const Conv88BwdGroup g = tail_bwd_group(P, bp, q, gO, t);
            TRY(linr_conv_bwd_gm_launch(cmap(c), &g, 1, c.s));
        } else
            TRY(linear(c, t.gI + 4, 8, c.R, P + q.c12_w, 1, 4, nullptr, 4, 4, nullptr, 0, t.M, 4, t.gM, 4, LINR_RELU_MASK));
        TRY(linear_wgrad(c, t.M, 4, t.gI + 4, 8, c.R, 4, 4, q.c12_w, 4, 1, q.c12_b));
        // I[:,0:4] = conv3(H0; c01) + X[:,0:4], M = relu(conv3(H1; c11))
        const Dual44BwdGroup gd = dual_bwd_group(P, q, t);
        TRY(linr_conv3_wgrad_dual44(&gd, 1, 8, 4, c.f->nbr, c.nbr_ld, c.R, wg_t8t(c), a.BIG, c.L.total, c.nb, c.s));
        TRY(linr_dual44_bwd_launch(cmap(c), &gd, 1, c.s));
        // H0 = relu(conv3(X; c00)), H1 = relu(X @ c10)
        TRY(conv3_wgrad(c, X, 8, t.gH, 8, 8, 4, q.c00_w, q.c00_b));
        TRY(linear_wgrad(c, X, 8, t.gH + 4, 8, c.R, 8, 4, q.c10_w, 4, 1, q.c10_b));
        // input gradient: gX = bwd(gH[:,0:4]; W00) + gI (the layer's own residual) + gH[:,4:8] @ W10^T; layer 0's input is
        // A = relu(.) so it is masked by (A > 0), after the ResNetBlock's extra skip (nl > 1: + gI of the last layer)
        const bool skip = (l == 0 && nl > 1);
        if (skip)
            TRY(linr_hip_rc(hipMemcpyAsync(gX, last.gI, (size_t)c.R * 8 * sizeof(float), hipMemcpyDeviceToDevice, c.s)));
        const Conv84BwdGroup ga = c00_bwd_group(P, q, l == 0 ? a.A[b] : nullptr, t, gX);
        TRY(linr_conv_bwd_ga_launch(cmap(c), &ga, 1, (l == 0 ? LINR_RELU_MASK : 0u) | (skip ? LINR_ACCUM : 0u), c.s));
    }
    // A = relu(conv3(in; a))
    TRY(conv3_wgrad(c, in, in_ld, a.gA[b], 8, bp.cin, 8, bp.a_w, bp.a_b));
    if (gin) TRY(conv3(c, true, a.gA[b], 8, P + bp.a_w, nullptr, bp.cin, 8, nullptr, 0, nullptr, 0, gin, 8, 0));
    return 0;
}

static int check_frame(const linr_frame* f, const void* params, const void* arena, size_t arena_bytes, Ctx& c) {
    if (!params || !arena) return LINR_EINVAL;
    TRY(linr_frame_layout(f, 0, c.L));
    if (f->rows > 0 && (!f->nbr || !f->nbr_lo || !f->nbr_mask || !f->offset_feat || !f->occ)) return LINR_EINVAL;
    if (!linr_rows_fit32(f->rows) || f->nbr_ld < f->rows) return LINR_EINVAL;
    if (arena_bytes < linr_net_arena_bytes(f->rows, c.L.BL)) return LINR_ENOSPC;
    if (!linr_aligned16(arena)) return LINR_EALIGN;
    c.f = f;
    c.P = (const float*)params;
    c.R = f->rows;
    c.nbr_ld = f->nbr_ld;
    c.nb = linr_wg_blocks_for(f->rows);
    make_arena(c.A, f->rows, (float*)arena, c.L.total, c.L.BL);
    if (f->flags & LINR_FRAME_OCC_PADDED) {        // the caller's occupancy buffer has the zero row in front: use it in place
        if (!f->occ || !linr_aligned16(f->occ)) return LINR_EINVAL;
        c.A.OCC = const_cast<float*>(f->occ);
    }
    return 0;
}

// Teacher-forced forward of all 8 stages with the 7 outter blocks and the 8 heads as grouped launches (their inputs -
// the ground-truth occupancy and x_glob - are all known up front).  Same kernels and per-row arithmetic as the staged
// path below, so the decoder reproduces these probabilities bit for bit.
static int forward_batched(Ctx& c, float* probs, double* bits_acc) {
    Arena& a = c.A;
    const float* P = c.P;
    const Layout& L = c.L;
    const LinrCmap m = cmap(c);
    const int64_t nblk = linr_grid(c.R, LINR_BLOCK);
    // join: block_in (arena slot 0; its first conv has already run) rides as group 0 of the Inception-layer launches - the
    // eight blocks have the same structure behind their first conv (models/upsample.py:88-97) and do not depend on each
    // other until prior_k = x_glob + outter_k.  g0 = first slot in the grouped launches, ng = their group count; the
    // occupancy conv and the tail conv (which needs x_glob as residual) always cover slots 1..7.
    const bool join = join_block_in(c);
    const int g0 = join ? 0 : 1, ng = 8 - g0;
    {   // first conv of every outter block: A[b] = relu(conv3(occ[:, :b]; a) + a_b), one shared gather (csrc/fused.hip)
        int64_t w_off[7], b_off[7], o_off[7];
        for (int g = 0; g < 7; ++g) { w_off[g] = L.outter[g].a_w; b_off[g] = L.outter[g].a_b; o_off[g] = a.A[g + 1] - a.A[1]; }
        ProfScope ps(c.s, PK_OCC7, 7);
        TRY(linr_occ_conv7_launch(a.OCC, m, P, w_off, b_off, a.A[1], o_off, c.s));
    }
    {   // H = [relu(conv0_0(A)) | relu(conv1_0(A))]
        ConvPwGroup g[8];
        for (int i = 0; i < ng; ++i) g[i] = pw_fwd_group(P, slot_block(L, g0 + i).inc[0], a.A[g0 + i], layer_bufs(a, g0 + i, 0));
        ProfScope ps(c.s, PK_CONVPW_FWD, ng);
        TRY(linr_conv_pw_fwd_launch(m, g, ng, c.s));
    }
    {   // both 4->4 convs + conv1_2 + residual -> M, I
        Dual44FwdGroup g[8];
        for (int i = 0; i < ng; ++i) g[i] = dual_fwd_group(P, slot_block(L, g0 + i).inc[0], a.A[g0 + i], layer_bufs(a, g0 + i, 0));
        ProfScope ps(c.s, PK_DUAL_FWD, ng);
        TRY(linr_dual44_fwd_launch(m, g, ng, c.s));
    }
    if (join)   // x_glob = O[0] = conv3(I[0]; b) of block_in: the one tail conv the others wait for
        TRY(conv3(c, false, a.I[0], 8, P + L.block_in.b_w, P + L.block_in.b_b, 8, 8, nullptr, 0, nullptr, 0, a.O[0], 8, 0));
    {   // O[b] = conv3(I; b) + x_glob
        ConvGroup g[7];
        for (int b = 1; b < 8; ++b) g[b - 1] = {a.I[b], P + L.outter[b - 1].b_w, P + L.outter[b - 1].b_b, a.O[0], nullptr, a.O[b]};
        ProfScope ps(c.s, PK_CONV88, 7);
        TRY(linr_cconv_launch(false, m, g, 7, 8, 8, 8, 8, 0, 8, 0, c.s));
    }
    {   // the 8 occupancy heads
        HeadFwdGroup g[8];
        for (int k = 0; k < 8; ++k) g[k] = head_fwd_group(c, k, bits_acc != nullptr);
        ProfScope ps(c.s, PK_HEAD_FWD, 8);
        TRY(linr_cconv_head_launch(m, g, 8, 8, c.s));
    }
    if (bits_acc) {
        ProfScope ps(c.s, PK_MISC, 0);
        TRY(linr_bits_finish_launch((const double*)a.slab, (int)(8 * nblk), bits_acc, c.s));
    }
    if (probs)
        for (int k = 0; k < 8; ++k)
            TRY(linr_hip_rc(hipMemcpyAsync(probs + (int64_t)k * c.R, a.P[k], (size_t)c.R * sizeof(float), hipMemcpyDeviceToDevice, c.s)));
    return linr_launch_rc();
}

extern "C" int linr_net_forward(const linr_frame* f, const float* params, float* arena, size_t arena_bytes,
                                int32_t stage_begin, int32_t stage_end, float* probs, double* bits_acc, void* stream) {
    Ctx c;
    TRY(check_frame(f, params, arena, arena_bytes, c));
    if (stage_begin < 0 || stage_end > 8 || stage_begin >= stage_end) return LINR_EINVAL;
    c.s = (hipStream_t)stream;
    if (c.R == 0) return 0;
    Arena& a = c.A;
    const float* P = c.P;
    // ground-truth / decoded occupancy (the decoder updates one column per call): gathered in place when the caller's buffer
    // has the zero row in front (check_frame points a.OCC at it), else copied into the padded arena matrix
    if (!(f->flags & LINR_FRAME_OCC_PADDED))
        TRY(linr_hip_rc(hipMemcpyAsync(a.OCC, f->occ, (size_t)c.R * 8 * sizeof(float), hipMemcpyDeviceToDevice, c.s)));
    // all 8 stages: grouped launches (forward_batched); a stage range (the decoder's single stages): stage by stage
    const bool all_stages = stage_begin == 0 && stage_end == 8;
    if (stage_begin == 0) {
        PadList pl;
        pl.n = a.npad;
        for (int i = 0; i < a.npad; ++i) { pl.off[i] = a.pad_off[i]; pl.w[i] = a.pad_w[i]; }
        {   // scale context: one small MLP per scale (model_core.py:48-53), all scales in one launch; its spare blocks clear the pad rows
            ProfScope ps(c.s, PK_SCE, 1);
            const SceArgs sa = sce_args(c.f, c.L);
            sce_fwd_k<float><<<sa.blk_off[sa.n_scales] + (a.npad + LINR_BLOCK / 32 - 1) / (LINR_BLOCK / 32), LINR_BLOCK, 0, c.s>>>(
                P, f->offset_feat, sa, c.R, nullptr, nullptr, a.X0, a.base, pl);      // (no hidden layer kept: sce_bwd_all_k recomputes it)
        }
        if (all_stages && join_block_in(c)) {
            // block_in's first conv only: its Inception layer runs as group 0 of the outter blocks' launches (forward_batched)
            const BlockP& bi = c.L.block_in;
            TRY(conv3(c, false, a.X0, 8, P + bi.a_w, P + bi.a_b, bi.cin, 8, nullptr, 0, nullptr, 0, a.A[0], 8, LINR_RELU));
        } else {
            TRY(block_fwd(c, c.L.block_in, a.X0, 8, 0, nullptr));       // O[0] = x_glob
        }
    }
    if (all_stages) return forward_batched(c, probs, bits_acc);
    const int64_t nblk = linr_grid(c.R, LINR_BLOCK);
    for (int k = stage_begin; k < stage_end; ++k) {
        // prior_k = x_glob + outter_blocks[k-1](occ[:, :k])   (upsample.py:206-214; always the original x_glob)
        if (k > 0) TRY(block_fwd(c, c.L.outter[k - 1], a.OCC, 8, k, a.O[0]));
        // prune conv + MLP + sigmoid + BCE partials in one launch (csrc/fused.hip)
        const HeadFwdGroup g = head_fwd_group(c, k, bits_acc != nullptr);
        TRY(linr_cconv_head_launch(cmap(c), &g, 1, 8, c.s));
        if (probs)
            TRY(linr_hip_rc(hipMemcpyAsync(probs + (int64_t)k * c.R, a.P[k], (size_t)c.R * sizeof(float),
                                           hipMemcpyDeviceToDevice, c.s)));
    }
    if (bits_acc)   // all stages' block partials in one fixed-order pass
        TRY(linr_bits_finish_launch((const double*)a.slab + (int64_t)stage_begin * nblk, (int)((stage_end - stage_begin) * nblk),
                                    bits_acc, c.s));
    return linr_launch_rc();
}

// ---- scale context as stand-alone ops (the launches linr_net_forward / _backward make for it) ---------------------------
extern "C" int linr_sce_fwd(const float* params, const linr_frame* f, float* mix, float* hid, float* x0, void* stream) {
    Layout L;
    TRY(linr_frame_layout(f, 0, L));
    if (f->rows == 0) return 0;
    if (!params || !f->offset_feat || !hid || !x0) return LINR_EINVAL;
    if ((mix && !linr_aligned16(mix)) || !linr_aligned16(hid) || !linr_aligned16(x0)) return LINR_EALIGN;
    const SceArgs sa = sce_args(f, L);
    sce_fwd_k<float><<<sa.blk_off[sa.n_scales], LINR_BLOCK, 0, (hipStream_t)stream>>>(params, f->offset_feat, sa, f->rows, mix, hid, x0, nullptr,
                                                                              PadList{{}, {}, 0});
    return linr_launch_rc();
}

struct Ptr8 { const float* p[8]; };
// dst = ((((((s7 + s6) + s5) + s4) + s3) + s2) + s1) + s0
__global__ __launch_bounds__(LINR_BLOCK) void sum8_k(Ptr8 src, int64_t n, float* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (i >= n) return;
    float t = src.p[7][i];
#pragma unroll
    for (int k = 6; k >= 0; --k) t = t + src.p[k][i];
    dst[i] = t;
}

// Backward of the 8 heads and the 7 outter blocks as grouped launches (one launch per layer, gridDim.y = group).
static int backward_batched(Ctx& c, float gz_scale) {
    Arena& a = c.A;
    const float* P = c.P;
    const Layout& L = c.L;
    const LinrCmap m = cmap(c);
    {
        {   // heads: gC and the four head-parameter gradients
            HeadBwdGroup g[8];
            for (int k = 0; k < 8; ++k)
                g[k] = {a.C[k], a.P[k], a.OCC + k, P + L.h0_w[k], P + L.h0_b[k], P + L.h2_w[k], a.gC[k], L.h0_w[k], L.h0_b[k], L.h2_w[k], L.h2_b[k]};
            ProfScope ps(c.s, PK_HEAD_BWD, 8);
            int hrows = 0;
            TRY(linr_head_bwd_launch(g, 8, 8, gz_scale, c.R, a.BIG, L.total, c.nb, &hrows, c.s));
            c.note_short(L.h0_w[0], L.h2_b[7] + 1, hrows);          // the heads' parameters are one contiguous range
        }
        // C = conv3(prior_k; prune_k)
        Conv88BwdGroup pr[8];
        for (int k = 0; k < 8; ++k) pr[k] = {a.gC[k], a.O[k], P + L.pr_w[k], a.gO[k], L.pr_w[k], L.pr_b[k], nullptr, nullptr, nullptr, 0, 0};
        if (fused_bwd(c)) {   // gO[k] = bwd(gC[k]) and the weight gradients from one gather of gC
            ProfScope ps(c.s, PK_FUSED88, 8);
            int rows = 0;
            TRY(linr_conv88_bwd_wgrad_launch(m, pr, 8, a.BIG, L.total, c.nb, &rows, c.s));
            c.note_short(L.pr_w[0], L.pr_b[7] + 8, rows);
        } else {
        {   // weight gradients ...
            WgradGroup g[8];
            for (int k = 0; k < 8; ++k) g[k] = wgrad_of(pr[k]);
            ProfScope ps(c.s, PK_WGRAD, 8);
            TRY(linr_conv3_wgrad_mfma(g, 8, 8, 8, c.f->nbr, c.nbr_ld, c.R, wg_t8t(c), 8, 8, a.BIG, L.total, c.nb, c.s));
        }
        {   // ... and gO[k] = bwd(gC[k])
            ConvGroup g[8];
            for (int k = 0; k < 8; ++k) g[k] = bwd_data_of(pr[k]);
            ProfScope ps(c.s, PK_BWD_DATA, 8);
            TRY(linr_cconv_launch(true, m, g, 8, 8, 8, 8, 0, 0, 8, 0, c.s));
        }
        }
        Ptr8 src;
        for (int k = 0; k < 8; ++k) src.p[k] = a.gO[k];
        ProfScope ps(c.s, PK_MISC, 0);
        sum8_k<<<linr_grid(c.R * 8, LINR_BLOCK), LINR_BLOCK, 0, c.s>>>(src, c.R * 8, a.gXG);
    }
    // outter blocks 1..7 (slot b = block b; gO[b] is the gradient of the block output) and, with `join`, block_in as slot 0
    // (output gradient gXG = the sum above): one group per slot, g0 = first slot, ng = group count
    const bool join = join_block_in(c);
    const int g0 = join ? 0 : 1, ng = 8 - g0;
    Conv88BwdGroup tail[8];          // O = conv3(I; b) with conv1_2 behind it
    Dual44BwdGroup dual[8];          // conv0_1, conv1_1
    Conv84BwdGroup c00[8];           // conv0_0, conv1_0
    WgradGroup first[8];             // A = relu(conv3(in; a)): the occupancy rows' first b channels (outter block b) or all 8 of x0 (block_in)
    for (int i = 0; i < ng; ++i) {
        const int b = g0 + i;
        const BlockP& bp = slot_block(L, b);
        const LayerBufs t = layer_bufs(a, b, 0);
        tail[i] = tail_bwd_group(P, bp, bp.inc[0], b == 0 ? a.gXG : a.gO[b], t);
        dual[i] = dual_bwd_group(P, bp.inc[0], t);
        c00[i] = c00_bwd_group(P, bp.inc[0], a.A[b], t, a.gA[b]);
        first[i] = {b == 0 ? a.X0 : a.OCC, a.gA[b], bp.a_w, bp.a_b, b == 0 ? 8 : b};
    }
    WgradGroup wg[8];                // operands of the stand-alone weight-gradient launches (two-kernel schedule)
    if (fused_bwd(c)) {   // O = conv3(I; b): gI = bwd(gO; b), gM = (gI[:,4:8] @ W12^T) * (M > 0) and the weight gradient, one gather of gO
        ProfScope ps(c.s, PK_FUSED88, ng);
        int rows = 0;
        TRY(linr_conv88_bwd_wgrad_launch(m, tail, ng, a.BIG, L.total, c.nb, &rows, c.s));
        // everything of a block behind its first conv comes from fused launches over the same groups (conv1_2 rides in this one,
        // conv0_0 / conv0_1 / conv1_0 / conv1_1 come below): one contiguous range of `rows` slab rows per block
        for (int i = 0; i < ng; ++i) c.note_short(c00[i].w00_off, tail[i].b_off + 8, rows);
    } else {
    {   // O = conv3(I; b): weight gradient
        for (int i = 0; i < ng; ++i) wg[i] = wgrad_of(tail[i]);
        ProfScope ps(c.s, PK_WGRAD, ng);
        TRY(linr_conv3_wgrad_mfma(wg, ng, 8, 8, c.f->nbr, c.nbr_ld, c.R, wg_t8t(c), 8, 8, a.BIG, L.total, c.nb, c.s));
    }
    {   // gI = bwd(gO; b), gM = (gI[:,4:8] @ W12^T) * (M > 0)
        ProfScope ps(c.s, PK_BWD_DATA, ng);
        TRY(linr_conv_bwd_gm_launch(m, tail, ng, c.s));
    }
    {   // conv1_2 weight gradient: M^T gI[:,4:8]  (the fused tail-conv launch above produces it on the side)
        for (int i = 0; i < ng; ++i) wg[i] = {tail[i].M, tail[i].out + 4, tail[i].w12_off, tail[i].b12_off, 0};
        ProfScope ps(c.s, PK_LIN_WGRAD, ng);
        TRY(linr_linear_wgrad_partial(wg, ng, 4, 8, c.R, 4, 4, a.BIG, L.total, 4, 1, c.nb, c.s));
    }
    }
    if (fused_bwd(c)) {   // both 4->4 convs: gH and the two kernel / bias gradients from one gather of [gI[:,0:4] | gM]
        ProfScope ps(c.s, PK_FUSED_DUAL, ng);
        int rows_inc = 0;
        TRY(linr_dual44_bwd_wgrad_launch(m, dual, ng, a.BIG, L.total, c.nb, &rows_inc, c.s));
        if (rows_inc != linr_fused_bwd_rows(c.R, c.nb, ng)) return LINR_EINVAL;        // (its parameters were registered with the tail conv)
    } else {   // both 4->4 convs: weight gradients, then gH
        {
            ProfScope ps(c.s, PK_WGRAD, ng);
            TRY(linr_conv3_wgrad_dual44(dual, ng, 8, 4, c.f->nbr, c.nbr_ld, c.R, wg_t8t(c), a.BIG, L.total, c.nb, c.s));
        }
        ProfScope ps(c.s, PK_BWD_DATA, ng);
        TRY(linr_dual44_bwd_launch(m, dual, ng, c.s));
    }
    if (fused_bwd(c)) {   // conv0_0 (8->4): gA = (bwd(gH[:,0:4]; W00) + gI + gH[:,4:8] @ W10^T) * (A > 0) and its weight gradient, one gather
        ProfScope ps(c.s, PK_FUSED_C00, ng);
        int rows_c00 = 0;
        TRY(linr_conv84_bwd_wgrad_launch(m, c00, ng, LINR_RELU_MASK, a.BIG, L.total, c.nb, &rows_c00, c.s));
        if (rows_c00 != linr_fused_bwd_rows(c.R, c.nb, ng)) return LINR_EINVAL;       // (registered with the tail conv)
    } else {
    {   // conv1_0 (1x1 8->4) weight gradient (the fused conv0_0 launch above produces it on the side)
        for (int i = 0; i < ng; ++i) wg[i] = {c00[i].A, c00[i].gH + 4, c00[i].w10_off, c00[i].b10_off, 0};
        ProfScope ps(c.s, PK_LIN_WGRAD, ng);
        TRY(linr_linear_wgrad_partial(wg, ng, 8, 8, c.R, 8, 4, a.BIG, L.total, 4, 1, c.nb, c.s));
    }
    {   // conv0_0 (8->4) weight gradient
        for (int i = 0; i < ng; ++i) wg[i] = {c00[i].A, c00[i].gH, c00[i].w00_off, c00[i].b00_off, 0};
        ProfScope ps(c.s, PK_WGRAD, ng);
        TRY(linr_conv3_wgrad_mfma(wg, ng, 8, 8, c.f->nbr, c.nbr_ld, c.R, wg_t8t(c), 8, 4, a.BIG, L.total, c.nb, c.s));
    }
    {   // gA = (bwd(gH[:,0:4]; W00) + gI + gH[:,4:8] @ W10^T) * (A > 0)
        ProfScope ps(c.s, PK_BWD_DATA, ng);
        TRY(linr_conv_bwd_ga_launch(m, c00, ng, LINR_RELU_MASK, c.s));
    }
    }
    {   // first convs: weight gradient
        // (with the fused backward block_in's first conv - slot 0 - gets its weight gradient from the launch that also produces
        // its input gradient, backward_core; the grouped launch then covers the outter blocks only)
        const int s0 = (join && fused_bwd(c)) ? 1 : 0, nq = ng - s0;
        if (g0 + s0 == 1 && fused_bwd(c)) {
            // the 7 outter blocks read the SAME occupancy rows: all seven weight gradients from one gather (csrc/occ_wgrad.hip)
            const float* gA7[7];
            int64_t w_off[7], b_off[7];
            for (int i = 0; i < 7; ++i) { gA7[i] = first[s0 + i].gout; w_off[i] = first[s0 + i].w_off; b_off[i] = first[s0 + i].b_off; }
            ProfScope ps(c.s, PK_WGRAD, nq);
            int rows = 0;
            TRY(linr_occ_wgrad7_launch(a.OCC, gA7, m, a.BIG, L.total, w_off, b_off, c.nb, c.s, &rows));
            for (int i = 0; i < 7; ++i) c.note_short(w_off[i], b_off[i] + 8, rows);
            return 0;
        }
        ProfScope ps(c.s, PK_WGRAD, nq);
        TRY(linr_conv3_wgrad_mfma(first + s0, nq, 8, 8, c.f->nbr, c.nbr_ld, c.R, wg_t8t(c), 1, 8, a.BIG, L.total, c.nb, c.s));
    }
    return 0;
}

// backward of gscale * bits: leaves the parameter gradient of THIS call in arena GSUM (flat, parameters() order)
static int backward_core(Ctx& c, float gscale) {
    const linr_frame* f = c.f;
    Arena& a = c.A;
    const float* P = c.P;
    const float gz_scale = gscale * 1.4426950408889634f;       // d(bits)/d(nats) = 1/ln 2
    TRY(backward_batched(c, gz_scale));
    const BlockP& bi = c.L.block_in;
    if (join_block_in(c) && fused_bwd(c)) {      // first conv of block_in: input gradient and weight gradient from one gather of gA[0]
        const Conv88BwdGroup g = {a.gA[0], a.X0, P + bi.a_w, a.gX0, bi.a_w, bi.a_b, nullptr, nullptr, nullptr, 0, 0};
        ProfScope ps(c.s, PK_FUSED88, 1);
        int rows = 0;
        TRY(linr_conv88_bwd_wgrad_launch(cmap(c), &g, 1, a.BIG, c.L.total, c.nb, &rows, c.s));
        c.note_short(bi.a_w, bi.a_b + 8, rows);
    } else if (join_block_in(c)) {      // everything but the input gradient of its first conv was part of the grouped launches
        TRY(conv3(c, true, a.gA[0], 8, P + bi.a_w, nullptr, bi.cin, 8, nullptr, 0, nullptr, 0, a.gX0, 8, 0));
    } else {
        TRY(block_bwd(c, bi, a.X0, 8, 0, a.gXG, a.gX0));
    }
    return linr_bwd_tail_launch(f, c.L, P, a.gX0, nullptr, a.BIG, a.GSUM, c.nb, c.shortr.data(), (int)c.shortr.size(), c.s);
}

extern "C" int linr_net_backward(const linr_frame* f, const float* params, float* arena, size_t arena_bytes, float gscale,
                                 float* grads, void* stream) {
    Ctx c;
    TRY(check_frame(f, params, arena, arena_bytes, c));
    if (!grads) return LINR_EINVAL;
    c.s = (hipStream_t)stream;
    if (c.R == 0) return 0;
    TRY(backward_core(c, gscale));
    return linr_axpy(c.A.GSUM, c.L.total, grads, 1, c.s);
}

// One overfit iteration.  `weights` is what the network is evaluated at and differentiated at: the fp32 master `params` itself, or
// with a->qparams != NULL its fake-quantised image (written here, csrc/fake_quant.hip) - the gradient then passes straight through
// to the master, which Adam (weight decay included) updates either way.
// dry: every check of the entry, no launch (csrc/overfit.hip checks a whole GOP in front of its first launch).
int linr_train_step_f32(const linr_frame* f, float* params, float* arena, size_t arena_bytes, const linr_step_args* a, void* stream,
                        bool dry) {
    if (!a || !a->exp_avg || !a->exp_avg_sq || !a->bits_acc || a->step < 1 || (a->qparams && a->qparams == params)) return LINR_EINVAL;
    Ctx c;
    TRY(check_frame(f, params, arena, arena_bytes, c));
    if (a->qparams) TRY(linr_fake_quant_check(params, c.L.total, a->bitdepth, a->qparams, nullptr));
    TRY(linr_scale_steps_check(f, c.L, a->scale_steps_h));       // before anything is launched
    if (dry) return 0;
    c.s = (hipStream_t)stream;
    const float* weights = params;
    if (a->qparams) {
        ProfScope ps(c.s, PK_MISC, 0);
        TRY(linr_fake_quant_launch(params, c.L.total, a->bitdepth, a->qparams, nullptr, nullptr, c.s));
        weights = a->qparams;
    }
    TRY(linr_net_forward(f, weights, arena, arena_bytes, 0, 8, nullptr, a->bits_acc, stream));
    if (c.R == 0) return 0;
    c.P = weights;
    TRY(backward_core(c, a->gscale));
    ProfScope ps(c.s, PK_MISC, 0);
    return linr_adam_step_launch(c.L, c.L.total, params, c.A.GSUM, *a, c.s);
}

extern "C" int linr_net_train_step(const linr_frame* f, float* params, float* arena, size_t arena_bytes, const linr_step_args* a,
                                   void* stream) {
    return linr_train_step_f32(f, params, arena, arena_bytes, a, stream, false);
}
