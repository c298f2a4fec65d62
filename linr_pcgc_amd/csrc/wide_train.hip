// The training step of the hidden_channel_conv = 16 / 32 network as C calls: the schedule of linr_pcgc_amd/wide_net.py
// (WideNet._forward(keep=True) / _Block.fwd and WideNet._backward / _Block.bwd in the fused-pointwise, paired-weight-gradient form)
// launch for launch, through the public entries of csrc/wide.hip / csrc/wide_mul.hip with the arguments the Python executor hands
// them - equal launches with equal arguments, so the bits, the gradient and the updated parameters are those of the Python schedule
// bit for bit.  main.py:305-321 at channels = 16 / 32; models/model_core.py:38-81, models/upsample.py:88-97,137-217,
// models/resnet.py:12-60 and their autograd backward.
//
// Here: the training arena (every tensor of the tape has its own blocks - all of them stay live until the backward -, the gradient
// blocks are reused by role), the two schedules, the deferred weight-gradient reductions in batches of a slab budget, and the
// entries.  Device code of its own: ONE glue launch per step (zero rows of all arena blocks, the gradient vector, the zero weight of
// the ReLU-mask pass); Adam is the launch of csrc/bwd_tail.hip over the wide layout, the fake quantisation that of csrc/fake_quant.hip.
#include "common.h"
#include "layout.h"
#include "prof.h"
#include "bwd_tail.h"
#include "fake_quant.h"
#include "wide_common.h"
#include "wide_layout.h"

namespace {

// slab bytes of the deferred weight-gradient reductions that may wait at once: when the next launch's slab does not fit behind
// the waiting ones they are reduced (linr_wide_reduce_many) and the region starts over.  Every reduction is independent and keeps its
// fixed order, so where the batches end does not change a bit.  The largest single slab is a 32 -> 32 convolution's: 256 rows x 16
// block pairs x WW_PAIR floats = 28.4 MB.
#define WT_SLAB_BUDGET ((size_t)64 << 20)
#define WT_MAX_DEFER 96

// ---- arena ---------------------------------------------------------------------------------------------------------------------
// Byte offsets of the regions; the blocks are fp32 [rows + 1][8] matrices with the zero row in front, back to back.  Block indices
// (nb = C / 8, nh = C / 16), slot s = 0: block_in (BL Inception layers), 1..7: outter_blocks[s - 1] (one layer):
//   tape:      x0 1 | occ 1 (the padded copy of an occupancy that has no zero row) |
//              per slot: a nb, per layer (h0 nh, h1 nh, m nh, i nb), out nb (slot 0: x_glob, slot k: prior_k) | c nb per stage
//   gradients: g_x0 1 | g_xg nb | g_c 8 nb | g_prior 7 nb | per-block roles, reused by every block's backward:
//              gm nh, gil nb, ga nb, gh1 nh, gh0 nh, gx nb x 2 (the layers of a deeper block_in alternate)
struct TSlot { int a, h0[MAX_BL], h1[MAX_BL], m[MAX_BL], i[MAX_BL], out; };
struct TArena {
    size_t hid;                   // the scale context's hidden layer [rows][16]
    size_t parts, p;              // 8 stages' per-block bits partials; 8 stages' probabilities [8][rows]
    size_t gvec;                  // the step's gradient vector (n_params floats)
    size_t zw;                    // 64 zero floats: the weight of the in-place ReLU-mask pass
    size_t head_slab, sce_slab;
    size_t wslab; size_t wslab_bytes;
    size_t blocks; int nblk; size_t block_bytes;
    int x0, occ, c[8], g_x0, g_xg, g_c[8], g_prior[8], gm, gil, ga, gh1, gh0, gx[2];
    TSlot slot[8];
    size_t total;
};

bool make_tarena(TArena& a, int64_t rows, int C, int BL, int64_t n_params) {
    if (rows < 0 || !linr_rows_fit32(rows) || (C != 16 && C != 32) || BL < 1 || BL > MAX_BL) return false;
    size_t cur = 0;
    auto takeb = [&](size_t bytes) { size_t o = cur; cur += wup256(bytes); return o; };
    a.hid = takeb((size_t)rows * 16 * sizeof(float));
    a.parts = takeb((size_t)8 * linr_grid(rows, LINR_BLOCK) * sizeof(double));
    a.p = takeb((size_t)8 * (size_t)rows * sizeof(float));
    a.gvec = takeb((size_t)n_params * sizeof(float));
    a.zw = takeb(64 * sizeof(float));
    a.head_slab = takeb(linr_head_wide_bwd_slab_bytes(C, 8));
    a.sce_slab = takeb(linr_sce_bwd_params_slab_bytes(MAX_SCALES));
    a.wslab_bytes = WT_SLAB_BUDGET;
    a.wslab = takeb(a.wslab_bytes);
    const int nb = C / 8, nh = C / 16;
    int r = 0;
    auto role = [&](int count) { int o = r; r += count; return o; };
    a.x0 = role(1); a.occ = role(1);
    for (int s = 0; s < 8; ++s) {
        TSlot& t = a.slot[s];
        t.a = role(nb);
        for (int l = 0; l < (s == 0 ? BL : 1); ++l) { t.h0[l] = role(nh); t.h1[l] = role(nh); t.m[l] = role(nh); t.i[l] = role(nb); }
        t.out = role(nb);
    }
    for (int k = 0; k < 8; ++k) a.c[k] = role(nb);
    a.g_x0 = role(1); a.g_xg = role(nb);
    for (int k = 0; k < 8; ++k) a.g_c[k] = role(nb);
    a.g_prior[0] = -1;
    for (int k = 1; k < 8; ++k) a.g_prior[k] = role(nb);
    a.gm = role(nh); a.gil = role(nb); a.ga = role(nb); a.gh1 = role(nh); a.gh0 = role(nh); a.gx[0] = role(nb); a.gx[1] = role(nb);
    a.nblk = r;
    a.block_bytes = (size_t)(rows + 1) * 32;
    a.blocks = takeb((size_t)a.nblk * a.block_bytes);
    a.total = cur;
    return true;
}

// ---- glue: what the library must initialise itself ---------------------------------------------------------------------------------
// the zero rows of all arena blocks (8 words each), `nvec` floats of a gradient vector, the 64 zero weights
struct TInit { uint32_t* blocks; int64_t stride_words; int nblk; float* vec; int64_t nvec; float* zw; };
__global__ __launch_bounds__(LINR_BLOCK) void wide_train_init_k(TInit a) {
    const int64_t t = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    const int64_t nz = (int64_t)a.nblk * 8;
    if (t < nz) a.blocks[(t >> 3) * a.stride_words + (t & 7)] = 0u;
    else if (t - nz < a.nvec) a.vec[t - nz] = 0.0f;
    else if (t - nz - a.nvec < 64) a.zw[t - nz - a.nvec] = 0.0f;
}
int train_init(char* base, const TArena& A, bool blocks, float* vec, int64_t nvec, hipStream_t s) {
    TInit a;
    a.blocks = (uint32_t*)(base + A.blocks); a.stride_words = (int64_t)(A.block_bytes / 4); a.nblk = blocks ? A.nblk : 0;
    a.vec = vec; a.nvec = vec ? nvec : 0; a.zw = (float*)(base + A.zw);
    linr_poison_hook(s, PK_WIDE);
    wide_train_init_k<<<linr_grid((int64_t)a.nblk * 8 + a.nvec + 64, LINR_BLOCK), LINR_BLOCK, 0, s>>>(a);
    return linr_launch_rc();
}

// ---- the pass ------------------------------------------------------------------------------------------------------------------------
struct Wt {
    const linr_frame* f; const float* P; const WLayout* W;
    char* base; const TArena* A;
    int64_t n; int nb, nh;
    unsigned mul;                 // LINR_MUL_BF16 or 0: the products of every 3x3x3 convolution of the pass (_Pass.mul)
    const float* occ;             // row 0 of the occupancy the launches gather and the heads read
    float* G;                     // the flat gradient the backward writes
    hipStream_t s;
    // deferred reductions waiting in the slab region
    linr_wide_reduce defer[WT_MAX_DEFER]; int n_defer; size_t slab_cur;
    WPtrs blk(int role, int count) const { return WPtrs(base + A->blocks, A->block_bytes, role, count); }
};

int wt_flush(Wt& c) {
    if (c.n_defer > 0) TRY(linr_wide_reduce_many(c.defer, c.n_defer, c.s));
    c.n_defer = 0; c.slab_cur = 0;
    return 0;
}
// `bytes` of the slab region for a launch that defers `items` reductions
int wt_slab(Wt& c, size_t bytes, int items, float** slab) {
    bytes = wup256(bytes);
    if (bytes > c.A->wslab_bytes) return LINR_ENOSPC;
    if (c.slab_cur + bytes > c.A->wslab_bytes || c.n_defer + items > WT_MAX_DEFER) TRY(wt_flush(c));
    *slab = (float*)(c.base + c.A->wslab + c.slab_cur);
    c.slab_cur += bytes;
    return 0;
}

int wt_conv(const Wt& c, int bwd, const float* const* in, int64_t w, const float* bias, int cin, int cout, const float* const* res,
            const float* const* act, float* const* out, unsigned flags, const linr_wide_pw* pw) {
    return linr_spconv_wide(bwd, in, c.f->nbr_lo, c.f->nbr_mask, c.f->nbr_ld, c.n, c.P + w, bias, cin, cout, res, act, out,
                            flags | (act ? LINR_RELU_MASK : 0u) | c.mul, pw, c.s);
}
// _Conv.bwd's weight gradient: partials into a slab of the region, the reduction deferred
int wt_conv_wgrad(Wt& c, const float* const* xs, const float* const* gs, int cin, int cout, int64_t w, int64_t b) {
    float* slab;
    TRY(wt_slab(c, (size_t)256 * ((cin + 7) / 8) * (cout / 8) * WW_PAIR * sizeof(float), 1, &slab));
    TRY(linr_spconv_wgrad_wide(xs, cin, gs, cout, c.f->nbr, c.f->nbr8t, c.f->nbr_ld, c.n, slab, nullptr, c.G + b, c.mul, c.s));
    c.defer[c.n_defer++] = {0, linr_spconv_wgrad_wide_blocks(cout, 1), cin, cout, 0, 0, slab, c.G + w, c.G + b};
    return 0;
}
// _Pointwise.wgrad (ME layout [cin][cout]: strides (cout, 1))
int wt_pw_wgrad(Wt& c, const float* const* xs, int cin, const float* const* gs, int cout, int64_t w, int64_t b) {
    const size_t bytes = linr_linear_wgrad_wide_workspace_bytes(c.n, cin, cout);
    float* ws;
    TRY(wt_slab(c, bytes, 1, &ws));
    TRY(linr_linear_wgrad_wide(xs, cin, 1, gs, cout, 1, c.n, nullptr, cout, 1, c.G + b, 0, ws, bytes, c.s));
    c.defer[c.n_defer++] = {1, linr_linear_wgrad_wide_blocks(c.n), cin, cout, cout, 1, ws, c.G + w, c.G + b};
    return 0;
}

// ---- forward (WideNet._forward(keep=True)) ---------------------------------------------------------------------------------------------
// make_block (models/upsample.py:88-97) as _Block.fwd runs it, every tensor in its own blocks of slot t
int wt_block_fwd(const Wt& c, const WBlock& bp, const TSlot& t, const float* const* in, const float* const* res) {
    const int C = c.W->C, h = C / 2, nb = c.nb, nh = c.nh;
    const WPtrs a = c.blk(t.a, nb);
    TRY(wt_conv(c, 0, in, bp.a_w, c.P + bp.a_b, bp.cin, C, nullptr, nullptr, a.out(), LINR_RELU, nullptr));
    WPtrs x = a;
    for (int l = 0; l < bp.nl; ++l) {
        const WInc& q = bp.inc[l];
        const WPtrs h0 = c.blk(t.h0[l], nh), h1 = c.blk(t.h1[l], nh), m = c.blk(t.m[l], nh), I = c.blk(t.i[l], nb);
        // conv1_0 rides in conv0_0's launch, conv1_2 + the residual's upper half in conv1_1's
        const linr_wide_pw pw1 = {1, c.P + q.c10_w, c.P + q.c10_b, nullptr, h1.out()};
        TRY(wt_conv(c, 0, x.in(), q.c00_w, c.P + q.c00_b, C, h, nullptr, nullptr, h0.out(), LINR_RELU, &pw1));
        TRY(wt_conv(c, 0, h0.in(), q.c01_w, c.P + q.c01_b, h, h, x.in(), nullptr, I.out(), 0, nullptr));
        const linr_wide_pw pw2 = {2, c.P + q.c12_w, c.P + q.c12_b, x.in() + nh, I.out() + nh};
        TRY(wt_conv(c, 0, h1.in(), q.c11_w, c.P + q.c11_b, h, h, nullptr, nullptr, m.out(), LINR_RELU, &pw2));
        x = I;
    }
    if (bp.nl > 1)           // ResNetBlock.forward: out += x (models/resnet.py:160-161)
        for (int b = 0; b < nb; ++b) TRY(linr_axpy(a.p[b], c.n * 8, x.p[b], 1, c.s));
    const WPtrs out = c.blk(t.out, nb);
    return wt_conv(c, 0, x.in(), bp.b_w, c.P + bp.b_b, C, C, res, nullptr, out.out(), 0, nullptr);
}

int forward_train(const Wt& c, double* bits_acc) {
    const WLayout& W = *c.W;
    const TArena& A = *c.A;
    const int C = W.C, nb = c.nb;
    const WPtrs x0 = c.blk(A.x0, 1), xg = c.blk(A.slot[0].out, nb);
    TRY(linr_sce_fwd(c.P, c.f, nullptr, (float*)(c.base + A.hid), x0.p[0], c.s));
    TRY(wt_block_fwd(c, W.block_in, A.slot[0], x0.in(), nullptr));
    const int64_t nblk = linr_grid(c.n, LINR_BLOCK);
    double* parts = bits_acc ? (double*)(c.base + A.parts) : nullptr;
    const float* occ_in[4] = {c.occ, nullptr, nullptr, nullptr};
    for (int k = 0; k < 8; ++k) {
        // prior_k = x_glob + outter_blocks[k - 1](occ[:, :k])   (upsample.py:206-214)
        if (k > 0) TRY(wt_block_fwd(c, W.outter[k - 1], A.slot[k], occ_in, xg.in()));
        const WPtrs prior = c.blk(A.slot[k].out, nb), cc = c.blk(A.c[k], nb);
        TRY(wt_conv(c, 0, prior.in(), W.pr_w[k], c.P + W.pr_b[k], C, C, nullptr, nullptr, cc.out(), 0, nullptr));
        float* p = (float*)(c.base + A.p) + (int64_t)k * c.n;
        double* part = parts ? parts + (int64_t)k * nblk : nullptr;
        TRY(linr_head_wide_fwd(cc.in(), C, c.P + W.h0_w[k], c.P + W.h0_b[k], c.P + W.h2_w[k], c.P + W.h2_b[k], part ? c.occ + k : nullptr,
                               part ? 8 : 1, c.n, p, nullptr, part, part ? (size_t)nblk * sizeof(double) : 0, c.s));
    }
    if (parts) TRY(linr_bits_finish(parts, (int64_t)8 * nblk, bits_acc, c.s));          // all stages' partials in one fixed-order pass
    return 0;
}

// ---- backward (WideNet._backward) --------------------------------------------------------------------------------------------------------
// _Block.bwd: g_out = the gradient of the block's output; gin: where the input gradient goes (block_in) or nullptr
int wt_block_bwd(Wt& c, const WBlock& bp, const TSlot& t, const float* const* in, const float* const* g_out, float* const* gin) {
    const TArena& A = *c.A;
    const int C = c.W->C, h = C / 2, nb = c.nb, nh = c.nh, nl = bp.nl;
    const WPtrs a = c.blk(t.a, nb), il = c.blk(t.i[nl - 1], nb);
    const WPtrs gm = c.blk(A.gm, nh), gil = c.blk(A.gil, nb), ga = c.blk(A.ga, nb), gh1 = c.blk(A.gh1, nh), gh0 = c.blk(A.gh0, nh);
    {   // the tail convolution; gM of the LAST Inception layer (backward of conv1_2 and of M's ReLU) rides in its backward-data launch
        const WInc& ql = bp.inc[nl - 1];
        const WPtrs ml = c.blk(t.m[nl - 1], nh);
        TRY(wt_conv_wgrad(c, il.in(), g_out, C, C, bp.b_w, bp.b_b));
        const linr_wide_pw pw3 = {3, c.P + ql.c12_w, nullptr, ml.in(), gm.out()};
        TRY(wt_conv(c, 1, g_out, bp.b_w, nullptr, C, C, nullptr, nullptr, gil.out(), 0, &pw3));
    }
    if (nl > 1)              // the extra skip: a receives g_il as well
        for (int b = 0; b < nb; ++b) TRY(linr_axpy(gil.p[b], c.n * 8, ga.p[b], 0, c.s));
    WPtrs gi = gil;
    for (int li = 0; li < nl; ++li) {
        const int l = nl - 1 - li;
        const WInc& q = bp.inc[l];
        const WPtrs x = l == 0 ? a : c.blk(t.i[l - 1], nb);
        const WPtrs h0 = c.blk(t.h0[l], nh), h1 = c.blk(t.h1[l], nh), m = c.blk(t.m[l], nh);
        TRY(wt_pw_wgrad(c, m.in(), h, gi.in() + nh, h, q.c12_w, q.c12_b));
        if (li > 0)          // conv1_2's backward-data pass with M's ReLU mask (the last layer's rode in the tail convolution)
            TRY(linr_linear_wide(gi.in() + nh, h, 1, c.P + q.c12_w, 1, h, nullptr, h, 1, nullptr, m.in(), gm.out(), c.n,
                                 LINR_RELU_MASK | LINR_NO_BIAS, c.s));
        TRY(wt_conv(c, 1, gm.in(), q.c11_w, nullptr, h, h, nullptr, h1.in(), gh1.out(), 0, nullptr));
        TRY(wt_conv(c, 1, gi.in(), q.c01_w, nullptr, h, h, nullptr, h0.in(), gh0.out(), 0, nullptr));
        {   // the weight gradients of conv0_1 and conv1_1 (same shape, independent) as ONE launch
            const int64_t stride = (int64_t)2 * nh * nh * WW_PAIR;
            float* slab;
            TRY(wt_slab(c, (size_t)256 * stride * sizeof(float), 2, &slab));
            TRY(linr_spconv_wgrad_wide2(h0.in(), gi.in(), h1.in(), gm.in(), h, c.f->nbr8t, c.n, slab, c.mul, c.s));
            c.defer[c.n_defer++] = {0, 256, h, h, (int32_t)stride, 0, slab, c.G + q.c01_w, c.G + q.c01_b};
            c.defer[c.n_defer++] = {0, 256, h, h, (int32_t)stride, 0, slab + (int64_t)nh * nh * WW_PAIR, c.G + q.c11_w, c.G + q.c11_b};
        }
        // the layer's input gradient: the residual's share g_i rides in conv0_0's backward-data epilogue (+ res), conv1_0's share is
        // added in front of the mask - for the one layer of a one-layer block the ReLU mask of a = relu(first conv)
        TRY(wt_pw_wgrad(c, x.in(), C, gh1.in(), h, q.c10_w, q.c10_b));
        TRY(wt_conv_wgrad(c, x.in(), gh0.in(), C, h, q.c00_w, q.c00_b));
        const WPtrs gx = c.blk(A.gx[li & 1], nb);
        const linr_wide_pw pw4 = {4, c.P + q.c10_w, nullptr, gh1.in(), nullptr};
        TRY(wt_conv(c, 1, gh0.in(), q.c00_w, nullptr, C, h, gi.in(), nl == 1 ? a.in() : nullptr, gx.out(), 0, &pw4));
        gi = gx;
    }
    if (nl > 1) {
        for (int b = 0; b < nb; ++b) TRY(linr_axpy(ga.p[b], c.n * 8, gi.p[b], 1, c.s));
        // g_i is the gradient of a = relu(first conv): mask it in place - the pointwise backward-data kernel with a zero weight block,
        // accumulate and mask: out = (0 + old) * (a > 0)
        const float* zw = (const float*)(c.base + A.zw);
        for (int b = 0; b < nb; ++b)
            TRY(linr_linear_bwd_data(gi.p[b], 8, c.n, zw, 8, 1, 8, 8, a.p[b], 8, gi.p[b], 8, LINR_ACCUM | LINR_RELU_MASK, c.s));
    }
    TRY(wt_conv_wgrad(c, in, gi.in(), bp.cin, C, bp.a_w, bp.a_b));
    if (!gin) return 0;
    return wt_conv(c, 1, gi.in(), bp.a_w, nullptr, bp.cin, C, nullptr, nullptr, gin, 0, nullptr);
}

int backward(Wt& c, float gscale) {
    const WLayout& W = *c.W;
    const TArena& A = *c.A;
    const int C = W.C, nb = c.nb;
    // d(bits)/d(nats) = 1 / ln 2, multiplied in double and rounded once: what the Python schedule hands the head kernel
    const float gz_scale = (float)((double)gscale * 1.4426950408889634);
    c.n_defer = 0; c.slab_cur = 0;
    const WPtrs gxg = c.blk(A.g_xg, nb);
    {   // all 8 heads first, as one grouped launch: the gradients of the prune convolutions' outputs and the heads' parameter gradients
        const float *cs[8 * 4], *ps[8], *ts[8], *w1[8], *b1[8], *w2[8];
        float* gcs[8 * 4];
        for (int k = 0; k < 8; ++k) {
            const WPtrs cc = c.blk(A.c[k], nb), gc = c.blk(A.g_c[k], nb);
            for (int b = 0; b < nb; ++b) { cs[k * nb + b] = cc.p[b]; gcs[k * nb + b] = gc.p[b]; }
            ps[k] = (const float*)(c.base + A.p) + (int64_t)k * c.n; ts[k] = c.occ + k;
            w1[k] = c.P + W.h0_w[k]; b1[k] = c.P + W.h0_b[k]; w2[k] = c.P + W.h2_w[k];
        }
        const size_t bytes = linr_head_wide_bwd_slab_bytes(C, 8);
        TRY(linr_head_wide_bwd(cs, ps, ts, 8, w1, b1, w2, C, 8, gz_scale, gcs, c.n, (float*)(c.base + A.head_slab), bytes,
                               c.G + W.h0_w[0], c.s));
    }
    const float* occ_in[4] = {c.occ, nullptr, nullptr, nullptr};
    for (int k = 7; k >= 0; --k) {
        const WPtrs prior = c.blk(A.slot[k].out, nb), gc = c.blk(A.g_c[k], nb);
        TRY(wt_conv_wgrad(c, prior.in(), gc.in(), C, C, W.pr_w[k], W.pr_b[k]));
        const WPtrs gp = k == 0 ? gxg : c.blk(A.g_prior[k], nb);
        TRY(wt_conv(c, 1, gc.in(), W.pr_w[k], nullptr, C, C, nullptr, nullptr, gp.out(), 0, nullptr));
        // prior_k = x_glob + block output: both receive g_prior
        if (k > 0) TRY(wt_block_bwd(c, W.outter[k - 1], A.slot[k], occ_in, gp.in(), nullptr));
    }
    // x_glob's gradient: stage 0's (in g_xg) + the seven priors' - one pass per block, the priors in the order 7 .. 1
    for (int b = 0; b < nb; ++b) {
        const float* src[7];
        for (int k = 7; k >= 1; --k) src[7 - k] = c.blk(A.g_prior[k], nb).p[b];
        TRY(linr_sum_many(src, 7, c.n * 8, gxg.p[b], 1, c.s));
    }
    const WPtrs x0 = c.blk(A.x0, 1), gx0 = c.blk(A.g_x0, 1);
    TRY(wt_block_bwd(c, W.block_in, A.slot[0], x0.in(), gxg.in(), gx0.out()));
    // scale context: ghid, the four parameter gradients of every scale's MLP and the embedding rows, into the gradient's leading floats
    const size_t sbytes = linr_sce_bwd_params_slab_bytes(c.f->model_scale_num);
    TRY(linr_sce_bwd_params(c.P, c.f, gx0.p[0], (const float*)(c.base + A.hid), (float*)(c.base + A.sce_slab), sbytes, c.G, c.s));
    return wt_flush(c);
}

// ---- the checks of the three entries, in their order ------------------------------------------------------------------------------------
// NULL f / params / arena (the caller: its own pointers), alignment, hidden, flags, arena size, [the caller's step arguments], the frame
int check_head(const linr_frame* f, const void* params, const void* arena, size_t arena_bytes, int hidden, uint32_t flags) {
    if (!f || !params || !arena) return LINR_EINVAL;
    if (((uintptr_t)arena) & 63u) return LINR_EALIGN;
    if (hidden != 16 && hidden != 32) return LINR_EINVAL;
    if (flags & ~LINR_MUL_BF16) return LINR_EINVAL;
    const size_t need = linr_net_wide_train_arena_bytes(f->rows, hidden, f->block_layers < 1 ? 1 : f->block_layers);
    if (need == 0) return LINR_EINVAL;
    if (arena_bytes < need) return LINR_ENOSPC;
    return 0;
}
int check_frame(const linr_frame* f, int hidden, Layout& L8, WLayout& W, TArena& A) {
    const int bl = f->block_layers < 1 ? 1 : f->block_layers;
    TRY(linr_frame_layout(f, 1, L8));
    if (!make_wlayout(W, f->model_scale_num, bl, hidden)) return LINR_EINVAL;
    WLayout Wmax;
    if (!make_wlayout(Wmax, MAX_SCALES, bl, hidden) || !make_tarena(A, f->rows, hidden, bl, Wmax.total)) return LINR_EINVAL;
    TRY(wide_frame_matrices_check(f));
    if (f->rows > 0) {           // the weight-gradient kernels read the kernel map and its tiled copy
        if (!f->nbr || !f->nbr8t) return LINR_EINVAL;
        if (!linr_aligned16(f->nbr8t)) return LINR_EALIGN;
    }
    return 0;
}

void make_pass(Wt& c, const linr_frame* f, const float* P, const WLayout& W, void* arena, const TArena& A, uint32_t flags, float* G,
               void* stream) {
    c.f = f; c.P = P; c.W = &W; c.base = (char*)arena; c.A = &A; c.n = f->rows; c.nb = W.C / 8; c.nh = W.C / 16;
    c.mul = flags & LINR_MUL_BF16; c.G = G; c.s = (hipStream_t)stream; c.n_defer = 0; c.slab_cur = 0;
    c.occ = f->occ;
}
// no zero row in front of the caller's occupancy: the launches gather a padded copy (its zero row is one of those the glue clears)
int pad_occ(Wt& c, bool copy) {
    if (c.f->flags & LINR_FRAME_OCC_PADDED) return 0;
    float* pad = c.blk(c.A->occ, 1).p[0];
    if (copy) TRY(linr_hip_rc(hipMemcpyAsync(pad, c.f->occ, (size_t)c.n * 32, hipMemcpyDeviceToDevice, c.s)));
    c.occ = pad;
    return 0;
}

}  // namespace

// sized for the largest scale_num: one arena serves any model of this width and depth
extern "C" size_t linr_net_wide_train_arena_bytes(int64_t rows, int32_t hidden, int32_t block_layers) {
    WLayout W;
    TArena A;
    if (rows < 0 || !make_wlayout(W, MAX_SCALES, block_layers, hidden) || !make_tarena(A, rows, hidden, block_layers, W.total)) return 0;
    return A.total;
}

extern "C" int linr_net_forward_train_wide(const linr_frame* f, const float* params, int32_t hidden, void* arena, size_t arena_bytes,
                                           uint32_t flags, double* bits_acc, void* stream) {
    TRY(check_head(f, params, arena, arena_bytes, hidden, flags));
    Layout L8; WLayout W; TArena A;
    TRY(check_frame(f, hidden, L8, W, A));
    if (f->rows == 0) return 0;
    Wt c;
    make_pass(c, f, params, W, arena, A, flags, nullptr, stream);
    TRY(train_init(c.base, A, true, nullptr, 0, c.s));
    TRY(pad_occ(c, true));
    return forward_train(c, bits_acc);
}

extern "C" int linr_net_backward_wide(const linr_frame* f, const float* params, int32_t hidden, void* arena, size_t arena_bytes,
                                      uint32_t flags, float gscale, float* grads, void* stream) {
    if (!grads) return LINR_EINVAL;
    TRY(check_head(f, params, arena, arena_bytes, hidden, flags));
    Layout L8; WLayout W; TArena A;
    TRY(check_frame(f, hidden, L8, W, A));
    if (f->rows == 0) return 0;
    Wt c;
    make_pass(c, f, params, W, arena, A, flags, grads, stream);
    TRY(train_init(c.base, A, false, grads, W.total, c.s));
    TRY(pad_occ(c, false));          // (the forward on this arena made the copy)
    return backward(c, gscale);
}

// One overfit iteration.  `weights` is what the network is evaluated and differentiated at: the fp32 master `params` itself, or with
// a->qparams != NULL its fake-quantised image (written here) - the gradient then passes straight through to the master, which Adam
// (weight decay included) updates either way.
// dry: every check of the entry, no launch (csrc/overfit.hip checks a whole GOP in front of its first launch).
int linr_train_step_wide(const linr_frame* f, float* params, int32_t hidden, void* arena, size_t arena_bytes, uint32_t flags,
                         const linr_step_args* a, void* stream, bool dry) {
    if (!a) return LINR_EINVAL;
    TRY(check_head(f, params, arena, arena_bytes, hidden, flags));
    if (!a->exp_avg || !a->exp_avg_sq || !a->bits_acc || a->step < 1 || (a->qparams && a->qparams == params)) return LINR_EINVAL;
    if (a->qparams) TRY(linr_fake_quant_check(params, 1, a->bitdepth, a->qparams, nullptr));
    Layout L8; WLayout W; TArena A;
    TRY(check_frame(f, hidden, L8, W, A));
    TRY(linr_scale_steps_check(f, L8, a->scale_steps_h));       // before anything is launched
    if (dry || f->rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const float* weights = params;
    if (a->qparams) {
        linr_poison_hook(s, PK_WIDE);
        TRY(linr_fake_quant_launch(params, W.total, a->bitdepth, a->qparams, nullptr, nullptr, s));
        weights = a->qparams;
    }
    Wt c;
    float* gvec = (float*)((char*)arena + A.gvec);
    make_pass(c, f, weights, W, arena, A, flags, gvec, stream);
    TRY(train_init(c.base, A, true, gvec, W.total, s));          // the step's one glue launch
    TRY(pad_occ(c, true));
    TRY(forward_train(c, a->bits_acc));
    TRY(backward(c, a->gscale));
    linr_poison_hook(s, PK_WIDE);
    return linr_adam_step_launch(L8, W.total, params, gvec, *a, s);
}

extern "C" int linr_net_train_step_wide(const linr_frame* f, float* params, int32_t hidden, void* arena, size_t arena_bytes,
                                        uint32_t flags, const linr_step_args* a, void* stream) {
    return linr_train_step_wide(f, params, hidden, arena, arena_bytes, flags, a, stream, false);
}
