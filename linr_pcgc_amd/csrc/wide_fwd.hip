// The inference forward of the hidden_channel_conv = 16 / 32 network as ONE C call: the schedule of linr_pcgc_amd/wide_net.py
// (WideNet._forward / _Block.fwd in the fused-pointwise form; forward_bf16 / _block_bf16) launch for launch, through the public
// entries of csrc/wide.hip and csrc/wide_bf16.hip with the arguments the Python executor hands them - so the probabilities and the
// bits are those of the Python executor bit for bit, whichever of the two a frame was coded with.  Forward of
// models/model_core.py:38-81, models/upsample.py:88-97,137-217 and models/resnet.py:12-60 at channels = 16 / 32.
//
// Here (the wide parameter layout, parameters() order, is csrc/wide_layout.h): the arena (per-role blocks reused by all blocks and stages, as the Python
// executor's bf16 pool does), the two schedules and their entries.  The only device code is glue: one launch per (0, ...) call that
// clears the zero rows of all arena blocks and, for bf16, writes the convolution table of the prologue.
#include "common.h"
#include "layout.h"
#include "prof.h"
#include "wide_layout.h"

namespace {

// ---- the convolutions of the bf16 prologue's table, in the Python executor's order --------------------------------------------------
#define WF_MAX_CONV 64
struct WConvTab {
    int n;
    int64_t n_img;                     // 8-byte elements of all images
    int64_t v[WF_MAX_CONV * 4];        // kernel offset, cin, cout, image offset
};
int wtab_add(WConvTab& t, int64_t w, int cin, int cout) {
    const int i = t.n++;
    t.v[4 * i] = w; t.v[4 * i + 1] = cin; t.v[4 * i + 2] = cout; t.v[4 * i + 3] = t.n_img;
    t.n_img += linr_wide_bf16_image_elems(cin, cout);
    return i;
}
struct WBlockImg { int first, tail, c00[MAX_BL], c01[MAX_BL], c11[MAX_BL]; };
struct WImgs { WBlockImg blk[8]; int prune[8]; };
void wtab_block(WConvTab& t, const WBlock& b, int C, WBlockImg& bi) {
    const int h = C / 2;
    bi.first = wtab_add(t, b.a_w, b.cin, C);
    bi.tail = wtab_add(t, b.b_w, C, C);
    for (int l = 0; l < b.nl; ++l) {
        bi.c00[l] = wtab_add(t, b.inc[l].c00_w, C, h);
        bi.c01[l] = wtab_add(t, b.inc[l].c01_w, h, h);
        bi.c11[l] = wtab_add(t, b.inc[l].c11_w, h, h);
    }
}
void make_wtab(const WLayout& W, WConvTab& t, WImgs& im) {
    t.n = 0; t.n_img = 0;
    wtab_block(t, W.block_in, W.C, im.blk[0]);
    for (int k = 0; k < 7; ++k) wtab_block(t, W.outter[k], W.C, im.blk[k + 1]);
    for (int k = 0; k < 8; ++k) im.prune[k] = wtab_add(t, W.pr_w[k], W.C, W.C);
}

// ---- arena ---------------------------------------------------------------------------------------------------------------------
// Byte offsets.  The blocks are [rows + 1][8] matrices (fp32: 32-byte rows, bf16: 16-byte rows) with the zero row in front, back to
// back, a role's blocks side by side.  Roles, in blocks (nb = C / 8, nh = C / 16):
//   fp32: x0 1 | occ 1 (the padded copy of an occupancy that has no zero row) | xg nb | a nb | h0 nh | h1 nh | m nh | i0 nb | i1 nb |
//         o nb (prior) | c nb (prune output)
//   bf16: x0 1 | occ 1 | xg nb | a nb | h nb | i0 nb | i1 nb | o nb
// The Inception layers of a deeper block_in alternate between i0 and i1.
struct WArena {
    size_t pf, tab, img;          // bf16: de-quantised parameters, convolution table, weight images
    size_t hid;                   // fp32: the scale context's hidden layer [rows][16]
    size_t parts, p;              // 8 stages' per-block bits partials; probabilities when the caller wants none
    size_t blocks; int nblk; size_t block_bytes;
    size_t total;
};

// n_params / n_img: of the model (bf16), else 0
bool make_warena(WArena& a, int64_t rows, int C, int bf16, int64_t n_params, int n_conv, int64_t n_img) {
    if (rows < 0 || !linr_rows_fit32(rows)) return false;
    size_t cur = 0;
    auto takeb = [&](size_t bytes) { size_t o = cur; cur += wup256(bytes); return o; };
    a.pf = takeb(bf16 ? (size_t)n_params * 4 : 0);
    a.tab = takeb(bf16 ? (size_t)n_conv * 32 : 0);
    a.img = takeb(bf16 ? (size_t)n_img * 8 : 0);
    a.hid = takeb(bf16 ? 0 : (size_t)rows * 16 * 4);
    a.parts = takeb((size_t)8 * linr_grid(rows, LINR_BLOCK) * sizeof(double));
    a.p = takeb((size_t)rows * 4);
    const int nb = C / 8, nh = C / 16;
    a.nblk = bf16 ? 2 + 6 * nb : 2 + 6 * nb + 3 * nh;
    a.block_bytes = (size_t)(rows + 1) * (bf16 ? 16 : 32);
    a.blocks = takeb((size_t)a.nblk * a.block_bytes);
    a.total = cur;
    return true;
}

// ---- glue: zero rows of all blocks, the bf16 prologue's table ----------------------------------------------------------------------
struct WInit {
    uint32_t* blocks; int64_t stride_words; int nblk, wpr;          // wpr: 32-bit words of a row
    int64_t* tab; int n_tab;
    int64_t v[WF_MAX_CONV * 4];
};
__global__ __launch_bounds__(LINR_BLOCK) void wide_arena_init_k(WInit a) {
    const int t = blockIdx.x * LINR_BLOCK + threadIdx.x;
    const int nz = a.nblk * a.wpr;
    if (t < nz) a.blocks[(int64_t)(t / a.wpr) * a.stride_words + t % a.wpr] = 0u;
    else if (t - nz < a.n_tab) a.tab[t - nz] = a.v[t - nz];
}
int arena_init(char* base, const WArena& A, int bf16, const WConvTab* tab, hipStream_t s) {
    WInit a;
    a.blocks = (uint32_t*)(base + A.blocks); a.stride_words = (int64_t)(A.block_bytes / 4); a.nblk = A.nblk; a.wpr = bf16 ? 4 : 8;
    a.tab = (int64_t*)(base + A.tab); a.n_tab = tab ? 4 * tab->n : 0;
    for (int i = 0; i < WF_MAX_CONV * 4; ++i) a.v[i] = i < a.n_tab ? tab->v[i] : 0;
    linr_poison_hook(s, PK_WIDE);
    wide_arena_init_k<<<linr_grid(a.nblk * a.wpr + a.n_tab, LINR_BLOCK), LINR_BLOCK, 0, s>>>(a);
    return linr_launch_rc();
}

// ---- the checks both entries share, in their order ------------------------------------------------------------------------------------
// NULL, alignment, hidden, stage range, arena size, then the frame (linr_frame_layout and what the launches read of it)
int check_call(const linr_frame* f, const void* model, const void* arena, size_t arena_bytes, int hidden, int bf16, int stage_begin,
               int stage_end, WLayout& W, WArena& A, WConvTab& tab, WImgs& im) {
    if (!f || !model || !arena) return LINR_EINVAL;
    if (((uintptr_t)arena) & 63u) return LINR_EALIGN;
    if (hidden != 16 && hidden != 32) return LINR_EINVAL;
    if (stage_begin < 0 || stage_end > 8 || stage_begin >= stage_end) return LINR_EINVAL;
    const int bl = f->block_layers < 1 ? 1 : f->block_layers;
    const size_t need = linr_net_wide_arena_bytes(f->rows, hidden, bl, bf16);
    if (need == 0) return LINR_EINVAL;
    if (arena_bytes < need) return LINR_ENOSPC;
    Layout L8;
    TRY(linr_frame_layout(f, 0, L8));
    if (!make_wlayout(W, f->model_scale_num, bl, hidden)) return LINR_EINVAL;
    tab.n = 0; tab.n_img = 0;
    if (bf16) make_wtab(W, tab, im);
    if (!make_warena(A, f->rows, hidden, bf16, W.total, tab.n, tab.n_img)) return LINR_EINVAL;
    return wide_frame_matrices_check(f);
}

// ---- fp32 schedule (WideNet._forward) ---------------------------------------------------------------------------------------------------
struct Wf {
    const linr_frame* f; const float* P; const WLayout* W;
    char* base; const WArena* A;
    int64_t n; int nb, nh;
    const float* occ;             // row 0 of the occupancy the launches gather and the heads read
    hipStream_t s;
    // block r of the arena: its first row
    float* blk(int r) const { return (float*)(base + A->blocks + (size_t)r * A->block_bytes) + 8; }
    // roles (first block)
    int r_x0() const { return 0; }
    int r_occ() const { return 1; }
    int r_xg() const { return 2; }
    int r_a() const { return 2 + nb; }
    int r_h0() const { return 2 + 2 * nb; }
    int r_h1() const { return 2 + 2 * nb + nh; }
    int r_m() const { return 2 + 2 * nb + 2 * nh; }
    int r_i(int l) const { return 2 + 2 * nb + 3 * nh + (l & 1) * nb; }
    int r_o() const { return 2 + 4 * nb + 3 * nh; }
    int r_c() const { return 2 + 5 * nb + 3 * nh; }
};
// a role's blocks as the host array of device pointers the wide entries take
struct Ptrs {
    float* p[4];
    Ptrs(const Wf& c, int role, int count) { for (int i = 0; i < 4; ++i) p[i] = i < count ? c.blk(role + i) : nullptr; }
    const float* const* in() const { return p; }
    float* const* out() const { return p; }
};

int wf_conv(const Wf& c, const float* const* in, int64_t w, int64_t b, int cin, int cout, const float* const* res, float* const* out,
            unsigned flags, const linr_wide_pw* pw) {
    return linr_spconv_wide(0, in, c.f->nbr_lo, c.f->nbr_mask, c.f->nbr_ld, c.n, c.P + w, c.P + b, cin, cout, res, nullptr, out, flags, pw,
                            c.s);
}

// make_block (models/upsample.py:88-97) as _Block.fwd runs it: in (cin channels in one block, or C) -> out (+ res)
int wf_block(const Wf& c, const WBlock& bp, const float* const* in, const float* const* res, float* const* out) {
    const int C = c.W->C, h = C / 2, nb = c.nb, nh = c.nh;
    const Ptrs a(c, c.r_a(), nb), h0(c, c.r_h0(), nh), h1(c, c.r_h1(), nh), m(c, c.r_m(), nh);
    TRY(wf_conv(c, in, bp.a_w, bp.a_b, bp.cin, C, nullptr, a.out(), LINR_RELU, nullptr));
    Ptrs x = a;
    for (int l = 0; l < bp.nl; ++l) {
        const WInc& q = bp.inc[l];
        const Ptrs I(c, c.r_i(l), nb);
        // conv1_0 rides in conv0_0's launch, conv1_2 + the residual's upper half in conv1_1's
        const linr_wide_pw pw1 = {1, c.P + q.c10_w, c.P + q.c10_b, nullptr, h1.out()};
        TRY(wf_conv(c, x.in(), q.c00_w, q.c00_b, C, h, nullptr, h0.out(), LINR_RELU, &pw1));
        TRY(wf_conv(c, h0.in(), q.c01_w, q.c01_b, h, h, x.in(), I.out(), 0, nullptr));
        const linr_wide_pw pw2 = {2, c.P + q.c12_w, c.P + q.c12_b, x.in() + nh, I.out() + nh};
        TRY(wf_conv(c, h1.in(), q.c11_w, q.c11_b, h, h, nullptr, m.out(), LINR_RELU, &pw2));
        x = I;
    }
    if (bp.nl > 1)           // ResNetBlock.forward: out += x (models/resnet.py:160-161)
        for (int b = 0; b < nb; ++b) TRY(linr_axpy(a.p[b], c.n * 8, x.p[b], 1, c.s));
    return wf_conv(c, x.in(), bp.b_w, bp.b_b, C, C, res, out, 0, nullptr);
}

int forward_f32(const Wf& c, int k0, int k1, float* probs, double* bits_acc) {
    const WLayout& W = *c.W;
    const int C = W.C, nb = c.nb;
    const Ptrs xg(c, c.r_xg(), nb);
    if (k0 == 0) {
        TRY(arena_init(c.base, *c.A, 0, nullptr, c.s));
        const Ptrs x0(c, c.r_x0(), 1);
        TRY(linr_sce_fwd(c.P, c.f, nullptr, (float*)(c.base + c.A->hid), x0.p[0], c.s));
        TRY(wf_block(c, W.block_in, x0.in(), nullptr, xg.out()));
    }
    const int64_t nblk = linr_grid(c.n, LINR_BLOCK);
    double* parts = bits_acc ? (double*)(c.base + c.A->parts) : nullptr;
    const float* occ_in[4] = {c.occ, nullptr, nullptr, nullptr};
    const Ptrs o(c, c.r_o(), nb), cc(c, c.r_c(), nb);
    for (int k = k0; k < k1; ++k) {
        // prior_k = x_glob + outter_blocks[k - 1](occ[:, :k])   (upsample.py:206-214)
        if (k > 0) TRY(wf_block(c, W.outter[k - 1], occ_in, xg.in(), o.out()));
        const Ptrs& prior = k == 0 ? xg : o;
        TRY(wf_conv(c, prior.in(), W.pr_w[k], W.pr_b[k], C, C, nullptr, cc.out(), 0, nullptr));
        float* p = probs ? probs + (int64_t)k * c.n : (float*)(c.base + c.A->p);
        double* part = parts ? parts + (int64_t)(k - k0) * nblk : nullptr;
        TRY(linr_head_wide_fwd(cc.in(), C, c.P + W.h0_w[k], c.P + W.h0_b[k], c.P + W.h2_w[k], c.P + W.h2_b[k], part ? c.occ + k : nullptr,
                               part ? 8 : 1, c.n, p, nullptr, part, part ? (size_t)nblk * sizeof(double) : 0, c.s));
    }
    if (parts) TRY(linr_bits_finish(parts, (int64_t)(k1 - k0) * nblk, bits_acc, c.s));          // all stages' partials in one fixed-order pass
    return 0;
}

// ---- bf16 schedule (WideNet.forward_bf16) --------------------------------------------------------------------------------------------------
struct Wb {
    const linr_frame* f; const WLayout* W; const WConvTab* tab; const WImgs* im;
    char* base; const WArena* A;
    int64_t n, bs;                // rows; a block's elements, zero row included
    int nb, nh;
    hipStream_t s;
    const float* pf() const { return (const float*)(base + A->pf); }
    const void* img(int conv) const { return base + A->img + 8 * (size_t)tab->v[4 * conv + 3]; }
    uint16_t* blk(int r) const { return (uint16_t*)(base + A->blocks + (size_t)r * A->block_bytes) + 8; }
    int r_x0() const { return 0; }
    int r_occ() const { return 1; }
    int r_xg() const { return 2; }
    int r_a() const { return 2 + nb; }
    int r_h() const { return 2 + 2 * nb; }
    int r_i(int l) const { return 2 + 3 * nb + (l & 1) * nb; }
    int r_o() const { return 2 + 5 * nb; }
};

int wb_conv(const Wb& c, int epi, const uint16_t* in, int cin, int conv, int64_t bias, int cout, const uint16_t* res, const uint16_t* res2,
            int64_t pw_w, int64_t pw_b, int relu, uint16_t* out) {
    const float* pf = c.pf();
    return linr_spconv_wide_bf16(epi, in, c.bs, cin, c.f->nbr_lo, c.f->nbr_mask, c.f->nbr_ld, c.n, c.img(conv), pf + bias, cout, res,
                                 res ? c.bs : 0, res2, res2 ? c.bs : 0, pw_w >= 0 ? pf + pw_w : nullptr, pw_b >= 0 ? pf + pw_b : nullptr, relu,
                                 out, c.bs, c.s);
}

// make_block on bf16 blocks as _block_bf16 runs it
int wb_block(const Wb& c, const WBlock& bp, const WBlockImg& bi, const uint16_t* in, const uint16_t* res, uint16_t* out) {
    const int C = c.W->C, h = C / 2;
    const int64_t hi = (int64_t)c.nh * c.bs;          // the upper half of a C-wide matrix
    uint16_t* a = c.blk(c.r_a());
    uint16_t* H = c.blk(c.r_h());
    TRY(wb_conv(c, 0, in, bp.cin, bi.first, bp.a_b, C, nullptr, nullptr, -1, -1, 1, a));
    const uint16_t* x = a;
    for (int l = 0; l < bp.nl; ++l) {
        const WInc& q = bp.inc[l];
        const uint16_t* skip = (bp.nl > 1 && l == bp.nl - 1) ? a : nullptr;          // the extra skip rides in the last layer's launches
        uint16_t* I = c.blk(c.r_i(l));
        TRY(wb_conv(c, 1, x, C, bi.c00[l], q.c00_b, h, nullptr, nullptr, q.c10_w, q.c10_b, 0, H));
        TRY(wb_conv(c, 0, H, h, bi.c01[l], q.c01_b, h, x, skip, -1, -1, 0, I));
        TRY(wb_conv(c, 2, H + hi, h, bi.c11[l], q.c11_b, h, x + hi, skip ? skip + hi : nullptr, q.c12_w, q.c12_b, 0, I + hi));
        x = I;
    }
    return wb_conv(c, 0, x, C, bi.tail, bp.b_b, C, res, nullptr, -1, -1, 0, out);
}

int forward_bf16(const Wb& c, const uint8_t* codes, float min_param, float max_param, int k0, int k1, float* probs, double* bits_acc) {
    const WLayout& W = *c.W;
    const float* pf = c.pf();
    uint16_t* xg = c.blk(c.r_xg());
    uint16_t* occ = c.blk(c.r_occ());
    if (k0 == 0) {
        TRY(arena_init(c.base, *c.A, 1, c.tab, c.s));
        TRY(linr_wide_bf16_prep(codes, W.total, min_param, max_param, (const int64_t*)(c.base + c.A->tab), c.tab->n, c.tab->n_img,
                                (float*)(c.base + c.A->pf), c.base + c.A->img, c.s));
        uint16_t* x0 = c.blk(c.r_x0());
        TRY(linr_sce_fwd_bf16(pf, c.f, x0 - 8, c.s));
        TRY(linr_occ_to_bf16(c.f->occ, c.n, occ - 8, c.s));
        TRY(wb_block(c, W.block_in, c.im->blk[0], x0, nullptr, xg));
    } else {
        TRY(linr_occ_to_bf16(c.f->occ, c.n, occ - 8, c.s));          // the decoder fills the occupancy column by column
    }
    const int64_t nblk = linr_grid(c.n, LINR_BLOCK);
    double* parts = bits_acc ? (double*)(c.base + c.A->parts) : nullptr;
    uint16_t* o = c.blk(c.r_o());
    for (int k = k0; k < k1; ++k) {
        if (k > 0) TRY(wb_block(c, W.outter[k - 1], c.im->blk[k], occ, xg, o));
        const uint16_t* prior = k == 0 ? xg : o;
        float* p = probs ? probs + (int64_t)k * c.n : (float*)(c.base + c.A->p);
        double* part = parts ? parts + (int64_t)(k - k0) * nblk : nullptr;
        TRY(linr_head_wide_bf16_fwd(prior, c.bs, W.C, c.f->nbr_lo, c.f->nbr_mask, c.f->nbr_ld, c.n, c.img(c.im->prune[k]), pf + W.pr_b[k],
                                    pf + W.h0_w[k], pf + W.h0_b[k], pf + W.h2_w[k], pf + W.h2_b[k], part ? c.f->occ : nullptr, k, p, part,
                                    c.s));
    }
    if (parts) TRY(linr_bits_finish(parts, (int64_t)(k1 - k0) * nblk, bits_acc, c.s));
    return 0;
}

}  // namespace

extern "C" int64_t linr_param_count_wide(int32_t scale_num, int32_t block_layers, int32_t hidden) {
    WLayout W;
    return make_wlayout(W, scale_num, block_layers, hidden) ? W.total : 0;
}

// sized for the largest scale_num: one arena serves any model of this width and depth
extern "C" size_t linr_net_wide_arena_bytes(int64_t rows, int32_t hidden, int32_t block_layers, int32_t bf16) {
    WLayout W;
    if (rows < 0 || !make_wlayout(W, MAX_SCALES, block_layers, hidden)) return 0;
    WConvTab tab;
    WImgs im;
    tab.n = 0; tab.n_img = 0;
    if (bf16) make_wtab(W, tab, im);
    WArena A;
    if (!make_warena(A, rows, hidden, bf16 ? 1 : 0, W.total, tab.n, tab.n_img)) return 0;
    return A.total;
}

extern "C" int linr_net_forward_wide(const linr_frame* f, const float* params, int32_t hidden, void* arena, size_t arena_bytes,
                                     int32_t stage_begin, int32_t stage_end, float* probs, double* bits_acc, void* stream) {
    WLayout W; WArena A; WConvTab tab; WImgs im;
    TRY(check_call(f, params, arena, arena_bytes, hidden, 0, stage_begin, stage_end, W, A, tab, im));
    if (f->rows == 0) return 0;
    Wf c;
    c.f = f; c.P = params; c.W = &W; c.base = (char*)arena; c.A = &A; c.n = f->rows; c.nb = hidden / 8; c.nh = hidden / 16;
    c.s = (hipStream_t)stream;
    c.occ = f->occ;
    if (!(f->flags & LINR_FRAME_OCC_PADDED)) {
        // no zero row in front of the caller's occupancy: the launches gather a padded copy, made anew in every call (the decoder
        // fills the occupancy column by column); its zero row is one of those the (0, ...) call clears
        float* copy = c.blk(c.r_occ());
        TRY(linr_hip_rc(hipMemcpyAsync(copy, f->occ, (size_t)c.n * 32, hipMemcpyDeviceToDevice, c.s)));
        c.occ = copy;
    }
    return forward_f32(c, stage_begin, stage_end, probs, bits_acc);
}

extern "C" int linr_net_forward_wide_bf16(const linr_frame* f, const uint8_t* codes, float min_param, float max_param, int32_t hidden,
                                          void* arena, size_t arena_bytes, int32_t stage_begin, int32_t stage_end, float* probs,
                                          double* bits_acc, void* stream) {
    WLayout W; WArena A; WConvTab tab; WImgs im;
    TRY(check_call(f, codes, arena, arena_bytes, hidden, 1, stage_begin, stage_end, W, A, tab, im));
    if (f->rows == 0) return 0;
    Wb c;
    c.f = f; c.W = &W; c.tab = &tab; c.im = &im; c.base = (char*)arena; c.A = &A; c.n = f->rows; c.bs = (f->rows + 1) * 8;
    c.nb = hidden / 8; c.nh = hidden / 16; c.s = (hipStream_t)stream;
    return forward_bf16(c, codes, min_param, max_param, stage_begin, stage_end, probs, bits_acc);
}
