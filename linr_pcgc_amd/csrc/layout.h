// Parameter layout of LINR_PCGC_Model in parameters() order (models/model_core.py:31-35, models/upsample.py:43-76),
// shared by the fp32 executor (net.hip) and the bf16 / uint8-weight inference executor (net_bf16.hip), and the frame contract
// every executor entry checks against it.
#pragma once
#include <stdint.h>
#include "../../include/linr_hip.h"
#define MAX_SCALES 16
#define MAX_BL 4              // block_layers of block_in (main.py:521 default 1; the outter blocks always have 1, upsample.py:72-76)
struct IncP {                 // one InceptionResNet layer (models/resnet.py:7-60)
    int64_t c00_w, c00_b;     // conv0_0  conv3 8->4
    int64_t c01_w, c01_b;     // conv0_1  conv3 4->4
    int64_t c10_w, c10_b;     // conv1_0  1x1 8->4   kernel [8][4]
    int64_t c11_w, c11_b;     // conv1_1  conv3 4->4
    int64_t c12_w, c12_b;     // conv1_2  1x1 4->4   kernel [4][4]
};
struct BlockP {
    int cin;
    int nl;                   // Inception layers of the ResNetBlock (.2.layers.0 .. nl-1)
    int64_t a_w, a_b;         // .0   conv3 cin->8
    IncP inc[MAX_BL];
    int64_t b_w, b_b;         // .3   conv3 8->8
};

struct Layout {
    int S;
    int BL;                                        // block_layers of block_in
    int64_t emb;                                   // [S][8]
    int64_t m0_w[MAX_SCALES], m0_b[MAX_SCALES];    // Linear(15,16): weight [16][15]
    int64_t m2_w[MAX_SCALES], m2_b[MAX_SCALES];    // Linear(16,8):  weight [8][16]
    BlockP block_in;
    int64_t h0_w[8], h0_b[8], h2_w[8], h2_b[8];    // inner_mlps.k.0: Linear(8,24), Linear(24,1)
    int64_t pr_w[8], pr_b[8];                      // prune_blocks.k.0.conv: conv3 8->8
    BlockP outter[7];
    int64_t total;
};

static inline int64_t take(int64_t& cur, int64_t n) { int64_t o = cur; cur += n; return o; }

static inline void layout_block(BlockP& b, int cin, int nl, int64_t& cur) {
    b.cin = cin;
    b.nl = nl;
    b.a_w = take(cur, 27 * cin * 8);  b.a_b = take(cur, 8);
    for (int l = 0; l < nl; ++l) {
        IncP& q = b.inc[l];
        q.c00_w = take(cur, 27 * 8 * 4);  q.c00_b = take(cur, 4);
        q.c01_w = take(cur, 27 * 4 * 4);  q.c01_b = take(cur, 4);
        q.c10_w = take(cur, 8 * 4);       q.c10_b = take(cur, 4);
        q.c11_w = take(cur, 27 * 4 * 4);  q.c11_b = take(cur, 4);
        q.c12_w = take(cur, 4 * 4);       q.c12_b = take(cur, 4);
    }
    b.b_w = take(cur, 27 * 8 * 8);    b.b_b = take(cur, 8);
}

static inline const BlockP& slot_block(const Layout& L, int b) { return b == 0 ? L.block_in : L.outter[b - 1]; }   // block of slot b

static inline bool make_layout(Layout& L, int S, int BL = 1) {
    if (S < 1 || S > MAX_SCALES || BL < 1 || BL > MAX_BL) return false;
    L.S = S;
    L.BL = BL;
    int64_t cur = 0;
    L.emb = take(cur, (int64_t)S * 8);
    for (int s = 0; s < S; ++s) {
        L.m0_w[s] = take(cur, 16 * 15); L.m0_b[s] = take(cur, 16);
        L.m2_w[s] = take(cur, 8 * 16);  L.m2_b[s] = take(cur, 8);
    }
    layout_block(L.block_in, 8, BL, cur);
    for (int k = 0; k < 8; ++k) {
        L.h0_w[k] = take(cur, 24 * 8); L.h0_b[k] = take(cur, 24);
        L.h2_w[k] = take(cur, 24);     L.h2_b[k] = take(cur, 1);
    }
    for (int k = 0; k < 8; ++k) { L.pr_w[k] = take(cur, 27 * 8 * 8); L.pr_b[k] = take(cur, 8); }
    for (int k = 0; k < 7; ++k) layout_block(L.outter[k], k + 1, 1, cur);
    L.total = cur;
    return true;
}

// The structure of a linr_frame (include/linr_hip.h), checked once for every entry that takes one: 1..MAX_SCALES scales with their
// host arrays, row_off_h rising from 0 to rows, every scale_idx_h inside the model.  Builds L at block_layers, 0 = the frame's own
// (0 read as 1).  What an entry needs beyond this - its matrices, the row bound, its arena - it checks itself.  LINR_EINVAL or 0.
static inline int linr_frame_layout(const linr_frame* f, int block_layers, Layout& L) {
    if (!f || f->rows < 0 || f->n_scales < 1 || f->n_scales > MAX_SCALES || !f->row_off_h || !f->scale_idx_h) return LINR_EINVAL;
    if (block_layers == 0) block_layers = f->block_layers < 1 ? 1 : f->block_layers;
    if (!make_layout(L, f->model_scale_num, block_layers)) return LINR_EINVAL;
    if (f->row_off_h[0] != 0 || f->row_off_h[f->n_scales] != f->rows) return LINR_EINVAL;
    for (int s = 0; s < f->n_scales; ++s)
        if (f->row_off_h[s + 1] < f->row_off_h[s] || f->scale_idx_h[s] < 0 || f->scale_idx_h[s] >= f->model_scale_num) return LINR_EINVAL;
    return 0;
}

// scale_steps_h of the training steps (NULL: none), for a frame that has passed linr_frame_layout with L: no negative entry, and a scale
// that has rows in this frame cannot be "never started".  LINR_EINVAL or 0.
static inline int linr_scale_steps_check(const linr_frame* f, const Layout& L, const int64_t* scale_steps_h) {
    if (!scale_steps_h) return 0;
    for (int s = 0; s < L.S; ++s)
        if (scale_steps_h[s] < 0) return LINR_EINVAL;
    for (int j = 0; j < f->n_scales; ++j)
        if (f->row_off_h[j + 1] > f->row_off_h[j] && scale_steps_h[f->scale_idx_h[j]] < 1) return LINR_EINVAL;
    return 0;
}

// The per-scale table of the scale-context kernels (SceArgs of sce.h, BSce of bf16_common.h): every scale's first row and the
// offsets of its embedding and MLP parameters, for a frame that has passed linr_frame_layout with L.
template <class T>
static inline void linr_sce_table(const linr_frame* f, const Layout& L, T& a) {
    a.n_scales = f->n_scales;
    for (int s = 0; s < f->n_scales; ++s) {
        const int si = f->scale_idx_h[s];
        a.row_off[s] = f->row_off_h[s];
        a.emb[s] = L.emb + si * 8; a.w1[s] = L.m0_w[si]; a.b1[s] = L.m0_b[si]; a.w2[s] = L.m2_w[si]; a.b2[s] = L.m2_b[si];
    }
    a.row_off[f->n_scales] = f->rows;
}
