// What the C schedules of the hidden_channel_conv = 16 / 32 network share (csrc/wide_fwd.hip: the inference forward; csrc/wide_train.hip:
// the training step): the parameter layout in parameters() order, the block-pointer helper of an arena of [rows + 1][8] blocks and
// the frame checks common to their entries.  Not part of the C-ABI.
#pragma once
#include "common.h"
#include "layout.h"

#ifndef TRY
#define TRY(e) do { int rc_ = (e); if (rc_) return rc_; } while (0)
#endif

// ---- parameter layout ------------------------------------------------------------------------------------------------------------
struct WInc { int64_t c00_w, c00_b, c01_w, c01_b, c10_w, c10_b, c11_w, c11_b, c12_w, c12_b; };
struct WBlock {
    int cin, nl;
    int64_t a_w, a_b;         // .0  conv3 cin -> C
    WInc inc[MAX_BL];         // .2.layers.l: conv0_0 C -> h, conv0_1 h -> h, conv1_0 1x1 C -> h, conv1_1 h -> h, conv1_2 1x1 h -> h
    int64_t b_w, b_b;         // .3  conv3 C -> C
};
struct WLayout {
    int C, BL;
    int64_t sce_end;                                 // the scale context's parameters: [0, sce_end)
    WBlock block_in;
    int64_t h0_w[8], h0_b[8], h2_w[8], h2_b[8];      // inner_mlps.k.0: Linear(C, 24), Linear(24, 1)
    int64_t pr_w[8], pr_b[8];                        // prune_blocks.k.0.conv: conv3 C -> C
    WBlock outter[7];
    int64_t total;
};

static inline void wlayout_block(WBlock& b, int cin, int C, int nl, int64_t& cur) {
    const int h = C / 2;
    b.cin = cin; b.nl = nl;
    b.a_w = take(cur, 27 * cin * C); b.a_b = take(cur, C);
    for (int l = 0; l < nl; ++l) {
        WInc& q = b.inc[l];
        q.c00_w = take(cur, 27 * C * h); q.c00_b = take(cur, h);
        q.c01_w = take(cur, 27 * h * h); q.c01_b = take(cur, h);
        q.c10_w = take(cur, C * h);      q.c10_b = take(cur, h);
        q.c11_w = take(cur, 27 * h * h); q.c11_b = take(cur, h);
        q.c12_w = take(cur, h * h);      q.c12_b = take(cur, h);
    }
    b.b_w = take(cur, 27 * C * C); b.b_b = take(cur, C);
}

// the scale context leads the flat order at every width (layout.h: the 8-wide layout up to its block_in)
static inline bool make_wlayout(WLayout& W, int S, int BL, int C) {
    Layout L8;
    if ((C != 16 && C != 32) || !make_layout(L8, S, 1) || BL < 1 || BL > MAX_BL) return false;
    W.C = C; W.BL = BL;
    int64_t cur = L8.block_in.a_w;
    W.sce_end = cur;
    wlayout_block(W.block_in, 8, C, BL, cur);
    for (int k = 0; k < 8; ++k) {
        W.h0_w[k] = take(cur, 24 * C); W.h0_b[k] = take(cur, 24);
        W.h2_w[k] = take(cur, 24);     W.h2_b[k] = take(cur, 1);
    }
    for (int k = 0; k < 8; ++k) { W.pr_w[k] = take(cur, 27 * C * C); W.pr_b[k] = take(cur, C); }
    for (int k = 0; k < 7; ++k) wlayout_block(W.outter[k], k + 1, C, 1, cur);
    W.total = cur;
    return true;
}

static inline size_t wup256(size_t v) { return (v + 255) & ~(size_t)255; }

// up to 4 consecutive blocks of an arena as the host array of device pointers the wide entries take: block r's first row is
// blocks + r * block_bytes + one 32-byte zero row
struct WPtrs {
    float* p[4];
    WPtrs() { for (int i = 0; i < 4; ++i) p[i] = nullptr; }
    WPtrs(char* blocks, size_t block_bytes, int role, int count) {
        for (int i = 0; i < 4; ++i) p[i] = i < count ? (float*)(blocks + (size_t)(role + i) * block_bytes) + 8 : nullptr;
    }
    const float* const* in() const { return p; }
    float* const* out() const { return p; }
};

// what the forward launches read of a frame that has passed linr_frame_layout: its matrices, the map's leading dimension
static inline int wide_frame_matrices_check(const linr_frame* f) {
    if (f->rows > 0) {
        if (!f->nbr_lo || !f->nbr_mask || !f->offset_feat || !f->occ) return LINR_EINVAL;
        if (f->nbr_ld < f->rows || !linr_cmap_fits32(f->nbr_ld)) return LINR_EINVAL;
        if (!linr_aligned16(f->occ)) return LINR_EALIGN;
    }
    return 0;
}
