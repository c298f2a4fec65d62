// Internal helpers shared by the gfx950 kernels.  Not part of the C-ABI (include/linr_hip.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/linr_hip.h"

#define LINR_BLOCK 256
#define LINR_WAVE 64

static inline int linr_hip_rc(hipError_t e) { return e == hipSuccess ? 0 : (int)e; }
static inline int linr_launch_rc() { return linr_hip_rc(hipGetLastError()); }
// Order in which every 3x3x3 forward / backward-data convolution kernel visits its 27 taps: step kk handles tap
// LINR_TAP(kk) = dx-index (kk / 9) + 3 * dy-index ((kk / 3) % 3) + 9 * dz-index (kk % 3), i.e. x-slab by x-slab, inside a slab
// (dx,dy) column by column, the three dz taps of a column back to back.  In the x-major row order (z fastest) the dz neighbours
// of a column are consecutive rows and the three dy columns of a slab lie within a few dozen rows, so a 64-row tile reads
// each of its three ~3 KB neighbour regions once and then hits in the L1 for the other eight taps of the slab (pure gathers:
// 19.2 us per pass in ascending tap order, 17.6 column by column, 17.0 slab by slab - tools/gather_probe.hip; training step
// 2.216 -> 2.166 -> 2.135 ms).  The order is part of the arithmetic (fp32 accumulation order of every output): ALL kernels of
// that family use it - MFMA, VALU, gather-table reference, dual 4->4, shared occupancy conv, bf16 - which keeps them
// bit-identical to each other and the decoder to the encoder.
#define LINR_TAP(kk) (((kk) / 9) + 3 * (((kk) / 3) % 3) + 9 * ((kk) % 3))

static inline bool linr_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
// The gather kernels address rows with 32-bit byte offsets from the zero row in front of a matrix, so the n + 1 rows of row_bytes
// each (a power of two) must stay below 2^32: n < 2^27 - 1 for the 32-byte rows of an 8-channel fp32 matrix.  The frame of every
// executor is held to that bound (include/linr_hip.h: linr_frame.rows), the bf16 ones with their 16-byte rows included.
static inline bool linr_rows_fit32(int64_t n, int64_t row_bytes = 32) { return n < ((int64_t)1 << 32) / row_bytes - 1; }
// ... and the compressed kernel map: the kernels that have no 64-bit path read lo [9][ld] with 32-bit byte offsets,
// 9 * ld * 4 B < 2^32; the others pick the 32-bit path by the same test (conv_common.h, bf16_common.h: load_words16).
static inline bool linr_cmap_fits32(int64_t ld) { return ld < ((int64_t)1 << 26); }
static inline unsigned linr_grid(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// number of persistent blocks used by the two-pass reductions: enough to fill 256 CUs several times over,
// few enough that the partial slabs stay small.
static inline int linr_reduce_blocks(int64_t n, int rows_per_tile) {
    int64_t tiles = (n + rows_per_tile - 1) / rows_per_tile;
    int64_t nb = tiles < 512 ? tiles : 512;
    return (int)(nb < 1 ? 1 : nb);
}

// Destination of per-block partial weight gradients: element e of block b lands at base[b*block_stride + off + e].
// The network executor points this at one big [LINR_WG_BLOCKS][n_params] slab indexed by flat parameter offset, so
// ONE final pass sums every parameter's partials in fixed order (deterministic) - fused with Adam in the train step.
struct LinrWgradDst {
    float* base;
    int64_t block_stride;
    int64_t w_off;       // weight tensor offset
    int64_t b_off;       // bias offset
    int cin_valid;       // conv3 only: input channels actually present (<= kernel width)
};
struct LinrLinDst {      // pointwise layers: element (ci,co) at w_off + ci*ws_ci + co*ws_co, bias co at b_off + co
    float* base;
    int64_t block_stride;
    int64_t w_off;
    int ws_ci, ws_co;
    int64_t b_off;
};
// per-range Adam schedule (csrc/loss_optim.hip: adam_k); 16 = MAX_SCALES of the executor
struct LinrAdamRanges {
    int count;               // 0: none
    int64_t begin, len;      // range r = [begin + r*len, begin + (r+1)*len)
    int active[16];
    float step_size[16], bc2_sqrt[16];
};
// torch.optim.Adam's single-tensor update, the ONE definition every kernel that applies it uses (adam_k; the tail-fold experiments of
// round 4 used it too): the operations
// are pinned - separate multiplies and adds for the moments, one fused multiply-add for the step (what adam_k has compiled to since
// round 1) - so that the fused and the stand-alone path update parameters bit-identically whatever the surrounding code looks like.
__device__ __forceinline__ float linr_adam_update(float p, float grad, float& m, float& v, float step_size, float bc2_sqrt, float beta1,
                                                  float omb1, float beta2, float omb2, float eps, float wd) {
#pragma clang fp contract(off)
    const float g = fmaf(wd, p, grad);
    const float mi = m * beta1 + omb1 * g;           // exp_avg.mul_(beta1).add_(grad, alpha=1-beta1)
    const float vi = v * beta2 + (omb2 * g) * g;     // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
    m = mi;
    v = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    return fmaf(-step_size, mi / denom, p);
}
__attribute__((visibility("hidden")))
int linr_adam_launch(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double step_size,
                     double bc2_sqrt, double beta1, double beta2, double eps, double weight_decay,
                     const LinrAdamRanges* rg, hipStream_t s);
#define LINR_WG_BLOCKS 512   // persistent blocks of every weight-gradient kernel (2 per CU; sweep: tools/wg_blocks_sweep.sh)
#define LINR_TILE8T_SPARE 12 // all -1 groups behind a transposed tiled table (csrc/kmap.hip: linr_kmap_tile8t) for the prefetches of csrc/wgrad.hip

// Grouped launches: independent layers of equal shape (the 7 outter blocks, the 8 occupancy heads, whose inputs are the
// ground-truth occupancy and x_glob during overfitting / encoding) run as ONE launch with gridDim.y = groups.  Group g adds
// these ELEMENT offsets to the kernel's base pointers; a plain launch passes all zeros.  Per-row arithmetic is identical
// in grouped and plain launches, so the staged decoder (plain) reproduces the encoder (grouped) bit for bit.
// Grp is the kernels' side of this and is filled by the launchers alone: a caller describes every group with the launcher's
// typed struct below (one element per group, a plain launch is an array of one); the launcher takes the kernel's base pointers
// and slab offsets from element 0 and writes the differences of the others into the slots its kernel reads.  What a slot
// (e0..e6 above all) means is the business of the kernel and of the launcher next to it, nobody else names one.
#define LINR_MAXG 8
struct Grp {
    int64_t in[LINR_MAXG], w[LINR_MAXG], b[LINR_MAXG], res[LINR_MAXG], act[LINR_MAXG], out[LINR_MAXG];
    int64_t e0[LINR_MAXG], e1[LINR_MAXG], e2[LINR_MAXG], e3[LINR_MAXG], e4[LINR_MAXG], e5[LINR_MAXG], e6[LINR_MAXG];
    int64_t n[LINR_MAXG];      // > 0: the group's own row count (groups of unequal size: the scales of a frame)
};

// compressed kernel map of n rows: lo [9][ld], mask [ld]
struct LinrCmap { const int32_t* lo; const uint32_t* mask; int64_t ld, n; };

// ---- one group's operands, per launcher ---------------------------------------------------------------------------------------
// Pointers are the group's own matrices and parameter tensors; *_off are offsets into a row of the partial weight-gradient
// slab.  A pointer the launch does not use is NULL in every group.
struct ConvGroup {           // linr_cconv_launch: out = conv3(in; W) (+ bias) (+ res), masked by act > 0 with LINR_RELU_MASK
    const float *in, *W, *bias, *res, *act;
    float* out;
};
struct HeadFwdGroup {        // linr_cconv_head_launch: c_out = conv3(in; W) + bias, p_out = sigmoid(w2 . relu(w1 c + b1) + b2)
    const float *in, *W, *bias;
    float* c_out;
    const float *w1, *b1, *w2, *b2;
    const float* target;   // the group's occupancy column, or NULL (probabilities only)
    float* p_out;
    double* partial;       // [linr_grid(n, 256)] block partials of the bits, or NULL
};
struct HeadBwdGroup {        // linr_head_bwd_launch
    const float *c, *p, *target, *w1, *b1, *w2;
    float* gc;
    int64_t w1_off, b1_off, w2_off, b2_off;
};
struct ConvPwGroup {         // linr_conv_pw_fwd_launch: H = [relu(conv3(A; w00) + b00) | relu(A @ w10 + b10)]
    const float *A, *w00, *b00, *w10, *b10;
    float* H;
};
struct Dual44FwdGroup {      // linr_dual44_fwd_launch
    const float *H, *w01, *b01, *w11, *b11, *A, *w12, *b12;
    float *M, *I;
};
// backward of the two 4->4 convolutions of an Inception layer: linr_dual44_bwd_launch (gH alone; no offsets), linr_conv3_wgrad_dual44
// (the weight gradients alone; no w01 / w11 / gH), linr_dual44_bwd_wgrad_launch (both)
struct Dual44BwdGroup {
    const float *gI, *gM, *H, *w01, *w11;
    float* gH;
    int64_t w01_off, b01_off, w11_off, b11_off;
};
// backward of a conv 8->8 with input xin: linr_conv88_bwd_wgrad_launch (out = bwd(g; W) and the weight gradient), with w12 != NULL
// in every group also gM = (out[:, 4:8] @ w12^T) * (M > 0) and conv1_2's weight gradient; linr_conv_bwd_gm_launch (out and gM alone;
// no xin, no offsets)
struct Conv88BwdGroup {
    const float *g, *xin, *W;
    float* out;
    int64_t w_off, b_off;
    const float *w12, *M;
    float* gM;
    int64_t w12_off, b12_off;
};
// backward of conv0_0 8->4 | conv1_0 1x1 of an Inception layer with input A: linr_conv84_bwd_wgrad_launch (gA and both weight
// gradients), linr_conv_bwd_ga_launch (gA alone; A only as the ReLU mask, no offsets)
struct Conv84BwdGroup {
    const float *gH, *A, *gI, *w00, *w10;
    float* gA;
    int64_t w00_off, b00_off, w10_off, b10_off;
};
struct WgradGroup {          // linr_conv3_wgrad_mfma, linr_linear_wgrad_partial: the layer's input and its output gradient
    const float *in, *gout;
    int64_t w_off, b_off;
    int cin_live;          // conv3 only, > 0: input channels this group actually has (<= cin)
};

// ---- internal launchers shared with the network executor (C++ linkage, not exported) ---------------------------
// epilogue order of both: acc (+ bias) -> + res -> + old (LINR_ACCUM) -> * (act > 0) (LINR_RELU_MASK) -> ReLU
__attribute__((visibility("hidden")))
int linr_conv3_launch(bool bwd, const float* in, int in_ld, const int32_t* nbr, int64_t nbr_ld, int64_t n,
                      const float* W, const float* bias, int cin, int cout, const float* res, int res_ld,
                      const float* act, int act_ld, float* out, int out_ld, unsigned flags, hipStream_t s);
__attribute__((visibility("hidden")))
int linr_linear_launch(const float* in, int in_ld, int64_t n, const float* W, int ws_ci, int ws_co, const float* bias,
                       int cin, int cout, const float* res, int res_ld, const float* act, int act_ld, float* out,
                       int out_ld, unsigned flags, hipStream_t s);
__attribute__((visibility("hidden")))
int linr_conv3_wgrad_partial(const float* in, int in_ld, const float* gout, int gout_ld, const int32_t* nbr,
                             int64_t nbr_ld, int64_t n, int cin, int cout, LinrWgradDst d, int nblocks, unsigned flags,
                             hipStream_t s);
// The grouped launchers: g[0 .. ng) describes the groups, 1 <= ng <= LINR_MAXG (else LINR_EINVAL).  Those that write weight-gradient
// partials put element e of block b at big[b * block_stride + the group's offset + e].
// pointwise layers: element (ci, co) at w_off + ci * ws_ci + co * ws_co, bias co at b_off + co
__attribute__((visibility("hidden")))
int linr_linear_wgrad_partial(const WgradGroup* g, int ng, int in_ld, int gout_ld, int64_t n, int cin, int cout, float* big,
                              int64_t block_stride, int ws_ci, int ws_co, int nblocks, hipStream_t s);
__attribute__((visibility("hidden"))) int linr_lin_blocks(int64_t n);
__attribute__((visibility("hidden")))
int linr_linear_slab_reduce_launch(const float* slab, int nblocks, int64_t stride, int cin, int cout, float* gW, int ws_ci, int ws_co,
                                   float* gb, unsigned flags, hipStream_t s);
__attribute__((visibility("hidden")))
int linr_cconv_launch(bool bwd, LinrCmap m, const ConvGroup* g, int ng, int in_ld, int cin, int cout, int res_ld, int act_ld,
                      int out_ld, unsigned flags, hipStream_t s);
__attribute__((visibility("hidden")))
int linr_cconv_head_launch(LinrCmap m, const HeadFwdGroup* g, int ng, int target_ld, hipStream_t s);
// rows_written == nullptr: slab rows 0 .. nblocks - 1 are all written; otherwise only the active blocks' rows (see csrc/fused.hip)
__attribute__((visibility("hidden")))
int linr_head_bwd_launch(const HeadBwdGroup* g, int ng, int target_ld, float gscale, int64_t n, float* big, int64_t block_stride,
                         int nblocks, int* rows_written, hipStream_t s);
__attribute__((visibility("hidden")))
int linr_bits_finish_launch(const double* partial, int count, double* bits_acc, hipStream_t s);
__attribute__((visibility("hidden")))
int linr_dual44_fwd_launch(LinrCmap m, const Dual44FwdGroup* g, int ng, hipStream_t s);
__attribute__((visibility("hidden")))
int linr_dual44_bwd_launch(LinrCmap m, const Dual44BwdGroup* g, int ng, hipStream_t s);
__attribute__((visibility("hidden")))
int linr_conv_pw_fwd_launch(LinrCmap m, const ConvPwGroup* g, int ng, hipStream_t s);
__attribute__((visibility("hidden")))
int linr_conv_bwd_gm_launch(LinrCmap m, const Conv88BwdGroup* g, int ng, hipStream_t s);
__attribute__((visibility("hidden")))
int linr_conv_bwd_ga_launch(LinrCmap m, const Conv84BwdGroup* g, int ng, unsigned flags, hipStream_t s);
__attribute__((visibility("hidden")))
int linr_occ_conv7_launch(const float* occ, LinrCmap m, const float* P, const int64_t* w_off, const int64_t* b_off, float* out,
                          const int64_t* out_off, hipStream_t s);
// cin, cout: the kernel's width (a group with fewer live input channels says so in cin_live); tile8t: the transposed tiled
// table (csrc/wgrad.hip: spconv_wgrad_t_k), or NULL: indices from nbr
__attribute__((visibility("hidden")))
int linr_conv3_wgrad_mfma(const WgradGroup* g, int ng, int in_ld, int gout_ld, const int32_t* nbr, int64_t nbr_ld, int64_t n,
                          const int32_t* tile8t, int cin, int cout, float* big, int64_t block_stride, int nblocks, hipStream_t s);
__attribute__((visibility("hidden")))
int linr_fused_bwd_rows(int64_t n, int nb, int ngroups);
// The fused launches (csrc/fused_bwd.hip): backward-data + weight gradient from one gather.  rows_written == nullptr: rows
// 0 .. nb - 1 of the slab are all written; otherwise only the grid's rows, and *rows_written tells the caller how many.
__attribute__((visibility("hidden")))
int linr_conv88_bwd_wgrad_launch(LinrCmap m, const Conv88BwdGroup* g, int ng, float* big, int64_t block_stride, int nb,
                                 int* rows_written, hipStream_t s);
__attribute__((visibility("hidden")))
int linr_dual44_bwd_wgrad_launch(LinrCmap m, const Dual44BwdGroup* g, int ng, float* big, int64_t block_stride, int nb,
                                 int* rows_written, hipStream_t s);
__attribute__((visibility("hidden")))
int linr_conv84_bwd_wgrad_launch(LinrCmap m, const Conv84BwdGroup* g, int ng, unsigned flags, float* big, int64_t block_stride,
                                 int nb, int* rows_written, hipStream_t s);
// the weight gradients of both 4->4 convolutions from H, gI (ld gI_ld) and gM (ld gM_ld)
__attribute__((visibility("hidden")))
int linr_conv3_wgrad_dual44(const Dual44BwdGroup* g, int ng, int gI_ld, int gM_ld, const int32_t* nbr, int64_t nbr_ld, int64_t n,
                            const int32_t* tile8t, float* big, int64_t block_stride, int nblocks, hipStream_t s);

// csrc/occ_wgrad.hip: weight gradients of the first convolutions of the 7 outter blocks from one gather of the occupancy rows
__attribute__((visibility("hidden")))
int linr_occ_wgrad7_launch(const float* occ, const float* const* g, LinrCmap m, float* big, int64_t block_stride,
                           const int64_t* w_off, const int64_t* b_off, int nb, hipStream_t s, int* rows_written);

// ---- the levels of several frames back to back (the lock-step GOP decoder: csrc/kmap.hip, csrc/decode.hip) --------------------
// The segment table travels by value: off[i] = first row of segment i for i <= n_seg, INT32_MAX behind.  A row finds the bounds of
// its segment with LINR_DECODE_MAX_FRAMES uniform compares (empty segments drop out: the last start <= r and the first start > r).
struct LinrSegTab { int32_t off[LINR_DECODE_MAX_FRAMES + 1]; };

__device__ __forceinline__ void linr_seg_bounds(const LinrSegTab& t, int32_t r, int32_t& lo, int32_t& hi) {
    lo = 0;
    hi = INT32_MAX;
#pragma unroll
    for (int i = 1; i <= LINR_DECODE_MAX_FRAMES; ++i) {
        const int32_t v = t.off[i];          // non-decreasing
        lo = v <= r ? v : lo;
        hi = (v > r && v < hi) ? v : hi;
    }
}
// HOST offsets -> by-value table (csrc/kmap.hip); LINR_EINVAL unless 1 <= n_seg <= LINR_DECODE_MAX_FRAMES and the offsets rise from
// 0 to *n < 2^31 - 1
__attribute__((visibility("hidden"))) int linr_seg_tab(const int64_t* seg_off_h, int32_t n_seg, LinrSegTab* tab, int64_t* n);
