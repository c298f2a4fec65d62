// Launchers of csrc/bwd_tail.hip: the end of a backward pass, shared by the fp32 executor (csrc/net.hip), the bf16 training executor
// (csrc/train_bf16.hip) and the op-level entries of csrc/fused.hip and csrc/wide.hip.  Not part of the C-ABI.
#pragma once
#include "common.h"
#include "layout.h"
#include <vector>

struct LinrShortRange { int64_t b, e; int rows; };     // parameters [b, e) hold partials in the first `rows` slab rows only
// Base of both training executors' contexts: a fused launch writes only `rows` slab rows for parameters [b, e) (no zero fill), the
// final reduction stops there.  The table holds every such range of a backward pass: 8 blocks x 2 + the prune convs + block_in's
// first conv + the 7 outter first convs + up to 16 scale-context MLPs = 41
struct LinrShortList {
    int nb;                  // persistent blocks of the weight-gradient kernels = partial rows of the slab for this frame
    std::vector<LinrShortRange> shortr;
    void note_short(int64_t b, int64_t e, int rows) {
        if (rows < nb) shortr.push_back({b, e, rows});          // (csrc/bwd_tail.hip: short_push aborts if the kernel's table overflows)
    }
};
__attribute__((visibility("hidden"))) int linr_wg_blocks_for(int64_t rows);
__attribute__((visibility("hidden")))
int linr_bwd_tail_launch(const linr_frame* f, const Layout& L, const float* P, const float* gx0, const float* hid, float* big,
                         float* gsum, int nb, const LinrShortRange* sh, int nsh, hipStream_t stream);
__attribute__((visibility("hidden")))
int linr_slab_reduce_launch(const float* big, int nblocks, int64_t total, float* gsum, hipStream_t s);
__attribute__((visibility("hidden")))
// L: the layout whose scale context leads the flat order (at every width: layout.h, wide_layout.h) - its MLPs take their own step counts
// from a.scale_steps_h; total: all parameters of the model (L.total at width 8, linr_param_count_wide at 16 / 32), the rest use a.step
int linr_adam_step_launch(const Layout& L, int64_t total, float* params, const float* gsum, const linr_step_args& a, hipStream_t s);
// The three training steps behind their C entries (csrc/net.hip, csrc/train_bf16.hip, csrc/wide_train.hip).  dry: every check of the
// entry in its order and no launch - linr_overfit_gop (csrc/overfit.hip) checks a whole GOP in front of its first launch.
__attribute__((visibility("hidden")))
int linr_train_step_f32(const linr_frame* f, float* params, float* arena, size_t arena_bytes, const linr_step_args* a, void* stream,
                        bool dry);
__attribute__((visibility("hidden")))
int linr_train_step_bf16(const linr_frame* f, float* params, void* arena, size_t arena_bytes, const uint16_t* occ_bf16,
                         const linr_step_args* a, void* stream, bool dry);
__attribute__((visibility("hidden")))
int linr_train_step_wide(const linr_frame* f, float* params, int32_t hidden, void* arena, size_t arena_bytes, uint32_t flags,
                         const linr_step_args* a, void* stream, bool dry);
