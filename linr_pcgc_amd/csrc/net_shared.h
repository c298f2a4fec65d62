// Launchers of csrc/net.hip that the bf16 training executor (csrc/train_bf16.hip) shares with the fp32 one.  Not part of the C-ABI.
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
        if (rows < nb) shortr.push_back({b, e, rows});          // (csrc/net.hip: short_push aborts if the kernel's table overflows)
    }
};
__attribute__((visibility("hidden")))
int linr_bwd_tail_launch(const linr_frame* f, const Layout& L, const float* P, const float* gx0, const float* hid, float* big,
                         float* gsum, int nb, const LinrShortRange* sh, int nsh, hipStream_t stream);
__attribute__((visibility("hidden")))
int linr_adam_step_launch(const Layout& L, float* params, const float* gsum, float* exp_avg, float* exp_avg_sq, double lr, int64_t step,
                          const int64_t* scale_steps_h, double beta1, double beta2, double eps, double weight_decay, hipStream_t s);
__attribute__((visibility("hidden"))) int linr_wg_blocks_for(int64_t rows);
// live kernel timing / poison hook of csrc/net.hip (include/linr_hip.h: linr_prof_*) around a launch of another file
struct LinrProf {
    void* impl;
    LinrProf(hipStream_t s, int kind, int passes);
    ~LinrProf();
    LinrProf(const LinrProf&) = delete;
    LinrProf& operator=(const LinrProf&) = delete;
};
