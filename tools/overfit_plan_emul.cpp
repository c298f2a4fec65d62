// Host-only sanitizer check of linr_overfit_plan (csrc/overfit.hip): the schedule of the one-call overfit written into buffers of EXACTLY
// the documented sizes (heap allocations, so AddressSanitizer sees one element too many), against a plain restatement of
// FlatAdam.advance / scheduler_step / clamp_lr.  No GPU call is made: the executors' steps and the profiler, which overfit.hip links
// against, are stubs here and abort when reached.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -x hip tools/overfit_plan_emul.cpp \
//         linr_pcgc_amd/csrc/overfit.hip -o overfit_plan_emul && ./overfit_plan_emul
//
// Runs on a machine without a GPU (the HIP runtime is linked, never initialised).  Exit status 0 and "overfit_plan_emul: ok" on success.
#include "../linr_pcgc_amd/csrc/bwd_tail.h"
#include "../linr_pcgc_amd/csrc/prof.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

// ---- what overfit.hip links against, never reached by the plan ----
static int unreachable(const char* what) { fprintf(stderr, "overfit_plan_emul: %s was called\n", what); abort(); }
int linr_train_step_f32(const linr_frame*, float*, float*, size_t, const linr_step_args*, void*, bool) { return unreachable("the fp32 step"); }
int linr_train_step_bf16(const linr_frame*, float*, void*, size_t, const uint16_t*, const linr_step_args*, void*, bool) { return unreachable("the bf16 step"); }
int linr_train_step_wide(const linr_frame*, float*, int32_t, void*, size_t, uint32_t, const linr_step_args*, void*, bool) { return unreachable("the wide step"); }
extern "C" int64_t linr_param_count(int32_t, int32_t) { return unreachable("linr_param_count"); }
extern "C" int64_t linr_param_count_wide(int32_t, int32_t, int32_t) { return unreachable("linr_param_count_wide"); }
ProfScope::ProfScope(hipStream_t s_, int kind_, int) : s(s_), kind(kind_), live(false) { unreachable("ProfScope"); }
ProfScope::~ProfScope() {}

struct Frame {
    std::vector<int64_t> row_off;
    std::vector<int32_t> idx;
    linr_frame c;
    Frame(std::vector<int64_t> rows, std::vector<int32_t> scale_idx, int S) : row_off(rows.size() + 1, 0), idx(scale_idx), c() {
        for (size_t i = 0; i < rows.size(); ++i) row_off[i + 1] = row_off[i] + rows[i];
        c.rows = row_off.back(); c.n_scales = (int32_t)rows.size(); c.model_scale_num = S; c.block_layers = 1;
        c.row_off_h = row_off.data(); c.scale_idx_h = idx.data();
    }
};

static int fail(const char* what, long k) { fprintf(stderr, "overfit_plan_emul: %s differs at %ld\n", what, k); return 1; }

static int run_case(const std::vector<Frame*>& frames, int epochs, int S, int64_t step, int64_t sched, double lr, std::vector<int64_t> scale,
                    int64_t step_size, double gamma, double min_lr) {
    const int n = (int)frames.size();
    const size_t k = (size_t)epochs * n;
    std::vector<const linr_frame*> fp;
    for (Frame* f : frames) fp.push_back(&f->c);
    // exact sizes, each its own heap block
    double* lr_out = new double[k];
    int64_t* step_out = new int64_t[k];
    int64_t* scale_out = new int64_t[k * S];
    int64_t* end_step = new int64_t[epochs];
    int64_t* end_sched = new int64_t[epochs];
    double* end_lr = new double[epochs];
    int64_t* end_scale = new int64_t[(size_t)epochs * S];
    int bad = 0;
    if (linr_overfit_plan(fp.data(), n, epochs, S, step, sched, lr, scale.data(), step_size, gamma, min_lr, lr_out, step_out, scale_out, end_step,
                          end_sched, end_lr, end_scale) != 0)
        bad = fail("the return value", 0);
    // FlatAdam.advance / scheduler_step / clamp_lr, restated
    size_t at = 0;
    for (int e = 0; e < epochs && !bad; ++e) {
        for (int j = 0; j < n && !bad; ++j, ++at) {
            const Frame& f = *frames[j];
            std::vector<char> present(S, 0);
            for (size_t i = 0; i < f.idx.size(); ++i)
                if (f.row_off[i + 1] > f.row_off[i]) present[f.idx[i]] = 1;
            for (int s = 0; s < S; ++s)
                if (present[s] || scale[s] > 0) scale[s] += 1;
            step += 1;
            if (lr_out[at] != lr) bad = fail("lr", (long)at);
            if (step_out[at] != step) bad = fail("step", (long)at);
            for (int s = 0; s < S; ++s)
                if (scale_out[at * S + s] != scale[s]) bad = fail("scale_steps", (long)at);
            sched += 1;
            if (sched % step_size == 0) lr *= gamma;
        }
        if (end_step[e] != step || end_sched[e] != sched || end_lr[e] != lr) bad = fail("the epoch's end", e);
        for (int s = 0; s < S; ++s)
            if (end_scale[(size_t)e * S + s] != scale[s]) bad = fail("end_scale_steps", e);
        if (lr < min_lr) lr = min_lr;
    }
    delete[] lr_out; delete[] step_out; delete[] scale_out; delete[] end_step; delete[] end_sched; delete[] end_lr; delete[] end_scale;
    return bad;
}

int main() {
    int bad = 0;
    {   // frames that lack the coarsest scales, a scale with zero rows, a scale that first appears in frame 2; the clamp in epoch 1
        Frame a({50, 20, 0, 4}, {0, 1, 2, 3}, 5), b({30, 12}, {0, 1}, 5), c({20, 7, 3, 2, 1}, {0, 1, 2, 3, 4}, 5);
        bad |= run_case({&a, &b, &c}, 4, 5, 0, 0, 0.01, std::vector<int64_t>(5, 0), 2, 0.5, 4e-3);
        bad |= run_case({&a, &b, &c}, 3, 5, 96, 97, 3.7e-4, {96, 96, 90, 64, 0}, 32, 0.992, 4e-4);          // warm start
        bad |= run_case({&b}, 1, 5, 0, 0, 0.01, std::vector<int64_t>(5, 0), 1, 0.9, 0.0);
        bad |= run_case({&c, &a}, 0, 5, 0, 0, 0.01, std::vector<int64_t>(5, 0), 1, 0.9, 0.0);          // no epoch: nothing is written
    }
    {   // the largest model: 16 scales, every one its own frame
        std::vector<Frame*> fs;
        for (int s = 0; s < 16; ++s) fs.push_back(new Frame({(int64_t)(s + 1)}, {(int32_t)s}, 16));
        bad |= run_case(fs, 2, 16, 0, 0, 0.01, std::vector<int64_t>(16, 0), 5, 0.7, 1e-3);
        for (Frame* f : fs) delete f;
    }
    // refusals write nothing
    Frame good({5, 3}, {0, 1}, 5), wrong({5, 3}, {0, 5}, 5);
    const linr_frame* fp[2] = {&good.c, &wrong.c};
    double* one = new double[1];
    one[0] = -1.0;
    if (linr_overfit_plan(fp, 2, 1, 5, 0, 0, 0.01, nullptr, 32, 0.9, 1e-4, one, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != LINR_EINVAL ||
        linr_overfit_plan(fp, 1, 1, 17, 0, 0, 0.01, nullptr, 32, 0.9, 1e-4, one, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != LINR_EINVAL ||
        linr_overfit_plan(fp, 1, 1, 5, 0, 0, 0.01, nullptr, 0, 0.9, 1e-4, one, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != LINR_EINVAL ||
        linr_overfit_plan(nullptr, 1, 1, 5, 0, 0, 0.01, nullptr, 32, 0.9, 1e-4, one, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != LINR_EINVAL ||
        one[0] != -1.0)
        bad |= fail("a refusal", 0);
    if (linr_overfit_plan(fp, 1, 1, 5, 0, 0, 0.01, nullptr, 32, 0.9, 1e-4, one, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0 || one[0] != 0.01)
        bad |= fail("the smallest plan", 0);
    delete[] one;
    if (linr_overfit_ws_bytes(-1, 1, 1) != 0 || linr_overfit_ws_bytes(5, 1, 1) < 60 + 8 + 8 + 8) bad |= fail("linr_overfit_ws_bytes", 0);
    if (!bad) printf("overfit_plan_emul: ok\n");
    return bad;
}
