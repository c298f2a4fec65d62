// The overfit of a whole GOP as one call (include/linr_hip.h: linr_overfit_plan, linr_overfit_ws_bytes, linr_overfit_gop): the loop of
// main.py:297-437 - frames in fixed order, one optimiser and one StepLR step per frame, the learning-rate clamp after each epoch, the
// epoch with the lowest mean loss kept - queued on one stream with ONE synchronisation at its end.  The steps are the executors' own
// (csrc/net.hip, csrc/train_bf16.hip, csrc/wide_train.hip: the same launches with the same arguments as their C entries); what is new
// here is the host schedule (learning rate and step counts of every step follow from which frames hold which scales) and three small
// kernels per epoch that replace the host's reading of the loss: are the parameters finite, close the epoch (mean loss, is it the best
// so far), copy parameters and moments when it is.
#include "common.h"
#include "layout.h"
#include "bwd_tail.h"
#include "params_avg.h"
#include "prof.h"
#include <math.h>
#include <string.h>
#include <vector>

#define TRY(e) do { int rc_ = (e); if (rc_) return rc_; } while (0)

namespace {

// ---- device state ----------------------------------------------------------------------------------------------------------------------
struct OvState {
    double best_loss;        // lowest loss of a competing epoch so far, +inf: none
    int32_t best_epoch;      // its epoch, -1: none
    int32_t take;            // the epoch just closed is the best so far: snapshot_k copies
    int32_t finite;          // and-reduction of isfinite over the parameters (params_finite_k clears, epoch_close_k sets it again)
    int32_t has_best;        // an epoch was taken: the final restore copies
};
static_assert(sizeof(OvState) == 24, "OvState is read back as 24 bytes");

struct OvWs {                // byte offsets into the workspace, each 16-byte aligned
    size_t bits, pn, state, losses, snap, total;
    int64_t np4;             // floats of one snapshot buffer (n_params rounded up to a multiple of 4)
};
OvWs make_ws(int64_t n_params, int32_t n_frames, int32_t epochs) {
    OvWs w;
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    size_t cur = 0;
    w.bits = cur;   cur = up16(cur + 8 * (size_t)n_frames);
    w.pn = cur;     cur = up16(cur + 8 * (size_t)n_frames);
    w.state = cur;  cur = up16(cur + sizeof(OvState));          // state and losses are adjacent: one copy to the host
    w.losses = cur; cur = up16(cur + 8 * (size_t)epochs);
    w.np4 = (n_params + 3) & ~(int64_t)3;
    w.snap = cur;   cur += 3 * 4 * (size_t)w.np4;
    w.total = cur;
    return w;
}

#define OV_PN_CHUNK 32
struct OvPn { double v[OV_PN_CHUNK]; };

// point numbers (as kernel arguments: no host buffer has to outlive the call), zeroed bits and, with st, the starting state
__global__ __launch_bounds__(64) void overfit_init_k(double* bits, double* pn, int base, int count, OvPn p, OvState* st) {
    const int i = threadIdx.x;
    if (i < count) { pn[base + i] = p.v[i]; bits[base + i] = 0.0; }
    if (st && i == 0) {
        st->best_loss = INFINITY; st->best_epoch = -1; st->take = 0; st->finite = 1; st->has_best = 0;
    }
}

__device__ __forceinline__ bool ov_finite(uint32_t u) { return (u & 0x7f800000u) != 0x7f800000u; }

// and-reduction of isfinite over p[0, n) into *flag (1 before the launch): 16-byte loads over n / 4 quads, the tail element by element
__global__ __launch_bounds__(LINR_BLOCK) void params_finite_k(const float* __restrict__ p, int64_t n, int32_t* flag) {
    const int64_t n4 = n >> 2;
    const int64_t t = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * LINR_BLOCK;
    bool ok = true;
    const uint4* q = reinterpret_cast<const uint4*>(p);
    for (int64_t i = t; i < n4; i += stride) {
        const uint4 v = q[i];
        ok = ok && ov_finite(v.x) && ov_finite(v.y) && ov_finite(v.z) && ov_finite(v.w);
    }
    const int64_t j = (n4 << 2) + t;
    if (j < n) ok = ok && ov_finite(__float_as_uint(p[j]));
    if (!ok) atomicAnd(flag, 0);
}

// one workgroup: the epoch's mean loss (frame order, double), +inf when a parameter is not finite; is it the best competing epoch so
// far; bits zeroed and the flag set for the next epoch
__global__ __launch_bounds__(64) void epoch_close_k(double* bits, const double* __restrict__ pn, int n_frames, double* losses, int epoch,
                                                    int competes, OvState* st) {
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int j = 0; j < n_frames; ++j) sum += bits[j] / pn[j];
        double loss = sum / (double)n_frames;
        if (!st->finite) loss = INFINITY;
        st->finite = 1;
        losses[epoch] = loss;
        int take = 0;
        if (competes && loss < st->best_loss) {          // false for NaN and +inf: they never win, the first finite epoch always does
            take = 1;
            st->best_loss = loss; st->best_epoch = epoch; st->has_best = 1;
        }
        st->take = take;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < n_frames; j += 64) bits[j] = 0.0;
}

struct OvCopy { const float* src[3]; float* dst[3]; };
// dst[y] = src[y] over n floats for the three buffers (parameters, both moments) when *flag is set; returns at once otherwise
__global__ __launch_bounds__(LINR_BLOCK) void snapshot_k(const int32_t* __restrict__ flag, OvCopy c, int64_t n) {
    if (*flag == 0) return;
    const float* __restrict__ src = c.src[blockIdx.y];
    float* __restrict__ dst = c.dst[blockIdx.y];
    const int64_t n4 = n >> 2;
    const int64_t t = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * LINR_BLOCK;
    for (int64_t i = t; i < n4; i += stride) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
    const int64_t j = (n4 << 2) + t;
    if (j < n) dst[j] = src[j];
}

unsigned flat_grid(int64_t n) {
    const int64_t b = ((n >> 2) + LINR_BLOCK - 1) / LINR_BLOCK;
    return (unsigned)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

// ---- the schedule ------------------------------------------------------------------------------------------------------------------------
struct OvOpt {               // FlatAdam's host state
    int64_t step, sched;
    double lr;
    int64_t scale[MAX_SCALES];
};

int plan_frame_check(const linr_frame* f, int S) {
    if (!f || f->n_scales < 1 || f->n_scales > MAX_SCALES || !f->row_off_h || !f->scale_idx_h) return LINR_EINVAL;
    for (int j = 0; j < f->n_scales; ++j)
        if (f->scale_idx_h[j] < 0 || f->scale_idx_h[j] >= S) return LINR_EINVAL;
    return 0;
}

// the counters of the next update on frame f: scales that have rows in it start, started scales advance
void plan_advance(OvOpt& o, const linr_frame* f, int S) {
    bool present[MAX_SCALES] = {};
    for (int j = 0; j < f->n_scales; ++j)
        if (f->row_off_h[j + 1] > f->row_off_h[j]) present[f->scale_idx_h[j]] = true;
    for (int s = 0; s < S; ++s)
        if (present[s] || o.scale[s] > 0) o.scale[s] += 1;
    o.step += 1;
}

// o: the starting state, left as the state after the last epoch's clamp
int plan_core(const linr_frame* const* frames, int n_frames, int epochs, int S, OvOpt& o, int64_t step_size, double gamma, double min_lr,
              double* lr_out, int64_t* step_out, int64_t* scale_out, int64_t* end_step, int64_t* end_sched, double* end_lr,
              int64_t* end_scale) {
    if (!frames || n_frames < 1 || epochs < 0 || S < 1 || S > MAX_SCALES || step_size < 1) return LINR_EINVAL;
    for (int j = 0; j < n_frames; ++j) TRY(plan_frame_check(frames[j], S));
    for (int e = 0; e < epochs; ++e) {
        for (int j = 0; j < n_frames; ++j) {
            const int64_t k = (int64_t)e * n_frames + j;
            plan_advance(o, frames[j], S);
            if (lr_out) lr_out[k] = o.lr;
            if (step_out) step_out[k] = o.step;
            if (scale_out) for (int s = 0; s < S; ++s) scale_out[k * S + s] = o.scale[s];
            o.sched += 1;                                // StepLR.step(), chainable form: one multiply, so a clamp persists
            if (o.sched % step_size == 0) o.lr *= gamma;
        }
        if (end_step) end_step[e] = o.step;
        if (end_sched) end_sched[e] = o.sched;
        if (end_lr) end_lr[e] = o.lr;
        if (end_scale) for (int s = 0; s < S; ++s) end_scale[(int64_t)e * S + s] = o.scale[s];
        if (o.lr < min_lr) o.lr = min_lr;                // main.py:433-437
    }
    return 0;
}

void start_state(OvOpt& o, int64_t step, int64_t sched, double lr, const int64_t* scale_steps_h, int S) {
    o.step = step; o.sched = sched; o.lr = lr;
    for (int s = 0; s < MAX_SCALES; ++s) o.scale[s] = (scale_steps_h && s < S) ? scale_steps_h[s] : 0;
}

// one step of the chosen executor; dry: its checks only
int run_step(const linr_overfit_args& a, const linr_overfit_frame& fr, const linr_step_args& sa, void* stream, bool dry) {
    switch (a.executor) {
    case LINR_OVERFIT_F32:
        return linr_train_step_f32(fr.f, a.params, (float*)a.arena, a.arena_bytes, &sa, stream, dry);
    case LINR_OVERFIT_BF16:
        return linr_train_step_bf16(fr.f, a.params, a.arena, a.arena_bytes, fr.occ_bf16, &sa, stream, dry);
    default:
        return linr_train_step_wide(fr.f, a.params, a.hidden, a.arena, a.arena_bytes, a.flags, &sa, stream, dry);
    }
}

}  // namespace

extern "C" int linr_overfit_plan(const linr_frame* const* frames_h, int32_t n_frames, int32_t epochs, int32_t model_scale_num, int64_t step,
                                 int64_t sched_steps, double lr, const int64_t* scale_steps_h, int64_t step_size, double gamma,
                                 double min_lr, double* lr_out, int64_t* step_out, int64_t* scale_steps_out, int64_t* end_step,
                                 int64_t* end_sched, double* end_lr, int64_t* end_scale_steps) {
    if (model_scale_num < 1 || model_scale_num > MAX_SCALES) return LINR_EINVAL;
    OvOpt o;
    start_state(o, step, sched_steps, lr, scale_steps_h, model_scale_num);
    return plan_core(frames_h, n_frames, epochs, model_scale_num, o, step_size, gamma, min_lr, lr_out, step_out, scale_steps_out, end_step,
                     end_sched, end_lr, end_scale_steps);
}

extern "C" size_t linr_overfit_ws_bytes(int64_t n_params, int32_t n_frames, int32_t epochs) {
    if (n_params < 0 || n_frames < 0 || epochs < 0) return 0;
    return make_ws(n_params, n_frames, epochs).total;
}

// linr_overfit_gop (avg == NULL: to the letter) and linr_overfit_gop_avg (the averaging launch behind every step)
static int overfit_core(const linr_overfit_frame* frames, const linr_overfit_args* args, const linr_overfit_avg* avg,
                        linr_overfit_result* result, void* stream) {
    // ---- every check in front of the first launch ----
    if (!frames || !args || !result) return LINR_EINVAL;
    const linr_overfit_args& a = *args;
    if (!a.params || !a.exp_avg || !a.exp_avg_sq || !a.arena || !a.ws) return LINR_EINVAL;
    if (a.n_frames < 1) return LINR_EINVAL;
    for (int j = 0; j < a.n_frames; ++j)
        if (!frames[j].f) return LINR_EINVAL;
    if (a.epochs < 0 || (a.epochs > 0 && !result->losses_h)) return LINR_EINVAL;
    if (a.qat_from < 0 || a.qat_from > a.epochs) return LINR_EINVAL;
    if (a.qat_from < a.epochs && !a.qparams) return LINR_EINVAL;
    if (a.qparams && (a.bitdepth < 2 || a.bitdepth > 16)) return LINR_EINVAL;
    if (a.step_size < 1 || a.step < 0 || a.sched_steps < 0) return LINR_EINVAL;
    for (int j = 0; j < a.n_frames; ++j)
        if (!(frames[j].point_num > 0.0) || !isfinite(frames[j].point_num)) return LINR_EINVAL;
    int64_t n_params = 0;
    const linr_frame* f0 = frames[0].f;
    const int S = f0->model_scale_num, bl = f0->block_layers < 1 ? 1 : f0->block_layers;
    switch (a.executor) {
    case LINR_OVERFIT_F32:
    case LINR_OVERFIT_BF16:
        if (a.hidden != 8 || a.flags != 0) return LINR_EINVAL;
        n_params = linr_param_count(S, bl);
        break;
    case LINR_OVERFIT_WIDE:
        if ((a.hidden != 16 && a.hidden != 32) || (a.flags & ~LINR_MUL_BF16)) return LINR_EINVAL;
        n_params = linr_param_count_wide(S, bl, a.hidden);
        break;
    default:
        return LINR_EINVAL;
    }
    if (n_params < 1) return LINR_EINVAL;          // (a scale_num or depth the executor does not have)
    std::vector<const linr_frame*> fp(a.n_frames);
    for (int j = 0; j < a.n_frames; ++j) {
        fp[j] = frames[j].f;
        if (fp[j]->model_scale_num != S || (fp[j]->block_layers < 1 ? 1 : fp[j]->block_layers) != bl) return LINR_EINVAL;
    }
    if (!linr_aligned16(a.params) || !linr_aligned16(a.exp_avg) || !linr_aligned16(a.exp_avg_sq) || !linr_aligned16(a.ws)) return LINR_EALIGN;
    const OvWs w = make_ws(n_params, a.n_frames, a.epochs);
    if (a.ws_bytes < w.total) return LINR_ENOSPC;
    if (avg) {
        int rc = linr_params_average_check(a.params, n_params, avg->weight, avg->n_avg, avg->stride, avg->avg);
        if (rc < 0) return rc;
    }

    // the schedule
    const int64_t n_steps = (int64_t)a.epochs * a.n_frames;
    std::vector<double> lr(n_steps), end_lr(a.epochs);
    std::vector<int64_t> step(n_steps), scale(n_steps * S), end_step(a.epochs), end_sched(a.epochs), end_scale((int64_t)a.epochs * S);
    OvOpt last;
    start_state(last, a.step, a.sched_steps, a.lr, a.scale_steps_h, S);
    TRY(plan_core(fp.data(), a.n_frames, a.epochs, S, last, a.step_size, a.gamma, a.min_lr, lr.data(), step.data(), scale.data(),
                  end_step.data(), end_sched.data(), end_lr.data(), end_scale.data()));

    char* ws = (char*)a.ws;
    double* bits = (double*)(ws + w.bits);
    double* pn = (double*)(ws + w.pn);
    OvState* st = (OvState*)(ws + w.state);
    double* losses = (double*)(ws + w.losses);
    float* snap = (float*)(ws + w.snap);
    auto step_args = [&](int e, int j) {
        const int64_t k = (int64_t)e * a.n_frames + j;
        linr_step_args sa;
        sa.gscale = (float)(1.0 / frames[j].point_num);
        sa.exp_avg = a.exp_avg; sa.exp_avg_sq = a.exp_avg_sq;
        sa.lr = lr[k]; sa.step = step[k]; sa.scale_steps_h = scale.data() + k * S;
        sa.beta1 = a.beta1; sa.beta2 = a.beta2; sa.eps = a.eps; sa.weight_decay = a.weight_decay;
        sa.bits_acc = bits + j;
        sa.qparams = e >= a.qat_from ? a.qparams : nullptr;
        sa.bitdepth = a.bitdepth;
        return sa;
    };
    // every frame as its step entry checks it: the counters only grow, so the first plain and the first quantisation-aware epoch decide
    if (a.epochs > 0) {
        for (int j = 0; j < a.n_frames; ++j) TRY(run_step(a, frames[j], step_args(0, j), stream, true));
        if (a.qat_from > 0 && a.qat_from < a.epochs)
            for (int j = 0; j < a.n_frames; ++j) TRY(run_step(a, frames[j], step_args(a.qat_from, j), stream, true));
    }

    // ---- the launches ----
    hipStream_t s = (hipStream_t)stream;
    for (int base = 0; base < a.n_frames; base += OV_PN_CHUNK) {
        OvPn p;
        const int count = a.n_frames - base < OV_PN_CHUNK ? a.n_frames - base : OV_PN_CHUNK;
        for (int i = 0; i < OV_PN_CHUNK; ++i) p.v[i] = i < count ? frames[base + i].point_num : 1.0;
        ProfScope ps(s, PK_MISC, 0);
        overfit_init_k<<<1, 64, 0, s>>>(bits, pn, base, count, p, base == 0 ? st : nullptr);
    }
    TRY(linr_launch_rc());
    if (avg)          // the averages start from zero; what lies behind n_params in a row is left alone
        for (int k = 0; k < avg->n_avg; ++k) TRY(linr_hip_rc(hipMemsetAsync(avg->avg + k * avg->stride, 0, 4 * (size_t)n_params, s)));
    const OvCopy save = {{a.params, a.exp_avg, a.exp_avg_sq}, {snap, snap + w.np4, snap + 2 * w.np4}};
    const OvCopy restore = {{snap, snap + w.np4, snap + 2 * w.np4}, {a.params, a.exp_avg, a.exp_avg_sq}};
    const bool qat = a.qat_from < a.epochs;
    for (int e = 0; e < a.epochs; ++e) {
        for (int j = 0; j < a.n_frames; ++j) {
            TRY(run_step(a, frames[j], step_args(e, j), stream, false));
            if (avg) TRY(linr_params_average_launch(a.params, n_params, avg->weight, avg->n_avg, avg->stride, avg->avg, s));
        }
        {
            ProfScope ps(s, PK_MISC, 0);
            params_finite_k<<<flat_grid(n_params), LINR_BLOCK, 0, s>>>(a.params, n_params, &st->finite);
        }
        {
            ProfScope ps(s, PK_MISC, 0);
            epoch_close_k<<<1, 64, 0, s>>>(bits, pn, a.n_frames, losses, e, (a.keep_best && (!qat || e >= a.qat_from)) ? 1 : 0, st);
        }
        if (a.keep_best) {
            ProfScope ps(s, PK_MISC, 0);
            snapshot_k<<<dim3(flat_grid(n_params), 3), LINR_BLOCK, 0, s>>>(&st->take, save, n_params);
        }
        TRY(linr_launch_rc());
    }
    if (a.keep_best && a.epochs > 0) {          // on the device's own flag: only when an epoch was taken
        ProfScope ps(s, PK_MISC, 0);
        snapshot_k<<<dim3(flat_grid(n_params), 3), LINR_BLOCK, 0, s>>>(&st->has_best, restore, n_params);
        TRY(linr_launch_rc());
    }
    // state and losses are adjacent: one copy, the call's one synchronisation
    std::vector<double> host((w.losses - w.state) / 8 + a.epochs);
    TRY(linr_hip_rc(hipMemcpyAsync(host.data(), st, (w.losses - w.state) + 8 * (size_t)a.epochs, hipMemcpyDeviceToHost, s)));
    TRY(linr_hip_rc(hipStreamSynchronize(s)));
    OvState hs;
    memcpy(&hs, host.data(), sizeof(hs));
    for (int e = 0; e < a.epochs; ++e) result->losses_h[e] = host[(w.losses - w.state) / 8 + e];
    result->best_epoch = hs.best_epoch;
    result->best_loss = hs.best_loss;
    const int be = hs.best_epoch;
    if (a.keep_best && be >= 0 && be < a.epochs) {
        result->step = end_step[be]; result->sched_steps = end_sched[be]; result->lr = end_lr[be];
        if (result->scale_steps_h) for (int k = 0; k < S; ++k) result->scale_steps_h[k] = end_scale[(int64_t)be * S + k];
    } else {
        result->step = last.step; result->sched_steps = last.sched; result->lr = last.lr;
        if (result->scale_steps_h) for (int k = 0; k < S; ++k) result->scale_steps_h[k] = last.scale[k];
    }
    return 0;
}

extern "C" int linr_overfit_gop(const linr_overfit_frame* frames, const linr_overfit_args* args, linr_overfit_result* result, void* stream) {
    return overfit_core(frames, args, nullptr, result, stream);
}

extern "C" int linr_overfit_gop_avg(const linr_overfit_frame* frames, const linr_overfit_args* args, const linr_overfit_avg* avg,
                                    linr_overfit_result* result, void* stream) {
    return overfit_core(frames, args, avg, result, stream);
}
