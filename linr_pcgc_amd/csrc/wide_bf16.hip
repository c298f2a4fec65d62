// bf16 / uint8-weight inference executor for hidden_channel_conv = 16 / 32 (main.py:520; the channel-blocked network of
// linr_pcgc_amd/wide_net.py), BASELINE config[4]'s numerics at the wider widths - the rule of csrc/net_bf16.hip:
//   * the model is its uint8 codes, de-quantised as w = q / 255 * (max - min) + min in fp32 (dequant_code, bit-exact with
//     quant_uniform2's reconstruction); every 3x3x3 kernel is rounded to bf16 (RNE) once, products are accumulated in fp32;
//   * biases, the pointwise convolutions conv1_0 / conv1_2, the scale-context MLP, the head MLP (C -> 24 -> 1), sigmoid and the bits are
//     fp32 on the de-quantised fp32 parameters;
//   * every matrix that is stored is bf16 and every consumer sees the stored value: x_low, per block A, H (both halves), M, I, the
//     ResNetBlock's extra-skip sum (block_layers > 1), the block output O / x_glob and the prior bf16(o + x_glob); the prune convolution's
//     output goes into the head MLP unrounded.
// Activations are channel-blocked: a C-wide matrix is C / 8 bf16 [1 + rows][8] blocks (zero row in front), `bs` elements apart.
//
// Kernels (the Python schedule, WideNet.forward_bf16, launches them one layer at a time - encoder and stage-serial decoder run the same
// launches, so their probabilities are bit-identical):
//   wprep_k    one launch per call: the fp32 copy of every parameter and, for every 3x3x3 convolution, its bf16 A-operand image
//   wconv16_k  a 3x3x3 convolution Ci -> Co on v_mfma_f32_4x4x4_16b_bf16 with CBSZ = 4: the lane's row is the N column of its 4x4 block,
//              B = four input channels of the gathered row, A = a 4 cout x 4 cin weight block broadcast from block ABID of a register
//              the wave reads from the LDS copy of the image.  Every input block of a row is gathered once per tap and feeds all Co
//              outputs.  Epilogues: bias, ReLU, the residual and the extra skip (bf16 rows), the Inception layer's pointwise conv1_0
//              (behind conv0_0) and conv1_2 (behind conv1_1), or the occupancy head (prune convolution + MLP + sigmoid + the stage's
//              bits partials).
// Inference only: nothing is kept for a backward pass.
#include "bf16_common.h"
#include "prof.h"

// ---- prologue ------------------------------------------------------------------------------------------------------------------
// Image of a convolution (kernel [27][cin][co], ME layout): combos c = s * NC + cq * (co / 4) + oq (s = the step of the tap loop, tap
// LINR_TAP(s); cq = input channel quad over ceil(cin / 8) * 8 channels; oq = output quad), NC = (cinp / 4) (co / 4); groups of 16 combos,
// one uint2 per lane: block (lane >> 2) of group g is combo 16 g + (lane >> 2), lane i = lane & 3 holds A[i][kk] = W[tap][4 cq + kk][4 oq + i]
// (zero for ci >= cin and past the last combo).
static inline int64_t wimg_elems(int cin, int co) {
    const int64_t nc = (int64_t)2 * ((cin + 7) / 8) * (co / 4);
    return (27 * nc + 15) / 16 * 64;
}

__global__ __launch_bounds__(LINR_BLOCK) void wprep_k(const uint8_t* __restrict__ codes, int64_t n_params, float range, float minv,
                                                     float* __restrict__ pf, const int64_t* __restrict__ tab, int n_conv, int64_t n_img,
                                                     uint2* __restrict__ img) {
    const int64_t t = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (t < n_params) {
        pf[t] = dequant(codes, t, range, minv);
        return;
    }
    const int64_t u = t - n_params;
    if (u >= n_img) return;
    int lo = 0, hi = n_conv - 1;                        // the last convolution whose image starts at or before u
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid * 4 + 3] <= u) lo = mid; else hi = mid - 1;
    }
    const int64_t w = tab[lo * 4];
    const int cin = (int)tab[lo * 4 + 1], co = (int)tab[lo * 4 + 2];
    const int64_t e = u - tab[lo * 4 + 3];
    const int nqo = co / 4, nc = 2 * ((cin + 7) / 8) * nqo;
    const int l = (int)(e & 63), c = (int)(e >> 6) * 16 + (l >> 2), i = l & 3;
    unsigned v[4] = {0u, 0u, 0u, 0u};
    if (c < 27 * nc) {
        const int s = c / nc, loc = c % nc, cq = loc / nqo, oq = loc % nqo, k = LINR_TAP(s);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int ci = 4 * cq + kk;
            if (ci < cin) v[kk] = f2bf(dequant(codes, w + ((int64_t)k * cin + ci) * co + 4 * oq + i, range, minv));
        }
    }
    img[u] = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
}

extern "C" int64_t linr_wide_bf16_image_elems(int32_t cin, int32_t cout) {
    if (cin < 1 || cin > 32 || (cout != 8 && cout != 16 && cout != 32)) return LINR_EINVAL;
    return wimg_elems(cin, cout);
}

extern "C" int linr_wide_bf16_prep(const uint8_t* codes, int64_t n_params, float min_param, float max_param, const int64_t* conv_tab,
                                   int32_t n_conv, int64_t n_img, float* pf, void* img, void* stream) {
    if (!codes || !pf || n_params < 1 || n_conv < 0 || n_img < 0 || (n_img > 0 && (!img || !conv_tab || n_conv < 1))) return LINR_EINVAL;
    if (((uintptr_t)img) & 15u) return LINR_EALIGN;
    const float range = max_param - min_param;                 // fp32 subtraction, like ten_range (csrc/net_bf16.hip)
    const int64_t total = n_params + n_img;
    wprep_k<<<linr_grid(total, LINR_BLOCK), LINR_BLOCK, 0, (hipStream_t)stream>>>(codes, n_params, range, min_param, pf, conv_tab, n_conv,
                                                                                  n_img, reinterpret_cast<uint2*>(img));
    return linr_launch_rc();
}

// ---- convolution ---------------------------------------------------------------------------------------------------------------
enum { WE_PLAIN = 0, WE_PW1 = 1, WE_PW2 = 2, WE_HEAD = 3 };
struct WArgs {
    const bf16_t* in; int64_t ibs;                 // input block 0 (first row; its zero row in front), block stride (elements)
    bf16_t* out; int64_t obs;
    const bf16_t* res; int64_t rbs;                // PLAIN: + res (before the ReLU);  PW2: the residual x's upper half
    const bf16_t* res2; int64_t r2bs;              // + the stored value of res2 after the rounding (the ResNetBlock's extra skip)
    const int32_t* lo; const uint32_t* mask; int64_t ld, n;
    const uint2* img; const float* bias;           // the convolution's image and fp32 bias [Co]
    const float* pw_w; const float* pw_b;          // PW1: conv1_0 [Ci][Co];  PW2: conv1_2 [Co][Co] (ME layout)
    int relu;
    const float *h_w1, *h_b1, *h_w2, *h_b2;        // HEAD: Linear(Co, 24) [24][Co], [24]; Linear(24, 1) [24], [1]
    const float* target; int64_t t_col;            // HEAD: occupancy column (fp32 [n][8]) or NULL
    float* p_out; double* partial;                 // HEAD: p [n]; per-workgroup nats or NULL
};

// NBI input blocks, CO output channels; grid: one 256-row workgroup per 256 rows, 2 waves per SIMD (the image in LDS is at most 54 KB)
template <int NBI, int CO, int EPI>
__global__ __launch_bounds__(LINR_BLOCK, 2) void wconv16_k(WArgs a) {
    constexpr int NQO = CO / 4;
    constexpr int NC = 2 * NBI * NQO;                        // weight blocks per tap
    constexpr int NGT = (27 * NC + 15) / 16;                 // register groups of the image
    constexpr int NGS = NC >= 16 ? NC / 16 : 1;              // groups per step
    constexpr int PF = NBI >= 4 ? 1 : (NBI == 2 ? 2 : 4);    // steps of gathers in flight ahead
    __shared__ uint4 wl[NGT * 32];
    {
        const uint4* src = reinterpret_cast<const uint4*>(a.img);
        for (int e = threadIdx.x; e < NGT * 32; e += LINR_BLOCK) wl[e] = src[e];
    }
    const int lane = threadIdx.x & 63;
    const int64_t row_raw = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    const bool live = row_raw < a.n;
    const int64_t row = live ? row_raw : a.n - 1;              // every lane stays in the MFMAs (they ignore EXEC)
    uint32_t off[27];
    decode_offsets16(a.lo, a.mask, a.ld, row, off);
    f32x4 acc[NQO];
#pragma unroll
    for (int q = 0; q < NQO; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[q][j] = a.bias[4 * q + j];
    const char* pad = reinterpret_cast<const char*>(a.in - 8);
    const int64_t bsb = a.ibs * 2;
    uint4 x[PF + 1][NBI];
#pragma unroll
    for (int u = 0; u < PF; ++u)
#pragma unroll
        for (int b = 0; b < NBI; ++b) x[u][b] = *reinterpret_cast<const uint4*>(pad + b * bsb + off[LINR_TAP(u)]);
    __syncthreads();                                            // the image is in LDS
    const uint2* wl2 = reinterpret_cast<const uint2*>(wl);
    s16x4 wc[NGS], wn[NGS];
#pragma unroll
    for (int j = 0; j < NGS; ++j) wc[j] = __builtin_bit_cast(s16x4, wl2[j * 64 + lane]);
    __builtin_amdgcn_sched_barrier(0);
    sfor<27>([&](auto kc) {
        constexpr int kk = decltype(kc)::value;
        if constexpr (kk + PF < 27) {
#pragma unroll
            for (int b = 0; b < NBI; ++b)
                x[(kk + PF) % (PF + 1)][b] = *reinterpret_cast<const uint4*>(pad + b * bsb + off[LINR_TAP(kk + PF)]);
        }
        if constexpr (kk + 1 < 27) {
            constexpr int g1 = ((kk + 1) * NC) / 16;
#pragma unroll
            for (int j = 0; j < NGS; ++j) wn[j] = __builtin_bit_cast(s16x4, wl2[(g1 + j) * 64 + lane]);
        }
        __builtin_amdgcn_sched_barrier(0);
        constexpr int g0 = (kk * NC) / 16;
        sfor<NBI>([&](auto bc) {
            constexpr int b = decltype(bc)::value;
            const uint4 r = x[kk % (PF + 1)][b];
            const s16x4 q0 = __builtin_bit_cast(s16x4, make_uint2(r.x, r.y));
            const s16x4 q1 = __builtin_bit_cast(s16x4, make_uint2(r.z, r.w));
            sfor<NQO>([&](auto oc) {
                constexpr int oq = decltype(oc)::value;
                constexpr int c0 = kk * NC + (2 * b) * NQO + oq, c1 = c0 + NQO;
                acc[oq] = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(wc[c0 / 16 - g0], q0, acc[oq], 4, c0 % 16, 0);
                acc[oq] = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(wc[c1 / 16 - g0], q1, acc[oq], 4, c1 % 16, 0);
            });
        });
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (kk + 1 < 27) {
#pragma unroll
            for (int j = 0; j < NGS; ++j) wc[j] = wn[j];
        }
    });
    if constexpr (EPI == WE_HEAD) {
        // ---- occupancy head on the fp32 accumulators (the prune convolution's output is never rounded) -------------------------
        // (every store comes behind the MLP, so its uniform weight loads stay scalar loads: see bconv_k MODE 1)
        float c[CO];
#pragma unroll
        for (int q = 0; q < NQO; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) c[4 * q + j] = acc[q][j];
        float z = a.h_b2[0];
#pragma unroll 4
        for (int o = 0; o < 24; ++o) {
            float h = a.h_b1[o];
#pragma unroll
            for (int i = 0; i < CO; ++i) h = fmaf(c[i], a.h_w1[o * CO + i], h);
            z = fmaf(fmaxf(h, 0.0f), a.h_w2[o], z);
        }
        const float p = 1.0f / (1.0f + expf(-z));
        float t = 0.0f;
        if (a.partial != nullptr && live) t = a.target[a.t_col + row * 8];
        if (live) a.p_out[row] = p;
        if (a.partial != nullptr) {
            __shared__ double sred[LINR_BLOCK / 64];
            double nats = 0.0;
            if (live) nats = (double)((t - 1.0f) * fmaxf(logf(1.0f - p), -100.0f) - t * fmaxf(logf(p), -100.0f));
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) nats += __shfl_xor(nats, d, 64);
            if (lane == 0) sred[threadIdx.x >> 6] = nats;
            __syncthreads();
            if (threadIdx.x == 0) {
                double tot = sred[0];
                for (int w = 1; w < LINR_BLOCK / 64; ++w) tot += sred[w];
                a.partial[blockIdx.x] = tot;
            }
        }
        return;
    } else {
        if (!live) return;
        float o[CO];
#pragma unroll
        for (int q = 0; q < NQO; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) o[4 * q + j] = acc[q][j];
        if constexpr (EPI == WE_PLAIN) {
            if (a.res != nullptr) {
#pragma unroll
                for (int ob = 0; ob < CO / 8; ++ob) {
                    float r[8];
                    unpack_row(*reinterpret_cast<const uint4*>(a.res + ob * a.rbs + row * 8), r);
#pragma unroll
                    for (int j = 0; j < 8; ++j) o[8 * ob + j] += r[j];
                }
            }
            if (a.relu) {
#pragma unroll
                for (int j = 0; j < CO; ++j) o[j] = fmaxf(o[j], 0.0f);
            }
        } else if constexpr (EPI == WE_PW1) {
            // H = [relu(conv0_0) | relu(conv1_0 of the row itself)]: the second half goes to blocks CO / 8 .. 2 CO / 8 - 1 of out
            float xs[8 * NBI], h1[CO];
#pragma unroll
            for (int b = 0; b < NBI; ++b) {
                float r[8];
                unpack_row(*reinterpret_cast<const uint4*>(a.in + b * a.ibs + row * 8), r);
#pragma unroll
                for (int j = 0; j < 8; ++j) xs[8 * b + j] = r[j];
            }
#pragma unroll
            for (int j = 0; j < CO; ++j) h1[j] = a.pw_b[j];
#pragma unroll
            for (int i = 0; i < 8 * NBI; ++i)
#pragma unroll
                for (int j = 0; j < CO; ++j) h1[j] = fmaf(xs[i], a.pw_w[i * CO + j], h1[j]);
#pragma unroll
            for (int j = 0; j < CO; ++j) { o[j] = fmaxf(o[j], 0.0f); h1[j] = fmaxf(h1[j], 0.0f); }
#pragma unroll
            for (int ob = 0; ob < CO / 8; ++ob) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = h1[8 * ob + j];
                *reinterpret_cast<uint4*>(a.out + (CO / 8 + ob) * a.obs + row * 8) = pack_row(v);
            }
        } else {
            // I_hi = conv1_2(M) + x_hi with M = bf16(relu(conv1_1)), the value a stored M would have
            float m[CO], i1[CO];
#pragma unroll
            for (int j = 0; j < CO; ++j) { m[j] = bf2f(f2bf(fmaxf(o[j], 0.0f))); i1[j] = a.pw_b[j]; }
#pragma unroll
            for (int i = 0; i < CO; ++i)
#pragma unroll
                for (int j = 0; j < CO; ++j) i1[j] = fmaf(m[i], a.pw_w[i * CO + j], i1[j]);
#pragma unroll
            for (int ob = 0; ob < CO / 8; ++ob) {
                float r[8];
                unpack_row(*reinterpret_cast<const uint4*>(a.res + ob * a.rbs + row * 8), r);
#pragma unroll
                for (int j = 0; j < 8; ++j) o[8 * ob + j] = i1[8 * ob + j] + r[j];
            }
        }
        if (a.res2 != nullptr) {
#pragma unroll
            for (int ob = 0; ob < CO / 8; ++ob) {
                float r[8];
                unpack_row(*reinterpret_cast<const uint4*>(a.res2 + ob * a.r2bs + row * 8), r);
#pragma unroll
                for (int j = 0; j < 8; ++j) o[8 * ob + j] = bf2f(f2bf(o[8 * ob + j])) + r[j];
            }
        }
#pragma unroll
        for (int ob = 0; ob < CO / 8; ++ob) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = o[8 * ob + j];
            *reinterpret_cast<uint4*>(a.out + ob * a.obs + row * 8) = pack_row(v);
        }
    }
}

template <int NBI, int CO, int EPI>
static int wlaunch(const WArgs& a, hipStream_t s) {
    linr_poison_hook(s, PK_BF16_INFER);
    wconv16_k<NBI, CO, EPI><<<linr_grid(a.n, LINR_BLOCK), LINR_BLOCK, 0, s>>>(a);
    return linr_launch_rc();
}

static int wdispatch(int epi, int nbi, int co, const WArgs& a, hipStream_t s) {
#define WCASE(E, NB, C) if (epi == E && nbi == NB && co == C) return wlaunch<NB, C, E>(a, s)
    WCASE(WE_PLAIN, 1, 8);  WCASE(WE_PLAIN, 1, 16); WCASE(WE_PLAIN, 1, 32); WCASE(WE_PLAIN, 2, 16); WCASE(WE_PLAIN, 4, 32);
    WCASE(WE_PLAIN, 2, 8);  WCASE(WE_PLAIN, 2, 32); WCASE(WE_PLAIN, 4, 16);
    WCASE(WE_PW1, 2, 8);    WCASE(WE_PW1, 4, 16);
    WCASE(WE_PW2, 1, 8);    WCASE(WE_PW2, 2, 16);
    WCASE(WE_HEAD, 2, 16);  WCASE(WE_HEAD, 4, 32);
#undef WCASE
    return LINR_EINVAL;
}

static bool al16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

extern "C" int linr_spconv_wide_bf16(int32_t epi, const uint16_t* in, int64_t in_bs, int32_t cin, const int32_t* lo, const uint32_t* mask,
                                     int64_t ld, int64_t n, const void* img, const float* bias, int32_t cout, const uint16_t* res, int64_t res_bs,
                                     const uint16_t* res2, int64_t res2_bs, const float* pw_w, const float* pw_b, int32_t relu, uint16_t* out,
                                     int64_t out_bs, void* stream) {
    if (n < 0) return LINR_EINVAL;
    if (n == 0) return 0;
    if (!in || !lo || !mask || !img || !bias || !out || ld < n || cin < 1 || cin > 32) return LINR_EINVAL;
    if (!linr_rows_fit32(n)) return LINR_EINVAL;
    const int nbi = (cin + 7) / 8;
    if ((epi == WE_PW1 || epi == WE_PW2) && (!pw_w || !pw_b)) return LINR_EINVAL;
    if (epi == WE_PW2 && !res) return LINR_EINVAL;
    if (epi == WE_HEAD) return LINR_EINVAL;
    const int64_t rows8 = 8 * (n + 1);                                              // a block's elements, zero row included
    if ((nbi > 1 && in_bs < rows8) || (cout > 8 && out_bs < rows8) || (res && cout > 8 && res_bs < rows8) ||
        (res2 && cout > 8 && res2_bs < rows8) || (epi == WE_PW1 && out_bs < rows8))
        return LINR_EINVAL;
    if (!al16(in) || !al16(out) || !al16(img) || (res && !al16(res)) || (res2 && !al16(res2)) || (in_bs & 7) || (out_bs & 7) ||
        (res_bs & 7) || (res2_bs & 7))
        return LINR_EALIGN;
    WArgs a = WArgs();
    a.in = reinterpret_cast<const bf16_t*>(in); a.ibs = in_bs;
    a.out = reinterpret_cast<bf16_t*>(out); a.obs = out_bs;
    a.res = reinterpret_cast<const bf16_t*>(res); a.rbs = res_bs;
    a.res2 = reinterpret_cast<const bf16_t*>(res2); a.r2bs = res2_bs;
    a.lo = lo; a.mask = mask; a.ld = ld; a.n = n;
    a.img = reinterpret_cast<const uint2*>(img); a.bias = bias; a.pw_w = pw_w; a.pw_b = pw_b; a.relu = relu;
    return wdispatch(epi, nbi, cout, a, (hipStream_t)stream);
}

extern "C" int linr_head_wide_bf16_fwd(const uint16_t* in, int64_t in_bs, int32_t C, const int32_t* lo, const uint32_t* mask, int64_t ld,
                                       int64_t n, const void* img, const float* bias, const float* w1, const float* b1, const float* w2,
                                       const float* b2, const float* target, int32_t t_col, float* p, double* partial, void* stream) {
    if (n < 0) return LINR_EINVAL;
    if (n == 0) return 0;
    if (!in || !lo || !mask || !img || !bias || !w1 || !b1 || !w2 || !b2 || !p || ld < n || (C != 16 && C != 32)) return LINR_EINVAL;
    if (partial && (!target || t_col < 0 || t_col > 7)) return LINR_EINVAL;
    if (!linr_rows_fit32(n) || in_bs < 8 * (n + 1)) return LINR_EINVAL;
    if (!al16(in) || !al16(img) || (in_bs & 7)) return LINR_EALIGN;
    WArgs a = WArgs();
    a.in = reinterpret_cast<const bf16_t*>(in); a.ibs = in_bs;
    a.lo = lo; a.mask = mask; a.ld = ld; a.n = n;
    a.img = reinterpret_cast<const uint2*>(img); a.bias = bias;
    a.h_w1 = w1; a.h_b1 = b1; a.h_w2 = w2; a.h_b2 = b2;
    a.target = target; a.t_col = t_col; a.p_out = p; a.partial = partial;
    return wdispatch(WE_HEAD, C / 8, C, a, (hipStream_t)stream);
}

// ---- scale context: x0 (8 wide at every width) on the width-8 executor's kernel ------------------------------------------------
extern "C" int linr_sce_fwd_bf16(const float* pf, const linr_frame* f, uint16_t* x0_padded, void* stream) {
    if (!pf || !x0_padded) return LINR_EINVAL;
    Layout L;
    if (const int rc = linr_frame_layout(f, 1, L)) return rc;          // the scale context leads the layout at every width
    BSce sa;
    linr_sce_table(f, L, sa);
    if (f->rows == 0) return 0;
    if (!f->offset_feat) return LINR_EINVAL;
    if (!al16(x0_padded)) return LINR_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    linr_poison_hook(s, PK_BF16_INFER);
    sce_bf16_k<<<linr_grid(f->rows, LINR_BLOCK), LINR_BLOCK, 0, s>>>(pf, f->offset_feat, sa, f->rows,
                                                                    reinterpret_cast<bf16_t*>(x0_padded) + 8);
    return linr_launch_rc();
}
