// linr_params_fake_quant_ranges_host (csrc/fake_quant.hip: the plain-loop twin of the range search's quantiser kernel, which indexes
// [K][stride] outputs) under AddressSanitizer + UBSan; no GPU is involved and nothing is launched.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       tools/fq_ranges_host_check.cpp linr_pcgc_amd/csrc/fake_quant.hip linr_pcgc_amd/csrc/prof.hip -o a.out && ./a.out 4000
// (host code only is instrumented; the device code of the two .hip files is compiled as ever and never runs)
// Every call gets heap buffers of exactly n floats in, K * stride floats / codes and 4 K counters out (a store behind any of them
// aborts), with every combination of the optional outputs; n around the multiples of 4, K in 1..16, stride = n rounded up to 4 plus
// 0..3 further groups, bit depths 2..16, ranges inside, at and outside the values' own, equal bounds among them, a NaN parameter now
// and then.  Checked beside the sanitizers: the padding of every row keeps its fill, codes stay within [0, 2^bitdepth - 1], the
// counters are the counts and sums of what was written, and the vector's own (min, max) gives what linr_params_fake_quant_host gives.
#include "../include/linr_hip.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

static std::mt19937_64 rng(20241019);

static void fail(const char* what, long n, long k, long a, long b) {
    fprintf(stderr, "FAIL %s: n = %ld, candidate %ld: %ld vs %ld\n", what, n, k, a, b);
    exit(1);
}

template <class T>
static T* exact(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }

int main(int argc, char** argv) {
    const long count = argc > 1 ? atol(argv[1]) : 4000;
    std::normal_distribution<float> normal(0.0f, 0.05f);
    long calls = 0;
    for (long it = 0; it < count; ++it) {
        const int64_t n = it % 7 == 0 ? 1 + (int64_t)(rng() % 9) : 1 + (int64_t)(rng() % 3000);
        const int K = 1 + (int)(rng() % 16);
        const int bitdepth = 2 + (int)(rng() % 15);
        const int64_t stride = ((n + 3) & ~(int64_t)3) + 4 * (int64_t)(rng() % 4);
        float* p = exact<float>(n);
        float mn = INFINITY, mx = -INFINITY;
        for (int64_t i = 0; i < n; ++i) {
            p[i] = normal(rng) * (rng() % 50 == 0 ? 40.0f : 1.0f);
            if (p[i] < mn) mn = p[i];
            if (p[i] > mx) mx = p[i];
        }
        float* r = exact<float>(2 * K);
        r[0] = mn; r[1] = mx;
        for (int k = 1; k < K; ++k) {
            float a = normal(rng) * 3.0f, b = normal(rng) * 3.0f;
            if (a > b) { float t = a; a = b; b = t; }
            if (k % 5 == 0) b = a;
            r[2 * k] = a; r[2 * k + 1] = b;
        }
        if (n > 2 && it % 11 == 0) p[rng() % n] = NAN;
        const int64_t sym_max = (1 << bitdepth) - 1;
        for (int variant = 0; variant < 4; ++variant) {
            float* q = exact<float>(K * stride);
            uint16_t* c = variant & 1 ? nullptr : exact<uint16_t>(K * stride);
            int64_t* st = variant & 2 ? nullptr : exact<int64_t>(4 * K);
            for (int64_t i = 0; i < K * stride; ++i) { q[i] = 7.0f; if (c) c[i] = 0xABCD; }
            int rc = linr_params_fake_quant_ranges_host(p, n, bitdepth, r, K, stride, q, c, st);
            if (rc) fail("return code", n, -1, rc, 0);
            ++calls;
            for (int k = 0; k < K; ++k) {
                int64_t below = 0, above = 0, sum = 0;
                for (int64_t i = 0; i < n; ++i) {
                    below += p[i] < r[2 * k];
                    above += p[i] > r[2 * k + 1];
                    if (c) { if (c[k * stride + i] > sym_max) fail("code out of range", n, k, c[k * stride + i], sym_max); sum += c[k * stride + i]; }
                }
                for (int64_t i = n; i < stride; ++i)
                    if (q[k * stride + i] != 7.0f || (c && c[k * stride + i] != 0xABCD)) fail("padding written", n, k, i, stride);
                if (st && (st[4 * k] != below || st[4 * k + 1] != above)) fail("counts", n, k, st[4 * k], below);
                if (st && c) {
                    if (st[4 * k + 2] != sum) fail("sum of the codes", n, k, st[4 * k + 2], sum);
                    const int64_t mu = (int64_t)rintf((float)sum / (float)n);
                    int64_t dev = 0;
                    for (int64_t i = 0; i < n; ++i) dev += llabs((long long)c[k * stride + i] - mu);
                    if (st[4 * k + 3] != dev) fail("sum of the deviations", n, k, st[4 * k + 3], dev);
                }
            }
            if (variant == 0 && n > 1 && it % 11) {          // the vector's own range: the plain quantiser
                float* q0 = exact<float>(n);
                uint16_t* c0 = exact<uint16_t>(n);
                if (linr_params_fake_quant_host(p, n, bitdepth, q0, c0, nullptr)) fail("plain quantiser", n, 0, 1, 0);
                if (memcmp(q0, q, n * sizeof(float)) || memcmp(c0, c, n * sizeof(uint16_t))) fail("own range differs from the plain quantiser", n, 0, 0, 0);
                free(q0); free(c0);
            }
            free(q); free(c); free(st);
        }
        free(p); free(r);
    }
    printf("%ld calls clean\n", calls);
    return 0;
}
