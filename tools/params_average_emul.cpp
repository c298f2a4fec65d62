// The host twin of the averaging kernel (linr_params_average_host, csrc/params_avg_host.cpp - the definition of what
// csrc/params_avg.hip computes) on the HOST under AddressSanitizer + UBSan; no GPU is involved and nothing is launched.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/params_average_emul.cpp \
//       linr_pcgc_amd/csrc/params_avg_host.cpp -o a.out && ./a.out
// The parameters sit in a heap buffer of exactly 4 n bytes, the weights in one of exactly 4 K, the averages in one of exactly
// 4 ((K - 1) stride + n) bytes - the last row has no padding at all, so a read or write at or behind any end aborts.  Checked, for
// n in {1, 3, 4, 5, 1023, 1024, 1025, 54712}, K in {1, 4} and strides n rounded up to 4 and + 8, over 5 chained updates: every element
// against this file's own restatement in double (within one fp32 ulp; bit for bit for +-0, inf and NaN classes), the padding of
// the rows before the last untouched, w = 1 copying the parameters into a zero average, and every refusal writing nothing.
#include "../include/linr_hip.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static std::mt19937_64 rng(20261021);
static long checked = 0;

static void fail(const char* what, long n, long k, long i) {
    fprintf(stderr, "FAIL %s (n %ld, row %ld, element %ld)\n", what, n, k, i);
    exit(1);
}

static float some_value(long i) {
    switch (i % 37) {
    case 5: return 0.0f;
    case 11: return -0.0f;
    case 17: return INFINITY;
    case 23: return -INFINITY;
    case 29: return NAN;
    }
    const double mant = 1.0 + (double)(rng() >> 11) / 9007199254740992.0;
    const int e = (int)(rng() % 25) - 20;                 // 2^-20 .. 2^4
    return (float)((rng() & 1 ? -1.0 : 1.0) * std::ldexp(mant, e));
}

static bool within_one_ulp(float got, double want) {
    if (std::isnan(want)) return std::isnan(got);
    if (std::isinf(want)) return got == (float)want;
    const float w = (float)want;
    return got == w || got == std::nextafterf(w, INFINITY) || got == std::nextafterf(w, -INFINITY);
}

static void run(long n, int K, long stride) {
    const float sentinel = 77.0f;
    float* p = (float*)malloc(4 * (size_t)n);
    float* w = (float*)malloc(4 * (size_t)K);
    const size_t total = (size_t)(K - 1) * stride + n;
    float* a = (float*)malloc(4 * total);
    static const double decay[4] = {0.0, 0.5, 0.9, 0.99};
    for (int k = 0; k < K; ++k) w[k] = (float)(1.0 - decay[k]);
    for (size_t i = 0; i < total; ++i) a[i] = sentinel;
    for (int k = 0; k < K; ++k) memset(a + k * stride, 0, 4 * (size_t)n);
    std::vector<double> ref((size_t)K * n, 0.0);
    for (int t = 0; t < 5; ++t) {
        for (long i = 0; i < n; ++i) p[i] = some_value(i + 7 * t);
        if (linr_params_average_host(p, n, w, K, stride, a) != 0) fail("refused", n, K, t);
        for (int k = 0; k < K; ++k)
            for (long i = 0; i < n; ++i) {
                const float before = (float)ref[(size_t)k * n + i];
                const double d = (double)(float)((double)p[i] - (double)before);          // the difference is one fp32 rounding
                const double want = std::fma((double)w[k], d, (double)before);
                const float got = a[k * stride + i];
                if (!within_one_ulp(got, want)) fail("value", n, k, i);
                // w = 1 on a zero average is a copy (of -0: +0); later updates round p - avg first, so they are copies only to rounding
                if (k == 0 && t == 0 && !std::isnan(p[i]) && !(got == p[i])) fail("w = 1 does not copy into a zero average", n, k, i);
                ref[(size_t)k * n + i] = std::isnan(got) ? (double)NAN : (double)got;     // chained from the twin's own value
                ++checked;
            }
        for (int k = 0; k + 1 < K; ++k)
            for (long i = n; i < stride; ++i)
                if (a[k * stride + i] != sentinel) fail("padding written", n, k, i);
    }
    free(p); free(w); free(a);
}

static void refusals() {
    float p[8] = {1, 2, 3, 4, 5, 6, 7, 8}, a[16], w[2] = {0.5f, 1.0f};
    for (float& x : a) x = 77.0f;
    float a0[16];
    memcpy(a0, a, sizeof(a));
    const float w_zero[2] = {0.0f, 0.5f}, w_big[2] = {0.5f, 1.5f}, w_nan[2] = {NAN, 0.5f}, w_neg[2] = {-0.5f, 0.5f};
    struct { const float* p; long n; const float* w; int K; long stride; float* a; } bad[] = {
        {p, -1, w, 2, 8, a}, {p, 8, w, 0, 8, a}, {p, 8, w, 5, 8, a}, {p, 8, nullptr, 2, 8, a}, {p, 8, w_zero, 2, 8, a}, {p, 8, w_big, 2, 8, a},
        {p, 8, w_nan, 2, 8, a}, {p, 8, w_neg, 2, 8, a}, {p, 8, w, 2, 4, a}, {p, 7, w, 2, 7, a}, {p, 6, w, 2, 6, a}, {nullptr, 8, w, 2, 8, a},
        {p, 8, w, 2, 8, nullptr}};
    long id = 0;
    for (const auto& b : bad) {
        if (linr_params_average_host(b.p, b.n, b.w, b.K, b.stride, b.a) != LINR_EINVAL) fail("a bad argument was accepted", id, 0, 0);
        if (memcmp(a, a0, sizeof(a)) != 0) fail("a refused call wrote", id, 0, 0);
        ++id;
    }
    if (linr_params_average_host(nullptr, 0, w, 2, 0, nullptr) != 0) fail("n == 0 is a no-op", 0, 0, 0);
    if (linr_params_average_host(p, 0, w, 2, 8, a) != 0 || memcmp(a, a0, sizeof(a)) != 0) fail("n == 0 wrote", 0, 0, 0);
}

int main() {
    const long sizes[] = {1, 3, 4, 5, 1023, 1024, 1025, 54712};
    for (long n : sizes)
        for (int K : {1, 4})
            for (long pad : {0L, 8L}) run(n, K, ((n + 3) & ~3L) + pad);
    refusals();
    printf("%ld elements, all as expected\n", checked);
    return 0;
}
