// The host twin of the geometry digest (linr_coords_digest_host, csrc/digest_host.cpp; body: csrc/digest_body.h - the text the kernels
// of csrc/digest.hip run) on the HOST under AddressSanitizer + UBSan; no GPU is involved and nothing is launched.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/digest_emul.cpp \
//       linr_pcgc_amd/csrc/digest_host.cpp -o a.out && ./a.out 200
// Every coordinate list sits in a heap buffer of exactly 12 n bytes (a read at or behind its end aborts), the origin in one of exactly
// 12.  Checked: the five known answers of include/linr_hip.h's definition; <count> random lists of n rows around the sizes 0, 1, 63,
// 64, 65, 1000 with coordinates over the whole int32 range (INT32_MIN / INT32_MAX rows and origins included: the additions must wrap
// without signed overflow) against this file's own restatement of the definition, their reversal (the digest is one of the set), and
// the refusals (n < 0 and a NULL list are the empty list).
#include "../include/linr_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static std::mt19937_64 rng(20261021);
static long checked = 0;

static void fail(const char* what, long a, unsigned long long want, unsigned long long got) {
    fprintf(stderr, "FAIL %s (%ld): want %016llx, got %016llx\n", what, a, want, got);
    exit(1);
}

// the definition once more, written on its own
static uint64_t m(uint64_t v) {
    v ^= v >> 30; v *= 0xBF58476D1CE4E5B9ull; v ^= v >> 27; v *= 0x94D049BB133111EBull; v ^= v >> 31;
    return v;
}
static uint64_t expect(const std::vector<int32_t>& rows, const int32_t* org) {
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    uint64_t s = 0;
    for (size_t i = 0; i + 2 < rows.size(); i += 3) {
        uint32_t u[3];
        for (int a = 0; a < 3; ++a) u[a] = (uint32_t)((int64_t)rows[i + a] + (org ? (int64_t)org[a] : 0));
        s += m(m((uint64_t)u[0] | ((uint64_t)u[1] << 32)) + u[2] + G);
    }
    return m(s ^ m((uint64_t)(rows.size() / 3) + G));
}

// the twin on exact-size heap copies
static uint64_t twin(const std::vector<int32_t>& rows, const int32_t* org) {
    int32_t* c = rows.empty() ? nullptr : (int32_t*)malloc(rows.size() * sizeof(int32_t));
    if (c) memcpy(c, rows.data(), rows.size() * sizeof(int32_t));
    int32_t* o = org ? (int32_t*)malloc(3 * sizeof(int32_t)) : nullptr;
    if (o) memcpy(o, org, 3 * sizeof(int32_t));
    const uint64_t d = linr_coords_digest_host(c, (int64_t)(rows.size() / 3), o);
    free(c); free(o);
    ++checked;
    return d;
}

static void known(const std::vector<int32_t>& rows, const int32_t* org, uint64_t want, long id) {
    const uint64_t got = twin(rows, org);
    if (got != want) fail("known answer", id, want, got);
    if (expect(rows, org) != want) fail("this file's restatement", id, want, expect(rows, org));
}

int main(int argc, char** argv) {
    const long count = argc > 1 ? atol(argv[1]) : 200;
    const int32_t org[3] = {10, -20, 30};
    known({}, nullptr, 0x48218226ff3cd4bfull, 0);
    known({0, 0, 0}, nullptr, 0x8e58975f6d0dc556ull, 1);
    known({1, 2, 3, -1, INT32_MAX, INT32_MIN}, nullptr, 0x2fb051dd12d1e535ull, 2);
    known({1, 2, 3, 4, 5, 6}, org, 0xf2be1d4320cbd4c0ull, 3);
    known({1, 2, 3, 1, 2, 3}, nullptr, 0x49e80c0367870be3ull, 4);

    const long sizes[] = {0, 1, 63, 64, 65, 1000};
    for (long t = 0; t < count; ++t) {
        const long n = sizes[t % 6] + (t % 7 == 6 ? (long)(rng() % 5) : 0);
        std::vector<int32_t> rows(3 * n);
        for (auto& v : rows) {
            const uint64_t r = rng();
            v = (r & 15) == 0 ? INT32_MIN : (r & 15) == 1 ? INT32_MAX : (int32_t)(uint32_t)(r >> 32);
        }
        int32_t o[3];
        for (int a = 0; a < 3; ++a) o[a] = t % 3 == 0 ? INT32_MAX : t % 3 == 1 ? INT32_MIN : (int32_t)(uint32_t)rng();
        const int32_t* op = t % 4 == 0 ? nullptr : o;
        const uint64_t want = expect(rows, op), got = twin(rows, op);
        if (got != want) fail("random list", t, want, got);
        std::vector<int32_t> rev(rows.size());
        for (long i = 0; i < n; ++i)
            for (int a = 0; a < 3; ++a) rev[3 * i + a] = rows[3 * (n - 1 - i) + a];
        if (twin(rev, op) != want) fail("reversed list", t, want, twin(rev, op));
    }

    const uint64_t none = 0x48218226ff3cd4bfull;
    int32_t one[3] = {1, 2, 3};
    if (linr_coords_digest_host(one, -1, nullptr) != none) fail("n < 0", -1, none, linr_coords_digest_host(one, -1, nullptr));
    if (linr_coords_digest_host(nullptr, 5, nullptr) != none) fail("NULL list", 5, none, linr_coords_digest_host(nullptr, 5, nullptr));
    printf("%ld digests, all as expected\n", checked);
    return 0;
}
