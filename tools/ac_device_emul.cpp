// The range encoder's one body (csrc/rc_body.h: what the device coder runs a wave per stream) run on the HOST through both of its host
// sources - linr_ac_encode_binary_codes (code values + symbol bit planes) and linr_ac_encode_binary (probabilities + symbol bytes; the
// 64-word staging array of their sink stands in for the lanes) - against the bit-at-a-time coder linr_ac_encode_cdf16 (rows [0, c1, 0],
// lp = 3, unshared), which shares no code with the body, under AddressSanitizer + UBSan; no GPU is involved and nothing is launched.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/ac_device_emul.cpp \
//       linr_pcgc_amd/csrc/ac.cpp -lpthread -o a.out && ./a.out 300000
// Every stream is coded into a heap buffer of exactly cap bytes (a store at or behind out + cap aborts), its code values, symbol
// words, probabilities and symbol bytes sit in buffers of exactly n, ceil(n / 32), n and n elements.  The probability of a symbol is
// 1 - (c1 - 1) / 65534, which the library's rounding takes back to c1.  Inputs: <count> random streams (lengths around the 32-symbol
// word, the 64-symbol chunk and the 64-word staging block; code values uniform, tiny with either symbol dominant, 32768 alternating),
// each also with cap = the stream's length (fits exactly), one byte less and 0 (LINR_ENOSPC); and greedy prefixes that drive `pending`
// past the 32- and 64-bit pieces of the run writer, resolved by bit 0, by bit 1 and by the end of the stream.
#include "../include/linr_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static std::mt19937_64 rng(20240607);
static long checked = 0;

static void fail(const char* what, size_t n, long a, long b) {
    fprintf(stderr, "FAIL %s: n = %zu, body %ld, comparand %ld\n", what, n, a, b);
    exit(1);
}

template <class T>
static T* exact(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }

// the three coders on one stream in exact-size buffers; returns the comparand's length
static int64_t compare(const std::vector<uint16_t>& c1v, const std::vector<uint8_t>& s, int64_t cap) {
    const size_t n = c1v.size(), nw = (n + 31) / 32;
    uint16_t* c1 = exact<uint16_t>(n);
    uint32_t* w = exact<uint32_t>(nw);
    float* p = exact<float>(n);
    uint8_t* sb = exact<uint8_t>(n);
    uint16_t* rows = exact<uint16_t>(3 * n);
    int16_t* sym = exact<int16_t>(n);
    memset(w, 0, nw * 4);
    for (size_t i = 0; i < n; ++i) {
        c1[i] = c1v[i];
        w[i >> 5] |= (uint32_t)(s[i] & 1) << (i & 31);
        p[i] = 1.0f - (float)(c1v[i] - 1) / 65534.0f;
        sb[i] = s[i];
        rows[3 * i] = 0; rows[3 * i + 1] = c1v[i]; rows[3 * i + 2] = 0;
        sym[i] = s[i] & 1;
    }
    uint8_t* out[3];
    for (auto& o : out) { o = exact<uint8_t>((size_t)cap); memset(o, 0xA5, cap ? (size_t)cap : 1); }
    const int64_t want = linr_ac_encode_cdf16(rows, 3, 0, sym, (int64_t)n, out[0], cap);
    const int64_t got[2] = {linr_ac_encode_binary_codes(c1, w, (int64_t)n, out[1], cap),
                            linr_ac_encode_binary(p, sb, (int64_t)n, out[2], cap)};
    for (int k = 0; k < 2; ++k) {
        if (got[k] != want) fail(k ? "length, probabilities" : "length, code values", n, (long)got[k], (long)want);
        if (want > 0 && memcmp(out[k + 1], out[0], (size_t)want)) fail(k ? "bytes, probabilities" : "bytes, code values", n, (long)got[k], (long)want);
    }
    for (auto& o : out) free(o);
    free(c1); free(w); free(p); free(sb); free(rows); free(sym);
    ++checked;
    return want;
}

static void all_caps(const std::vector<uint16_t>& c1, const std::vector<uint8_t>& s) {
    const int64_t len = compare(c1, s, 2 * (int64_t)c1.size() + 64);
    if (len < 1) fail("comparand length", c1.size(), 0, (long)len);
    if (compare(c1, s, len) != len) fail("exact cap", c1.size(), 0, (long)len);
    if (compare(c1, s, len - 1) != LINR_ENOSPC) fail("cap - 1", c1.size(), 0, (long)len);
    if (compare(c1, s, 0) != LINR_ENOSPC) fail("cap 0", c1.size(), 0, (long)len);
}

static void draw(int regime, size_t n, std::vector<uint16_t>& c1, std::vector<uint8_t>& s) {
    c1.resize(n); s.resize(n);
    for (size_t i = 0; i < n; ++i) {
        switch (regime) {
        case 0: c1[i] = (uint16_t)(1 + rng() % 65535); s[i] = rng() & 1; break;
        case 1: c1[i] = (uint16_t)(1 + rng() % 3); s[i] = (rng() % 1000) != 0; break;          // long stretches without output
        case 2: c1[i] = (uint16_t)(1 + rng() % 3); s[i] = (rng() % 1000) == 0; break;          // ~16 bits per symbol
        default: c1[i] = 32768; s[i] = i & 1; break;
        }
    }
}

// a plain model of the interval, one bit at a time: what a step does to (low, high, pending) and whether it emits a bit
struct Model { uint32_t low = 0, high = 0xFFFFFFFFu; uint64_t pending = 0; };
static bool step(Model& m, uint32_t c1, int sym) {
    const uint64_t span = (uint64_t)m.high - m.low + 1;
    const uint32_t t = (uint32_t)((span * c1) >> 16);
    if (sym) m.low += t; else m.high = m.low + t - 1;
    bool emitted = false;
    for (;;) {
        if (m.high < 0x80000000u || m.low >= 0x80000000u) {
            emitted = true; m.pending = 0;
            m.low <<= 1; m.high = (m.high << 1) | 1u;
        } else if (m.low >= 0x40000000u && m.high < 0xC0000000u) {
            ++m.pending;
            m.low = (m.low << 1) & 0x7FFFFFFFu; m.high = (m.high << 1) | 0x80000001u;
        } else break;
    }
    return emitted;
}

static void pending_runs() {
    for (int steps : {8, 16, 24, 40}) {
        Model m;
        std::vector<uint16_t> c1; std::vector<uint8_t> s;
        for (int i = 0; i < steps; ++i) {
            const uint64_t span = (uint64_t)m.high - m.low + 1;
            const int64_t c = (int64_t)((((uint64_t)0x80000000u - m.low) << 16) / span);
            bool have = false; Model best; uint32_t bc = 0; int bs = 0;
            for (int64_t cc = c - 1; cc <= c + 2; ++cc) for (int sym = 0; sym < 2; ++sym) {
                if (cc < 1 || cc > 65535) continue;
                Model t = m;
                if (step(t, (uint32_t)cc, sym)) continue;
                if (!have || t.pending > best.pending) { have = true; best = t; bc = (uint32_t)cc; bs = sym; }
            }
            if (!have) break;
            m = best; c1.push_back((uint16_t)bc); s.push_back((uint8_t)bs);
        }
        printf("pending prefix: %zu symbols, pending %llu\n", c1.size(), (unsigned long long)m.pending);
        if (steps >= 16 && m.pending < 96) fail("generator", c1.size(), (long)m.pending, 96);
        all_caps(c1, s);                                             // the end of the stream flushes the run
        for (int sym = 0; sym < 2; ++sym) {                          // resolved by bit 0 / bit 1: a near-certain symbol at either end
            std::vector<uint16_t> c2 = c1; std::vector<uint8_t> s2 = s;
            c2.push_back(sym ? 65535 : 1); s2.push_back((uint8_t)sym);
            for (int i = 0; i < 70; ++i) { c2.push_back((uint16_t)(1 + rng() % 65535)); s2.push_back(rng() & 1); }
            all_caps(c2, s2);
        }
    }
}

int main(int argc, char** argv) {
    const long count = argc > 1 ? atol(argv[1]) : 300000;
    std::vector<uint16_t> c1; std::vector<uint8_t> s;
    for (size_t n : {0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 70001})
        for (int regime = 0; regime < 4; ++regime) { draw(regime, n, c1, s); all_caps(c1, s); }
    pending_runs();
    for (long i = 0; i < count; ++i) {
        const int regime = (int)(rng() % 4);
        size_t n = rng() % 200;
        if (i % 64 == 0) n = 2000 + rng() % 3000;                    // regime 2 fills the staging block several times
        draw(regime, n, c1, s);
        if (i % 8 == 0) all_caps(c1, s); else compare(c1, s, 2 * (int64_t)n + 64);
    }
    printf("ac_device_emul: %ld comparisons, all equal\n", checked);
    return 0;
}
