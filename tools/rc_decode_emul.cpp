// The device range decoder's body (csrc/rc_dec_body.h: what rc_decode_k of csrc/ac_device_dec.hip runs a wave per entry) on the HOST
// under AddressSanitizer + UBSan, with the kernel's memory access modelled; no GPU is involved and nothing is launched.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/rc_decode_emul.cpp
//     linr_pcgc_amd/csrc/ac.cpp -lpthread -o a.out && ./a.out 40          (one command line)
// The In is the body's own RcWinIn over a Fetch that reads as the wave does: aligned 32-bit words of 64-word windows, lane l's word
// only when it starts in front of the entry's end, the next window asked for before the current one is walked.  The entries of a
// round - streams the host encoder wrote for all kinds of code values, and byte strings that are no streams at all - are packed back
// to back behind a lead of 0..7 non-zero bytes, so that they start at every alignment and every entry's neighbours are non-zero, in
// ONE heap buffer of exactly the size a caller owes the kernel: the total rounded up to 4 bytes (linr_rc_decode_probs' contract), or
// that rounded up to 256 bytes plus one 256-byte window (the decoder scales' workspace), the padding non-zero, too.  A read outside
// it aborts.  Code values and symbols sit in exact-size heap arrays.  Every entry must decode to what linr_ac_decode_binary_codes gives
// for its bytes alone (an exact-size copy): the bytes that follow an entry read as zeros, not as what is there.
#include "../include/linr_hip.h"
#include "../linr_pcgc_amd/csrc/rc_dec_body.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static std::mt19937_64 rng(20241019);
static long checked = 0;

static void fail(const char* what, long a, long b) {
    fprintf(stderr, "FAIL %s: %ld, %ld\n", what, a, b);
    exit(1);
}

// the wave's window loads: whole aligned words, guarded per lane by the entry's end
struct EmulFetch {
    const uint8_t* buf;
    uint32_t cur[RC_WIN_WORDS], nxt[RC_WIN_WORDS];
    explicit EmulFetch(const uint8_t* b) : buf(b) {}
    void load(int64_t w, int64_t end) {
        for (int l = 0; l < RC_WIN_WORDS; ++l) {
            nxt[l] = 0;
            if (4 * (w + l) < end) memcpy(&nxt[l], buf + 4 * (w + l), 4);
        }
    }
    void advance() { memcpy(cur, nxt, sizeof(cur)); }
    uint32_t get(int k) const { return cur[k]; }
};

// the wave's code values: lane l's element only when it exists
struct EmulSrc {
    const uint16_t* c; int64_t n;
    uint32_t cur[RC_CHUNK];
    void chunk(int64_t base) {
        for (int l = 0; l < RC_CHUNK; ++l) cur[l] = base + l < n ? c[base + l] : 0u;
    }
    uint32_t c1(int i) const { return cur[i]; }
};

struct Entry {
    std::vector<uint16_t> c1;
    std::vector<uint8_t> bytes;
};

static Entry coded(int64_t n, int regime) {
    Entry e;
    e.c1.resize((size_t)n);
    std::vector<uint32_t> sym((size_t)((n + 31) / 32) + 1, 0u);
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t r = (uint32_t)(rng() >> 32);
        uint32_t c, s;
        if (regime == 0) { c = 1 + r % 65535; s = (r >> 20) & 1; }
        else if (regime == 1) { c = 1 + r % 3; s = (r >> 8) % 1000 != 0; }          // quiet: long stretches without a shift
        else if (regime == 2) { c = 1 + r % 3; s = (r >> 8) % 1000 == 0; }          // loud: ~16 bits per symbol
        else { c = 32768; s = i & 1; }
        e.c1[(size_t)i] = (uint16_t)c;
        sym[(size_t)(i >> 5)] |= s << (i & 31);
    }
    e.bytes.resize((size_t)(2 * n + 64));
    const int64_t len = linr_ac_encode_binary_codes(e.c1.data(), sym.data(), n, e.bytes.data(), (int64_t)e.bytes.size());
    if (len < 1) fail("encode", (long)len, (long)n);
    e.bytes.resize((size_t)len);
    return e;
}

static Entry garbage(int64_t n, int64_t len) {
    Entry e;
    e.c1.resize((size_t)n);
    for (auto& c : e.c1) c = (uint16_t)(1 + rng() % 65535);
    e.bytes.resize((size_t)len);
    for (auto& b : e.bytes) b = (uint8_t)(rng() | 1);          // never zero
    return e;
}

// the entries back to back behind `lead` bytes, in a buffer padded as `workspace` says; each against the host decoder on its own bytes
static void round_of(const std::vector<Entry>& es, int lead, bool workspace) {
    size_t total = (size_t)lead;
    for (auto& e : es) total += e.bytes.size();
    const size_t size = workspace ? ((total + 255) & ~(size_t)255) + 256 : (total + 3) & ~(size_t)3;
    uint8_t* exact = (uint8_t*)malloc(size ? size : 1);
    memset(exact, 0xEE, size ? size : 1);
    size_t at = (size_t)lead;
    for (int i = 0; i < lead; ++i) exact[i] = 0xFF;
    for (auto& e : es) { if (!e.bytes.empty()) memcpy(exact + at, e.bytes.data(), e.bytes.size()); at += e.bytes.size(); }
    at = (size_t)lead;
    for (size_t i = 0; i < es.size(); ++i) {
        const Entry& e = es[i];
        const int64_t n = (int64_t)e.c1.size();
        uint16_t* c = (uint16_t*)malloc(n ? 2 * (size_t)n : 1);
        if (n) memcpy(c, e.c1.data(), 2 * (size_t)n);
        uint8_t* got = (uint8_t*)malloc(n ? (size_t)n : 1);
        uint8_t* want = (uint8_t*)malloc(n ? (size_t)n : 1);
        uint8_t* alone = (uint8_t*)malloc(e.bytes.size() ? e.bytes.size() : 1);
        if (!e.bytes.empty()) memcpy(alone, e.bytes.data(), e.bytes.size());
        memset(got, 0x77, n ? (size_t)n : 1);
        if (linr_ac_decode_binary_codes(n ? c : nullptr, n, e.bytes.empty() ? nullptr : alone, (int64_t)e.bytes.size(), n ? want : nullptr))
            fail("reference decode", (long)i, (long)n);
        EmulSrc src{c, n, {}};
        RcWinIn<EmulFetch> in{EmulFetch(exact)};
        in.open((int64_t)at, (int64_t)e.bytes.size());
        RcDecHostOut out{got};
        if (n > 0) rc_decode(src, n, in, out);                  // (the kernel leaves an empty entry at once)
        if (n && memcmp(got, want, (size_t)n)) {
            int64_t j = 0;
            while (got[j] == want[j]) ++j;
            fail("an entry decodes differently among neighbours", (long)i, (long)j);
        }
        free(c); free(got); free(want); free(alone);
        at += e.bytes.size();
        ++checked;
    }
    free(exact);
}

int main(int argc, char** argv) {
    const long rounds = argc > 1 ? atol(argv[1]) : 40;
    const int64_t ns[] = {0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 4097, 20000};
    const int64_t glen[] = {0, 1, 3, 4, 5, 255, 256, 257, 1000};
    for (int lead = 0; lead < 8; ++lead) {
        std::vector<Entry> es;
        for (size_t i = 0; i < sizeof(ns) / sizeof(ns[0]); ++i) es.push_back(coded(ns[i], (int)((i + lead) % 4)));
        for (int64_t len : glen) es.push_back(garbage(3000, len));
        {
            Entry cut = coded(300, 0);                            // a stream truncated at every length up to 16 bytes
            for (size_t len = 0; len <= 16 && len <= cut.bytes.size(); ++len) {
                Entry t = cut;
                t.bytes.resize(len);
                es.push_back(t);
            }
        }
        round_of(es, lead, false);
        round_of(es, lead, true);
    }
    for (long r = 0; r < rounds; ++r) {
        std::vector<Entry> es;
        const int count = 1 + (int)(rng() % 12);
        for (int i = 0; i < count; ++i) {
            const int64_t n = (int64_t)(rng() % (rng() % 8 == 0 ? 9000 : 700));
            if (rng() % 4 == 0) es.push_back(garbage(n, (int64_t)(rng() % 600)));
            else es.push_back(coded(n, (int)(rng() % 4)));
        }
        round_of(es, (int)(rng() % 8), r % 2 == 0);
    }
    printf("rc_decode_emul: %ld entries, all as expected\n", checked);
    return 0;
}
