// The binary range encoder's body, once, for the host (csrc/ac.cpp: linr_ac_encode_binary, linr_ac_encode_binary_codes) and for the
// device (csrc/ac_device.hip: rc_encode_k): everything that decides a byte of a stream.  It compiles for both sides and holds its
// whole state in a handful of integers that a wave can keep uniform:
//   interval update   t = (span * c1) >> 16;  symbol 1: low += t;  symbol 0: high = low + t - 1      (branch-free select)
//   renormalisation   all leading bits on which low and high agree at once (clz), the first of them followed by the pending
//                     complements; the straddle case low >= 0x40000000 && high < 0xC0000000 adds one pending bit per step, and
//                     the steps that follow each other are taken together (as decode_binary_body of csrc/ac.cpp takes them)
//   bit accumulator   fills 32-bit words MSB first; a finished word is handed on byte-swapped, i.e. as the little-endian load of
//                     its four stream bytes
//   finish            ++pending, the last bit, its run, zero padding to a byte
// It is parameterised on two things only:
//   Src   chunk(base) makes symbols [base, base + 64) current; c1(i) / mask(i) are the code value and the symbol (0 or ~0) of
//         symbol base + i
//   Out   word(w) takes a finished word; tail(w, nbytes) the last, partial one (its first nbytes bytes belong to the stream);
//         full() says that the stream no longer fits its buffer, which ends the walk early
// Every loop states its bound: the renormalisation loop repeats only while low == high and has a cap that a correct coder never
// reaches (a pass shifts at least one bit out of 32), the run loop counts down `pending`.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RC_HD __host__ __device__ inline
#else
#define RC_HD inline
#endif

#define RC_CHUNK 64              // symbols per chunk: one wave's load of code values, two symbol words
#define RC_STAGE_WORDS 64        // finished words staged before they leave: one per lane, 256 bytes
#define RC_RENORM_CAP 34
// Host only: a symbol that shifts nothing leaves rc_symbol after one test (most symbols of a trained model), and one that takes no
// straddle step skips that step's arithmetic: predicted branches keep both off the chain low, high -> next symbol
// (profiles/host_coder_one_body.txt).  On the device the early exit was measured and was not faster (profiles/device_coder_ab.txt),
// so the kernel's code stays as it is.
#if defined(__HIP_DEVICE_COMPILE__)
#define RC_QUIET_EXIT 0
#else
#define RC_QUIET_EXIT 1
#endif

struct RcState {
    uint32_t low, high;
    uint64_t pending;            // straddle bits owed; any length
    uint64_t acc;                // the low nacc bits are the bits not yet handed on (what lies above them is stale)
    int32_t nacc;                // 0..31 between calls
    int64_t nwords;              // words handed on
};

RC_HD void rc_init(RcState& s) {
    s.low = 0; s.high = 0xFFFFFFFFu; s.pending = 0; s.acc = 0; s.nacc = 0; s.nwords = 0;
}

RC_HD uint32_t rc_bswap(uint32_t v) { return __builtin_bswap32(v); }

template <class Out>
RC_HD void rc_put_bits(RcState& s, Out& out, uint32_t v, int n) {          // n in 0..32, v < 2^n
    s.acc = (s.acc << n) | v;
    s.nacc += n;
    if (s.nacc >= 32) {
        s.nacc -= 32;
        out.word(rc_bswap((uint32_t)(s.acc >> s.nacc)));
        ++s.nwords;
    }
}

template <class Out>
RC_HD void rc_put_run(RcState& s, Out& out, uint32_t bit, uint64_t count) {
    const uint32_t word = 0u - bit;
    for (; count >= 32; count -= 32) rc_put_bits(s, out, word, 32);
    if (count) rc_put_bits(s, out, word >> (32 - (int)count), (int)count);
}

template <class Out>
RC_HD void rc_symbol(RcState& s, Out& out, uint32_t c1, uint32_t one) {          // one: 0 for symbol 0, ~0 for symbol 1
    const uint64_t span = (uint64_t)s.high - (uint64_t)s.low + 1;
    const uint32_t t = (uint32_t)((span * c1) >> 16);
    const uint32_t lt = s.low + t;
    uint32_t high = (s.high & one) | ((lt - 1u) & ~one);
    uint32_t low = (lt & one) | (s.low & ~one);
    // the top bits differ and the interval does not straddle the middle as 01.. / 10..: nothing to shift (the test of
    // decode_binary_body in csrc/ac.cpp; as two branches it measured faster here than as that one)
    if (RC_QUIET_EXIT && (int32_t)(low ^ high) < 0 && !((low & ~high) & 0x40000000u)) {
        s.low = low; s.high = high;
        return;
    }
    for (int pass = 0; pass < RC_RENORM_CAP; ++pass) {
        const uint32_t diff = low ^ high;
        if (diff < 0x80000000u) {
            int k = diff ? __builtin_clz(diff) : 31;          // leading bits shared by low and high (>= 1)
            if (k > 31) k = 31;
            const uint32_t first = low >> 31;
            if (s.pending) {
                rc_put_bits(s, out, first, 1);
                rc_put_run(s, out, first ^ 1u, s.pending);
                s.pending = 0;
                if (k > 1) rc_put_bits(s, out, (low << 1) >> (33 - k), k - 1);
            } else {
                rc_put_bits(s, out, low >> (32 - k), k);
            }
            low <<= k;
            high = (high << k) | ((1u << k) - 1u);
            if (diff == 0) continue;                          // low == high: the new top bits may agree again
        }
        if (RC_QUIET_EXIT && !((low & ~high) & 0x40000000u)) break;          // host: no straddle step to take
        // The top bits differ now (low 0.., high 1..) and do so after every straddle step, so no bit can be shared again and
        // the steps can be taken at once: one per leading position below the top with low 1 and high 0 (none: j = 0).
        const int j = __builtin_clz(~((low & ~high) << 1));          // 0..31; bit 0 of the argument is set
        s.pending += (uint32_t)j;
        low = (low << j) & 0x7FFFFFFFu;
        high = (high << j) | 0x80000000u | ((1u << j) - 1u);
        break;
    }
    s.low = low;
    s.high = high;
}

// The end of a stream.  Returns its length in bytes, whether it fitted or not.
template <class Out>
RC_HD int64_t rc_finish(RcState& s, Out& out) {
    ++s.pending;
    const uint32_t last = s.low < 0x40000000u ? 0u : 1u;
    rc_put_bits(s, out, last, 1);
    rc_put_run(s, out, last ^ 1u, s.pending);
    s.pending = 0;
    const int nbytes = (s.nacc + 7) >> 3;                  // zero padding to a byte; 0..4
    const uint32_t w = s.nacc ? (uint32_t)(s.acc << (32 - s.nacc)) : 0u;
    out.tail(rc_bswap(w), nbytes);
    return 4 * s.nwords + nbytes;
}

template <class Src, class Out>
RC_HD int64_t rc_encode(Src& src, int64_t n, Out& out) {
    RcState s;
    rc_init(s);
    for (int64_t base = 0; base < n && !out.full(); base += RC_CHUNK) {
        const int m = (int)(n - base < RC_CHUNK ? n - base : RC_CHUNK);
        src.chunk(base);
        for (int i = 0; i < m; ++i) rc_symbol(s, out, src.c1(i), src.mask(i));
    }
    return rc_finish(s, out);
}

// ---- the host's Src and Out (csrc/ac.cpp) ------------------------------------------------------------------------------------
#include <string.h>

// Code values and symbol bit planes, read in place.  (The source of linr_ac_encode_binary, probabilities and symbol bytes, stands
// in csrc/ac.cpp beside c1_block, which it shares with the decoder.)
struct RcHostSrc {
    const uint16_t* c; const uint32_t* w; int64_t n;
    uint64_t bits = 0; int64_t base = 0;
    inline void chunk(int64_t b) {
        base = b;
        const int64_t i = b >> 5;
        bits = w[i];
        if (b + 32 < n) bits |= (uint64_t)w[i + 1] << 32;
    }
    inline uint32_t c1(int i) const { return c[base + i]; }
    inline uint32_t mask(int i) const { return 0u - (uint32_t)((bits >> i) & 1u); }
};

// Finished words are staged in a 64-word array, as in the lanes' registers on the device; a block leaves whole, the last one cut
// to the stream's length.  Nothing is stored at or behind out + cap: a block that would cross it raises `over` instead.
struct RcHostOut {
    uint8_t* out; int64_t cap;
    uint32_t stage[RC_STAGE_WORDS]; int k = 0; int64_t pos = 0; bool over = false;
    RcHostOut(uint8_t* o, int64_t c) : out(o), cap(c) {}
    inline bool full() const { return over; }
    inline void word(uint32_t v) {
        stage[k++] = v;
        if (k == RC_STAGE_WORDS) {
            if (!over && pos + 4 * RC_STAGE_WORDS <= cap) memcpy(out + pos, stage, 4 * RC_STAGE_WORDS); else over = true;
            pos += 4 * RC_STAGE_WORDS;
            k = 0;
        }
    }
    inline void tail(uint32_t v, int nbytes) {
        if (over || pos + 4 * k + nbytes > cap) { over = true; return; }
        if (k) memcpy(out + pos, stage, 4 * (size_t)k);
        if (nbytes) memcpy(out + pos + 4 * k, &v, (size_t)nbytes);          // little-endian host: the first nbytes stream bytes
    }
};
