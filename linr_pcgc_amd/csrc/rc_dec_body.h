// The binary range decoder's body, once, for the device (csrc/ac_device_dec.hip: rc_decode_k, a wave per stream or chunk) and for its
// host twin (csrc/ac.cpp: linr_ac_decode_binary_twin; tools/rc_decode_emul.cpp): everything that decides a decoded symbol.  The
// counterpart of csrc/rc_body.h; decode_binary_body of csrc/ac.cpp shares no text with it and is its reference.  The whole state is a
// handful of integers that a wave keeps uniform:
//   symbol            t = (span * c1) >> 16;  s = (value - low >= t);  symbol 1: low += t;  symbol 0: high = low + t - 1   (branch-free)
//   renormalisation   all leading bits on which low and high agree at once (clz), then all straddle steps that follow each other
//                     (low 01.., high 10..) at once; j of them leave value = (value << j | bits) - 2^31 mod 2^32.  None after the
//                     last symbol of a stream, as torchac takes none.
//   bit window        64 bits, MSB-aligned, topped up 32 bits at a time from In
// It is parameterised on three things:
//   Src   chunk(base) makes symbols [base, base + 64) current; c1(i) is the code value of symbol base + i
//   In    word() is the next 32 bits of the entry, big-endian; every byte at or behind the entry's end reads as zero, so the decoder
//         is defined on any byte string.  RcWinIn below is the one In: it walks aligned 64-word windows of a byte buffer in which the
//         entry starts at ANY byte; what it is parameterised on (Fetch) only says where a window's words are kept.
//   Out   chunk(base, m, bits) takes the m <= 64 decoded symbols of a chunk, symbol base + i in bit i
// Every loop states its bound: the symbol loops count to n, the renormalisation loop has a cap that it never reaches (a pass takes
// at least one bit and leaves an interval that needs no second one, except when low == high).
#pragma once
#include <stdint.h>
#include "rc_body.h"             // RC_HD, RC_CHUNK, RC_RENORM_CAP, rc_bswap

#define RC_WIN_WORDS 64          // aligned words of a window: one per lane, 256 bytes

struct RcDecState {
    uint32_t low, high, value;
    uint64_t win;                // the next nwin bits of the entry at the top, zeros below them
    int32_t nwin;
};

template <class In>
RC_HD void rc_dec_fill(RcDecState& s, In& in) {                    // afterwards nwin >= 32
    if (s.nwin < 32) {
        s.win |= (uint64_t)in.word() << (32 - s.nwin);
        s.nwin += 32;
    }
}

RC_HD uint32_t rc_dec_take(RcDecState& s, int n) {                 // n in 0..32, n <= nwin
    const uint32_t v = n ? (uint32_t)(s.win >> (64 - n)) : 0u;
    s.win <<= n;
    s.nwin -= n;
    return v;
}

template <class In>
RC_HD void rc_dec_init(RcDecState& s, In& in) {
    s.low = 0; s.high = 0xFFFFFFFFu; s.win = 0; s.nwin = 0;
    rc_dec_fill(s, in);
    s.value = rc_dec_take(s, 32);
}

// the symbol that `value` holds under code value c1, and the split point t that rc_dec_next needs
RC_HD uint32_t rc_dec_bit(const RcDecState& s, uint32_t c1, uint32_t& t) {
    const uint64_t span = (uint64_t)s.high - (uint64_t)s.low + 1;
    t = (uint32_t)((span * c1) >> 16);
    return s.value - s.low >= t ? 1u : 0u;
}

// the interval of the decoded symbol, renormalised
template <class In>
RC_HD void rc_dec_next(RcDecState& s, In& in, uint32_t t, uint32_t bit) {
    const uint32_t one = 0u - bit, lt = s.low + t;
    uint32_t high = (s.high & one) | ((lt - 1u) & ~one);
    uint32_t low = (lt & one) | (s.low & ~one);
    uint32_t value = s.value;
    for (int pass = 0; pass < RC_RENORM_CAP; ++pass) {
        const uint32_t diff = low ^ high;
        if (diff >= 0x80000000u && !((low & ~high) & 0x40000000u)) break;          // top bits differ, no straddle: nothing to shift
        const int k = __builtin_clz(diff | 1u);                     // agreeing leading bits: 0 when the top bits differ, 31 when low == high
        rc_dec_fill(s, in);
        low <<= k;
        high = (high << k) | ((1u << k) - 1u);
        value = (value << k) | rc_dec_take(s, k);
        // one straddle step per leading position below the top with low 1 and high 0 (none: j = 0, which sets the top bits apart)
        const int j = __builtin_clz(~((low & ~high) << 1));         // 0..31; bit 0 of the argument is set
        rc_dec_fill(s, in);
        low = (low << j) & 0x7FFFFFFFu;
        high = (high << j) | 0x80000000u | ((1u << j) - 1u);
        value = ((value << j) | rc_dec_take(s, j)) ^ (j ? 0x80000000u : 0u);
    }
    s.low = low; s.high = high; s.value = value;
}

template <class Src, class In, class Out>
RC_HD void rc_decode(Src& src, int64_t n, In& in, Out& out) {
    RcDecState s;
    rc_dec_init(s, in);
    for (int64_t base = 0; base < n; base += RC_CHUNK) {
        const int m = (int)(n - base < RC_CHUNK ? n - base : RC_CHUNK);
        src.chunk(base);
        uint64_t bits = 0;
        for (int i = 0; i < m; ++i) {
            uint32_t t;
            const uint32_t b = rc_dec_bit(s, src.c1(i), t);
            bits |= (uint64_t)b << i;
            if (base + i + 1 < n) rc_dec_next(s, in, t, b);         // no renormalisation after the last symbol
        }
        out.chunk(base, m, bits);
    }
}

// ---- the In: aligned windows of a byte buffer -------------------------------------------------------------------------------------
// The entry is the bytes [in_off, in_off + in_len) of a buffer of little-endian 32-bit words; in_off has no alignment.  Aligned word q
// of the buffer is taken from a window of RC_WIN_WORDS words that starts at a multiple of RC_WIN_WORDS; the window behind the current
// one is asked for (load) before the current one is walked.  Big-endian word j of the entry is the funnel shift of aligned words
// (in_off >> 2) + j and + j + 1, byte-swapped; the bytes of an aligned word at or behind the entry's end are masked to zero (they
// belong to the next entry, or to nobody), those in front of in_off leave through the shift.
//   Fetch   load(w, end) asks for words [w, w + RC_WIN_WORDS), word q only when 4 q < end (others read as 0: no address at or behind
//           `end` rounded up to 4 is formed); advance() makes the window asked for current; get(k) is its word k
template <class Fetch>
struct RcWinIn {
    Fetch f;
    int64_t end = 0, w0 = 0;          // the entry's end (byte offset), the current window's first word
    int k = 0, sh = 0;                // next word of the window; 8 (in_off & 3)
    uint32_t carry = 0;               // aligned word (in_off >> 2) + j, masked, for the entry's word j
    RC_HD explicit RcWinIn(Fetch fetch) : f(fetch) {}
    RC_HD void open(int64_t in_off, int64_t in_len) {
        const int64_t aw = in_off >> 2;
        end = in_off + in_len;
        sh = 8 * (int)(in_off & 3);
        w0 = aw & ~(int64_t)(RC_WIN_WORDS - 1);
        k = (int)(aw - w0);
        f.load(w0, end);
        f.advance();
        f.load(w0 + RC_WIN_WORDS, end);
        carry = aligned();
    }
    RC_HD uint32_t aligned() {
        if (k == RC_WIN_WORDS) {
            f.advance();
            w0 += RC_WIN_WORDS;
            k = 0;
            f.load(w0 + RC_WIN_WORDS, end);
        }
        const int64_t rem = end - 4 * (w0 + k);                     // bytes of this word that belong to the entry, when below 4
        uint32_t v = f.get(k);
        ++k;
        if (rem < 4) v = rem <= 0 ? 0u : v & ((1u << (8 * (int)rem)) - 1u);
        return v;
    }
    RC_HD uint32_t word() {
        const uint32_t hi = aligned();
        const uint32_t le = (uint32_t)((((uint64_t)hi << 32) | carry) >> sh);
        carry = hi;
        return rc_bswap(le);
    }
};

// ---- the host's Fetch and Out (csrc/ac.cpp) ---------------------------------------------------------------------------------------
// Windows in two 64-word arrays, as in the lanes' registers on the device.  The buffer is the entry's own bytes and nothing more, so a
// word's bytes are copied only as far as they exist (the kernel, whose buffer is padded to whole words, loads the word).
struct RcHostFetch {
    const uint8_t* bytes;
    uint32_t cur[RC_WIN_WORDS], nxt[RC_WIN_WORDS];
    explicit RcHostFetch(const uint8_t* b) : bytes(b) {}
    inline void load(int64_t w, int64_t end) {
        for (int l = 0; l < RC_WIN_WORDS; ++l) {
            const int64_t at = 4 * (w + l), have = end - at;
            nxt[l] = 0;
            if (have > 0) memcpy(&nxt[l], bytes + at, (size_t)(have < 4 ? have : 4));          // little-endian host
        }
    }
    inline void advance() { memcpy(cur, nxt, sizeof(cur)); }
    inline uint32_t get(int k) const { return cur[k]; }
};

// one byte per symbol, like linr_ac_decode_binary
struct RcDecHostOut {
    uint8_t* sym;
    inline void chunk(int64_t base, int m, uint64_t bits) {
        for (int l = 0; l < m; ++l) sym[base + l] = (uint8_t)((bits >> l) & 1u);
    }
};
