// Range-coder feed computed on the device: what the host coder needs of a probability is its 16-bit code value
//   c1 = (rint((1 - p) * 65534) + 1) & 0xFFFF                     (binary_c1 of csrc/ac.cpp; torchac's cdf row [0, c1, 2^16])
// and of the occupancy one bit.  One launch turns the [8][rows] probabilities of a forward and the [rows][8] occupancy into
// [8][rows] uint16 code values and 8 bit planes: 17 bits per symbol cross to the host instead of 40, and the coder threads
// read c1 instead of computing it (linr_ac_encode_binary_codes).
#include "common.h"
#include "rc_c1.h"

namespace {

// A block is 8 waves over the same 64 rows, wave k = stage k: the probability loads and the 2-byte stores of a wave are
// contiguous along the row index, the 8 waves read the same 64 occupancy rows (2 KB, each 32-byte sector fetched once and hit in
// the L1 by the other seven), and the ballot of a wave is the two symbol words of its 64 rows, stored by lanes 0 and 32.  No LDS,
// no atomics: every output element has exactly one writer.
__global__ __launch_bounds__(512) void ac_codes_k(const float* __restrict__ probs, int64_t probs_ld, const float* __restrict__ occ,
                                                  int occ_ld, int64_t n, uint16_t* __restrict__ c1, int64_t c1_ld,
                                                  uint32_t* __restrict__ sym, int64_t sym_ld) {
    const int lane = threadIdx.x, k = threadIdx.y;
    const int64_t i = (int64_t)blockIdx.x * LINR_WAVE + lane;
    bool bit = false;
    if (i < n) {
        const float p = probs[k * probs_ld + i];
        c1[k * c1_ld + i] = (uint16_t)linr_c1_from_p(p);          // (csrc/rc_c1.h: the range decoder's kernel computes the same)
        bit = occ[i * occ_ld + k] != 0.0f;
    }
    const unsigned long long b = __ballot(bit);          // lanes past n vote 0: the pad bits of the last word
    if ((lane & 31) == 0) {
        const int64_t w = (int64_t)blockIdx.x * 2 + (lane >> 5);
        if (w * 32 < n) sym[k * sym_ld + w] = (uint32_t)(b >> lane);
    }
}

}  // namespace

extern "C" size_t linr_ac_codes_sym_words(int64_t n) { return n > 0 ? (size_t)((n + 31) / 32) : 0; }

extern "C" int linr_ac_codes(const float* probs, int64_t probs_ld, const float* occ, int32_t occ_ld, int64_t n, uint16_t* c1,
                             int64_t c1_ld, uint32_t* sym, int64_t sym_ld, void* stream) {
    if (n < 0 || !probs || !occ || !c1 || !sym) return LINR_EINVAL;
    if (probs_ld < n || c1_ld < n || occ_ld < 8 || sym_ld < (int64_t)linr_ac_codes_sym_words(n)) return LINR_EINVAL;
    if (!linr_rows_fit32(n)) return LINR_EINVAL;
    if (n == 0) return 0;
    ac_codes_k<<<dim3(linr_grid(n, LINR_WAVE)), dim3(LINR_WAVE, 8), 0, (hipStream_t)stream>>>(probs, probs_ld, occ, occ_ld, n, c1, c1_ld,
                                                                                                sym, sym_ld);
    return linr_launch_rc();
}
