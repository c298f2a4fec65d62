// The range decoder on the device: linr_ac_decode_binary for many entries at once, a wave per entry.  Within a decode stage every
// probability is known before the first symbol is decoded, the decoder is defined on any byte string (zeros past the end) and the
// streams of a group's frames - or the chunks of a stream - are independent: so a wave decodes an entry from the probabilities where
// the forward left them and writes the occupancy column itself, and nothing crosses to the host.  The decoder itself is
// csrc/rc_dec_body.h, the same text that linr_ac_decode_binary_twin runs on the CPU; this file adds where a wave takes its code
// values and stream words from and where its symbols go.
#include "common.h"
#include "rc_c1.h"
#include "rc_dec_body.h"
#include "ac_device_dec.h"
#include <algorithm>
#include <vector>

namespace {

// Code values of a wave: per chunk of 64, lane l loads p[base + l] (one coalesced 256-byte load, only when base + l < n) and computes
// its c1.  chunk(base) makes the chunk loaded one call earlier current and issues the loads of the one behind it, so they are under
// way while the current chunk is walked.  The walk reads symbol i's code value with a readlane: i, and with it the whole coder state,
// is uniform.
struct RcDecWaveSrc {
    const float* p; int64_t n; int lane;
    uint32_t cur = 0;                      // per lane: c1 of the current chunk
    float nxt = 1.0f;                      // per lane: the probability loaded for the next one
    __device__ inline void load(int64_t base) {
        nxt = 1.0f;
        if (base + lane < n) nxt = p[base + lane];
    }
    __device__ inline void chunk(int64_t base) {
        cur = linr_c1_from_p(nxt);
        load(base + RC_CHUNK);
    }
    __device__ inline uint32_t c1(int i) const { return (uint32_t)__builtin_amdgcn_readlane((int)cur, i); }
};

// Stream words of a wave: lane l holds aligned word w + l of the current 64-word window and of the one behind it (one 256-byte load
// each, a word only when it starts in front of the entry's end); the walk takes word k with a readlane.
struct RcWaveFetch {
    const uint32_t* words; int lane;
    uint32_t cur = 0, nxt = 0;             // per lane
    __device__ inline void load(int64_t w, int64_t end) {
        nxt = 0;
        if (4 * (w + lane) < end) nxt = words[w + lane];
    }
    __device__ inline void advance() { cur = nxt; }
    __device__ inline uint32_t get(int k) const { return (uint32_t)__builtin_amdgcn_readlane((int)cur, k); }
};

// Decoded symbols of a wave: the 64 bits of a chunk are one uniform mask, lane l stores bit l to its row of the occupancy column as
// 0.0f / 1.0f (what occ_col_from_u8_k of csrc/decode.hip writes) and, when there is one, to the byte plane.  Per-lane vector stores
// under the lane mask; rows [row0, row0 + n) only.
struct RcDecWaveOut {
    float* occ_col; int64_t ld; uint8_t* sym; int64_t row0; int lane;
    __device__ inline void chunk(int64_t base, int m, uint64_t bits) {
        if (lane < m) {
            const uint32_t b = (uint32_t)(bits >> lane) & 1u;
            const int64_t r = row0 + base + lane;
            occ_col[r * ld] = b ? 1.0f : 0.0f;
            if (sym) sym[r] = (uint8_t)b;
        }
    }
};

// One wave per entry, block = one wave, blockIdx.x = entry.  No LDS, no atomics; every output element has one writer (the entries'
// row ranges do not overlap).
__global__ __launch_bounds__(LINR_WAVE) void rc_decode_k(const float* __restrict__ probs, const uint32_t* __restrict__ words,
                                                         const linr_rc_dec_entry* __restrict__ tab, float* __restrict__ occ_col,
                                                         int64_t occ_ld, uint8_t* __restrict__ sym) {
    const linr_rc_dec_entry d = tab[blockIdx.x];
    if (d.n <= 0) return;
    const int lane = threadIdx.x;
    RcDecWaveSrc src{probs + d.p_off, d.n, lane};
    RcWinIn<RcWaveFetch> in{RcWaveFetch{words, lane}};
    RcDecWaveOut out{occ_col, occ_ld, sym, d.out_row, lane};
    src.load(0);
    in.open(d.in_off, d.in_len);
    rc_decode(src, d.n, in, out);
}

// The table reaches the device as kernel arguments, RC_DEC_TAB_BATCH entries per launch: the runtime copies them when the launch is
// queued, so the caller's array is free when the entry returns, and nothing waits for the stream (rc_table_k's scheme, csrc/ac_device.hip).
#define RC_DEC_TAB_BATCH 96                 // 96 x 40 bytes = 3840 of the 4096 bytes of kernel arguments
struct RcDecTabBatch { linr_rc_dec_entry d[RC_DEC_TAB_BATCH]; };
__global__ __launch_bounds__(LINR_BLOCK) void rc_dec_table_k(RcDecTabBatch b, int32_t count, linr_rc_dec_entry* __restrict__ tab) {
    const int t = blockIdx.x * LINR_BLOCK + threadIdx.x;          // one 8-byte field each
    if (t < count * 5) reinterpret_cast<int64_t*>(tab)[t] = reinterpret_cast<const int64_t*>(b.d)[t];
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

int linr_rc_dec_check(const linr_rc_dec_entry* e, int32_t n_entries, int64_t n_probs, int64_t bytes_len, int64_t n_rows) {
    if (n_entries < 0 || n_probs < 0 || bytes_len < 0 || n_rows < 0) return LINR_EINVAL;
    if (n_entries > 0 && !e) return LINR_EINVAL;
    std::vector<std::pair<int64_t, int64_t>> rows;
    rows.reserve((size_t)n_entries);
    for (int32_t i = 0; i < n_entries; ++i) {
        const linr_rc_dec_entry& d = e[i];
        if (d.p_off < 0 || d.n < 0 || d.in_off < 0 || d.in_len < 0 || d.out_row < 0) return LINR_EINVAL;
        if (d.p_off > n_probs || d.n > n_probs - d.p_off) return LINR_EINVAL;
        if (d.in_off > bytes_len || d.in_len > bytes_len - d.in_off) return LINR_EINVAL;
        if (d.out_row > n_rows || d.n > n_rows - d.out_row) return LINR_EINVAL;
        if (d.n > 0) rows.emplace_back(d.out_row, d.out_row + d.n);
    }
    std::sort(rows.begin(), rows.end());
    for (size_t i = 1; i < rows.size(); ++i)
        if (rows[i].first < rows[i - 1].second) return LINR_EINVAL;
    return 0;
}

int linr_rc_dec_upload(const linr_rc_dec_entry* e, int32_t n_entries, linr_rc_dec_entry* tab_dev, hipStream_t s) {
    for (int32_t i = 0; i < n_entries; i += RC_DEC_TAB_BATCH) {
        RcDecTabBatch b;
        const int32_t m = std::min<int32_t>(RC_DEC_TAB_BATCH, n_entries - i);
        std::copy(e + i, e + i + m, b.d);
        std::fill(b.d + m, b.d + RC_DEC_TAB_BATCH, linr_rc_dec_entry{0, 0, 0, 0, 0});
        rc_dec_table_k<<<dim3(linr_grid(5 * RC_DEC_TAB_BATCH, LINR_BLOCK)), dim3(LINR_BLOCK), 0, s>>>(b, m, tab_dev + i);
        const int rc = linr_launch_rc();
        if (rc) return rc;
    }
    return 0;
}

int linr_rc_dec_launch(const float* probs, const uint8_t* bytes_dev, const linr_rc_dec_entry* tab_dev, int32_t n_entries, float* occ_col,
                       int64_t occ_ld, uint8_t* sym_dev, hipStream_t s) {
    if (n_entries <= 0) return 0;
    rc_decode_k<<<dim3((unsigned)n_entries), dim3(LINR_WAVE), 0, s>>>(probs, reinterpret_cast<const uint32_t*>(bytes_dev), tab_dev, occ_col,
                                                                      occ_ld, sym_dev);
    return linr_launch_rc();
}

extern "C" size_t linr_rc_decode_ws_bytes(int32_t n_entries) {
    if (n_entries < 0) return 0;
    return up256(sizeof(linr_rc_dec_entry) * (size_t)n_entries);
}

extern "C" int linr_rc_decode_probs(const float* probs_dev, int64_t n_probs, const uint8_t* bytes_dev, int64_t bytes_len,
                                    const linr_rc_dec_entry* entries_host, int32_t n_entries, float* occ_col_dev, int64_t occ_ld,
                                    int64_t n_rows, uint8_t* sym_dev, void* ws, size_t ws_bytes, void* stream) {
    if (n_entries < 0 || occ_ld < 1) return LINR_EINVAL;
    if (n_entries == 0) return 0;
    int rc = linr_rc_dec_check(entries_host, n_entries, n_probs, bytes_len, n_rows);
    if (rc) return rc;
    if (!probs_dev || !occ_col_dev || !ws || (bytes_len > 0 && !bytes_dev)) return LINR_EINVAL;
    if (ws_bytes < linr_rc_decode_ws_bytes(n_entries)) return LINR_EINVAL;
    if (((uintptr_t)bytes_dev & 3) || ((uintptr_t)ws & 7) || ((uintptr_t)probs_dev & 3) || ((uintptr_t)occ_col_dev & 3)) return LINR_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    linr_rc_dec_entry* tab = (linr_rc_dec_entry*)ws;
    if ((rc = linr_rc_dec_upload(entries_host, n_entries, tab, s))) return rc;
    return linr_rc_dec_launch(probs_dev, bytes_dev, tab, n_entries, occ_col_dev, occ_ld, sym_dev, s);
}
