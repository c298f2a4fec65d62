// The range coder on the device: linr_ac_encode_binary_codes for many streams at once, a wave per stream.  A stream is serial by its
// format, the streams of a group of frames (8 stages x scales x frames) are independent and outnumber the SIMDs of the device, so a
// group is coded in about the time of its longest stream and only stream bytes and lengths cross to the host.  The coder itself is
// csrc/rc_body.h, the same text that linr_ac_encode_binary_codes runs on the CPU; this file adds where a wave takes its symbols from
// and where its finished words go.
#include "common.h"
#include "rc_body.h"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <vector>

namespace {

// Symbols of a wave: per chunk of 64, lane l holds c1[base + l] (one coalesced 128-byte load) and the chunk's two symbol words
// are loaded uniformly.  chunk(base) makes the chunk loaded one call earlier current and issues the loads of the one behind it,
// so they are under way while the current chunk is walked.  The walk reads symbol i's code value with a readlane: i, and with it
// everything the coder computes from it, is uniform.
struct RcWaveSrc {
    const uint16_t* c; const uint32_t* w; int64_t n; int lane;
    uint32_t cur = 0, nxt = 0;             // per lane
    uint64_t bits = 0, nbits = 0;          // uniform
    __device__ inline void load(int64_t base) {
        nxt = 0; nbits = 0;
        if (base < n) {
            if (base + lane < n) nxt = c[base + lane];
            const int64_t i = base >> 5;
            nbits = w[i];
            if (base + 32 < n) nbits |= (uint64_t)w[i + 1] << 32;
        }
    }
    __device__ inline void chunk(int64_t base) {
        cur = nxt; bits = nbits;
        load(base + RC_CHUNK);
    }
    __device__ inline uint32_t c1(int i) const { return (uint32_t)__builtin_amdgcn_readlane((int)cur, i); }
    __device__ inline uint32_t mask(int i) const { return 0u - (uint32_t)((bits >> i) & 1u); }
};

// Finished words of a wave: lane j holds word j of the current 64-word block, a full block leaves as one coalesced
// 256-byte store, the last one lane-masked with its 1..3 odd bytes from lane 0.  pos, k and over are uniform.  Nothing is stored
// at or behind out + cap: a block that would cross it raises `over` instead (the stream needs more than its cap then, whatever follows).
struct RcWaveOut {
    uint8_t* out; int64_t cap; int lane;
    uint32_t stage = 0;                    // per lane
    int k = 0; int64_t pos = 0; bool over = false;
    __device__ inline bool full() const { return over; }
    __device__ inline void word(uint32_t v) {
        stage = lane == k ? v : stage;          // (this compiler has no writelane builtin; a compare and a select per finished word)
        if (++k == RC_STAGE_WORDS) {
            if (!over && pos + 4 * RC_STAGE_WORDS <= cap) reinterpret_cast<uint32_t*>(out + pos)[lane] = stage; else over = true;
            pos += 4 * RC_STAGE_WORDS;
            k = 0;
        }
    }
    __device__ inline void tail(uint32_t v, int nbytes) {
        if (over || pos + 4 * k + nbytes > cap) { over = true; return; }
        if (lane < k) reinterpret_cast<uint32_t*>(out + pos)[lane] = stage;
        if (lane < nbytes) out[pos + 4 * k + lane] = (uint8_t)(v >> (8 * lane));
    }
};

// One wave per stream, block = one wave, blockIdx.x = stream.  No LDS, no atomics; len[stream] has one writer.
__global__ __launch_bounds__(LINR_WAVE) void rc_encode_k(const uint16_t* __restrict__ c1, const uint32_t* __restrict__ sym,
                                                         const linr_rc_stream* __restrict__ tab, uint8_t* __restrict__ out,
                                                         int64_t* __restrict__ len) {
    const linr_rc_stream d = tab[blockIdx.x];
    const int lane = threadIdx.x;
    RcWaveSrc src{c1 + d.c1_off, sym + d.sym_off, d.n, lane};
    RcWaveOut o{out + d.out_off, d.cap, lane};
    src.load(0);
    // vmcnt(0) here, once: the first chunk has arrived before the loop, so inside it the compiler needs no wait between issuing the
    // next chunk's load and walking the current one (without this it placed a vmcnt(0) there, for the first pass's sake)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    const int64_t bytes = rc_encode(src, d.n, o);
    if (lane == 0) len[blockIdx.x] = o.over ? (int64_t)LINR_ENOSPC : bytes;
}

// The table reaches the device as kernel arguments, RC_TAB_BATCH descriptors per launch: the runtime copies them when the launch is
// queued, so the caller's array is free when the entry returns, and nothing waits for the stream (a copy from pageable memory may).
#define RC_TAB_BATCH 96                     // 96 x 40 bytes = 3840 of the 4096 bytes of kernel arguments
struct RcTabBatch { linr_rc_stream d[RC_TAB_BATCH]; };
__global__ __launch_bounds__(LINR_BLOCK) void rc_table_k(RcTabBatch b, int32_t count, linr_rc_stream* __restrict__ tab) {
    const int t = blockIdx.x * LINR_BLOCK + threadIdx.x;          // one 8-byte field each
    if (t < count * 5) reinterpret_cast<int64_t*>(tab)[t] = reinterpret_cast<const int64_t*>(b.d)[t];
}

// the scan's input: a stream without space counts as empty; one more element so that the scan's last output is the total
__global__ void rc_count_k(const int64_t* __restrict__ len, int32_t n_streams, int64_t* __restrict__ cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n_streams) cnt[i] = (i < n_streams && len[i] > 0) ? len[i] : 0;
}

// One block per stream: its len bytes to payload + offsets[stream].  offsets[i] + len <= sum of the caps <= payload_bytes.
__global__ __launch_bounds__(LINR_BLOCK) void rc_pack_k(const uint8_t* __restrict__ out, const linr_rc_stream* __restrict__ tab,
                                                        const int64_t* __restrict__ len, const int64_t* __restrict__ offsets,
                                                        uint8_t* __restrict__ payload) {
    const int64_t m = len[blockIdx.x];
    const uint8_t* src = out + tab[blockIdx.x].out_off;
    uint8_t* dst = payload + offsets[blockIdx.x];
    for (int64_t b = threadIdx.x; b < m; b += LINR_BLOCK) dst[b] = src[b];
}

struct RcWs { size_t tab, cnt, cub, cub_bytes, total; };

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

RcWs rc_ws(int32_t n_streams) {
    RcWs w;
    w.cub_bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, w.cub_bytes, (const int64_t*)nullptr, (int64_t*)nullptr, n_streams + 1);
    w.tab = 0;
    w.cnt = up256(sizeof(linr_rc_stream) * (size_t)n_streams);
    w.cub = w.cnt + up256(sizeof(int64_t) * ((size_t)n_streams + 1));
    w.total = w.cub + up256(w.cub_bytes);
    return w;
}

// What both entries ask of the host's table: every stream's descriptor within its bounds and its region inside out_dev, and no two
// regions overlapping.
int rc_check_streams(const linr_rc_stream* streams_host, int32_t n_streams, int64_t out_bytes) {
    std::vector<std::pair<int64_t, int64_t>> regions;
    regions.reserve((size_t)n_streams);
    for (int32_t i = 0; i < n_streams; ++i) {
        const linr_rc_stream& d = streams_host[i];
        if (d.n < 0 || d.cap < 0 || d.c1_off < 0 || d.sym_off < 0 || d.out_off < 0 || !linr_rows_fit32(d.n)) return LINR_EINVAL;
        if ((d.out_off & 3) || d.out_off > out_bytes || d.cap > out_bytes - d.out_off) return LINR_EINVAL;
        if (d.cap > 0) regions.emplace_back(d.out_off, d.out_off + d.cap);
    }
    std::sort(regions.begin(), regions.end());
    for (size_t i = 1; i < regions.size(); ++i)
        if (regions[i].first < regions[i - 1].second) return LINR_EINVAL;
    return 0;
}

// the host's table to `tab` on the device (rc_table_k)
int rc_upload_table(const linr_rc_stream* streams_host, int32_t n_streams, linr_rc_stream* tab, hipStream_t s) {
    for (int32_t i = 0; i < n_streams; i += RC_TAB_BATCH) {
        RcTabBatch b;
        const int32_t m = std::min<int32_t>(RC_TAB_BATCH, n_streams - i);
        std::copy(streams_host + i, streams_host + i + m, b.d);
        std::fill(b.d + m, b.d + RC_TAB_BATCH, linr_rc_stream{0, 0, 0, 0, 0});
        rc_table_k<<<dim3(linr_grid(5 * RC_TAB_BATCH, LINR_BLOCK)), dim3(LINR_BLOCK), 0, s>>>(b, m, tab + i);
        const int rc = linr_launch_rc();
        if (rc) return rc;
    }
    return 0;
}

}  // namespace

extern "C" size_t linr_rc_encode_ws_bytes(int32_t n_streams, int64_t total_cap) {
    if (n_streams < 0 || total_cap < 0) return 0;
    return rc_ws(n_streams).total;
}

extern "C" int linr_rc_encode_codes(const uint16_t* c1_dev, const uint32_t* sym_dev, const linr_rc_stream* streams_host, int32_t n_streams,
                                    uint8_t* out_dev, int64_t out_bytes, int64_t* len_dev, uint8_t* payload_dev, int64_t payload_bytes,
                                    int64_t* offsets_dev, void* ws, size_t ws_bytes, void* stream) {
    if (n_streams < 0 || out_bytes < 0 || payload_bytes < 0) return LINR_EINVAL;
    if (n_streams == 0) return 0;
    if (!c1_dev || !sym_dev || !streams_host || !out_dev || !len_dev || !payload_dev || !offsets_dev || !ws) return LINR_EINVAL;
    int rc = rc_check_streams(streams_host, n_streams, out_bytes);
    if (rc) return rc;
    int64_t total_cap = 0;
    for (int32_t i = 0; i < n_streams; ++i) {
        total_cap += streams_host[i].cap;
        if (total_cap > payload_bytes) return LINR_EINVAL;
    }
    const RcWs w = rc_ws(n_streams);
    if (ws_bytes < w.total) return LINR_EINVAL;
    if (((uintptr_t)out_dev & 7) || ((uintptr_t)ws & 7)) return LINR_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    linr_rc_stream* tab = (linr_rc_stream*)(base + w.tab);
    int64_t* cnt = (int64_t*)(base + w.cnt);
    if ((rc = rc_upload_table(streams_host, n_streams, tab, s))) return rc;
    rc_encode_k<<<dim3((unsigned)n_streams), dim3(LINR_WAVE), 0, s>>>(c1_dev, sym_dev, tab, out_dev, len_dev);
    if ((rc = linr_launch_rc())) return rc;
    rc_count_k<<<dim3(linr_grid((int64_t)n_streams + 1, LINR_BLOCK)), dim3(LINR_BLOCK), 0, s>>>(len_dev, n_streams, cnt);
    if ((rc = linr_launch_rc())) return rc;
    size_t cb = w.cub_bytes;
    if ((rc = linr_hip_rc(hipcub::DeviceScan::ExclusiveSum(base + w.cub, cb, cnt, offsets_dev, n_streams + 1, s)))) return rc;
    rc_pack_k<<<dim3((unsigned)n_streams), dim3(LINR_BLOCK), 0, s>>>(out_dev, tab, len_dev, offsets_dev, payload_dev);
    return linr_launch_rc();
}

// ---- chunked streams: a wave per chunk ---------------------------------------------------------------------------------------------
// With chunk_symbols = S a stream of n > S symbols is k = ceil(n / S) independent chunks, so a group's few thousand waves are about
// equally long.  The host's table stays per stream; the chunks' descriptors are derived here from it and from first[], the host's
// prefix sum of the k_i: chunk c of stream i (first[i] <= c < first[i + 1], j = c - first[i]) reads its symbols from j S on and owns
// the 2 n_c + 64 bytes at j (2 S + 64) of the stream's region, which the host has checked to hold all of them.  rc_encode_k codes them
// as it codes streams.  The final bytes of a stream - the LEB128 lengths of its chunks 0 .. k - 2, then the chunks; the lone chunk when
// k == 1 - are placed by two scans: one over the chunks (bytes, header bytes, chunks without space) and one over the streams.
namespace {

#define RC_FIRST_BATCH 960                  // 960 x 4 bytes = 3840 of the 4096 bytes of kernel arguments
struct RcFirstBatch { int32_t v[RC_FIRST_BATCH]; };
__global__ __launch_bounds__(LINR_BLOCK) void rc_first_k(RcFirstBatch b, int32_t count, int32_t* __restrict__ first) {
    const int t = blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (t < count) first[t] = b.v[t];
}

// what a chunk adds to its stream: its bytes, the bytes of its length in the header, 1 if it did not fit
struct alignas(16) RcSum { int64_t bytes; int32_t head; int32_t bad; };
struct RcSumOp {
    __host__ __device__ __forceinline__ RcSum operator()(const RcSum& a, const RcSum& b) const {
        return RcSum{a.bytes + b.bytes, a.head + b.head, a.bad + b.bad};
    }
};

__device__ inline int rc_leb_bytes(int64_t v) { return v < (1 << 7) ? 1 : v < (1 << 14) ? 2 : v < (1 << 21) ? 3 : v < (1 << 28) ? 4 : 5; }

// thread = chunk: the stream it belongs to (a search in first[]) and its descriptor
__global__ __launch_bounds__(LINR_BLOCK) void rc_chunk_table_k(const linr_rc_stream* __restrict__ tab, const int32_t* __restrict__ first,
                                                               int32_t n_streams, int32_t n_chunks, int64_t S,
                                                               linr_rc_stream* __restrict__ ctab, int32_t* __restrict__ owner) {
    const int c = blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (c >= n_chunks) return;
    int lo = 0, hi = n_streams - 1;                                   // the last stream i with first[i] <= c (every stream has a chunk)
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (first[mid] <= c) lo = mid; else hi = mid - 1; }
    const linr_rc_stream d = tab[lo];
    const int64_t j = c - first[lo];
    linr_rc_stream o;
    if (first[lo + 1] - first[lo] == 1) {
        o = d;                                                        // the stream itself, with its own cap
    } else {
        o.n = d.n - j * S < S ? d.n - j * S : S;
        o.c1_off = d.c1_off + j * S;
        o.sym_off = d.sym_off + j * (S >> 5);
        o.out_off = d.out_off + j * (2 * S + 64);
        o.cap = 2 * o.n + 64;
    }
    ctab[c] = o;
    owner[c] = lo;
}

// the first scan's input; one more element so that its last output is the total
__global__ __launch_bounds__(LINR_BLOCK) void rc_chunk_sum_k(const int64_t* __restrict__ clen, const int32_t* __restrict__ owner,
                                                             const int32_t* __restrict__ first, int32_t n_chunks, RcSum* __restrict__ val) {
    const int c = blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (c > n_chunks) return;
    RcSum v{0, 0, 0};
    if (c < n_chunks) {
        const int64_t m = clen[c];
        if (m < 0) v.bad = 1;
        else {
            v.head = c + 1 < first[owner[c] + 1] ? rc_leb_bytes(m) : 0;          // the last chunk's length is not written
            v.bytes = m + v.head;
        }
    }
    val[c] = v;
}

// thread = stream: its length (LINR_ENOSPC when one of its chunks did not fit) and the second scan's input, as rc_count_k
__global__ __launch_bounds__(LINR_BLOCK) void rc_stream_len_k(const RcSum* __restrict__ pre, const int32_t* __restrict__ first,
                                                              int32_t n_streams, int64_t* __restrict__ len, int64_t* __restrict__ cnt) {
    const int i = blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (i > n_streams) return;
    int64_t m = 0;
    if (i < n_streams) {
        const RcSum a = pre[first[i]], b = pre[first[i + 1]];
        m = b.bad - a.bad ? (int64_t)LINR_ENOSPC : b.bytes - a.bytes;
        len[i] = m;
    }
    cnt[i] = m > 0 ? m : 0;
}

// One block per chunk: its bytes behind the stream's header and the chunks in front of it, its length into the header.
// offsets[i] + (bytes of stream i) <= sum of the caps + 5 (n_chunks - n_streams) <= payload_bytes.
__global__ __launch_bounds__(LINR_BLOCK) void rc_pack_chunks_k(const uint8_t* __restrict__ out, const linr_rc_stream* __restrict__ ctab,
                                                               const int64_t* __restrict__ clen, const int32_t* __restrict__ owner,
                                                               const int32_t* __restrict__ first, const RcSum* __restrict__ pre,
                                                               const int64_t* __restrict__ len, const int64_t* __restrict__ offsets,
                                                               uint8_t* __restrict__ payload) {
    const int c = blockIdx.x, i = owner[c];
    if (len[i] < 0) return;
    const RcSum a = pre[first[i]], me = pre[c], z = pre[first[i + 1]];
    const int64_t m = clen[c];
    const int64_t head_all = z.head - a.head, head_before = me.head - a.head;
    uint8_t* base = payload + offsets[i];
    uint8_t* dst = base + head_all + (me.bytes - a.bytes) - head_before;
    const uint8_t* src = out + ctab[c].out_off;
    for (int64_t b = threadIdx.x; b < m; b += LINR_BLOCK) dst[b] = src[b];
    if (threadIdx.x == 0 && c + 1 < first[i + 1]) {
        uint8_t* h = base + head_before;
        uint64_t v = (uint64_t)m;
        while (v >= 0x80u) { *h++ = (uint8_t)(v | 0x80u); v >>= 7; }
        *h = (uint8_t)v;
    }
}

struct RcChunkWs { size_t tab, first, ctab, owner, clen, val, pre, cnt, cub, cub_bytes, total; };

RcChunkWs rc_chunk_ws(int32_t n_streams, int64_t n_chunks) {
    RcChunkWs w;
    size_t a = 0, b = 0;
    (void)hipcub::DeviceScan::ExclusiveScan(nullptr, a, (const RcSum*)nullptr, (RcSum*)nullptr, RcSumOp(), RcSum{0, 0, 0}, (int)(n_chunks + 1));
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const int64_t*)nullptr, (int64_t*)nullptr, n_streams + 1);
    w.cub_bytes = a > b ? a : b;
    size_t cur = 0;
    auto take = [&](size_t bytes) { size_t o = cur; cur += up256(bytes); return o; };
    w.tab = take(sizeof(linr_rc_stream) * (size_t)n_streams);
    w.first = take(4 * ((size_t)n_streams + 1));
    w.ctab = take(sizeof(linr_rc_stream) * (size_t)n_chunks);
    w.owner = take(4 * (size_t)n_chunks);
    w.clen = take(8 * (size_t)n_chunks);
    w.val = take(sizeof(RcSum) * ((size_t)n_chunks + 1));
    w.pre = take(sizeof(RcSum) * ((size_t)n_chunks + 1));
    w.cnt = take(8 * ((size_t)n_streams + 1));
    w.cub = take(w.cub_bytes);
    w.total = cur;
    return w;
}

}  // namespace

extern "C" size_t linr_rc_encode_chunked_ws_bytes(int32_t n_streams, int64_t n_chunks) {
    if (n_streams < 0 || n_chunks < n_streams || n_chunks >= INT32_MAX) return 0;
    return rc_chunk_ws(n_streams, n_chunks).total;
}

extern "C" int linr_rc_encode_codes_chunked(const uint16_t* c1_dev, const uint32_t* sym_dev, const linr_rc_stream* streams_host,
                                            int32_t n_streams, int64_t chunk_symbols, uint8_t* out_dev, int64_t out_bytes, int64_t* len_dev,
                                            uint8_t* payload_dev, int64_t payload_bytes, int64_t* offsets_dev, void* ws, size_t ws_bytes,
                                            void* stream) {
    if (chunk_symbols == 0)
        return linr_rc_encode_codes(c1_dev, sym_dev, streams_host, n_streams, out_dev, out_bytes, len_dev, payload_dev, payload_bytes,
                                    offsets_dev, ws, ws_bytes, stream);
    if (n_streams < 0 || out_bytes < 0 || payload_bytes < 0 || linr_stream_chunk_count(0, chunk_symbols) < 0) return LINR_EINVAL;
    if (n_streams == 0) return 0;
    if (!c1_dev || !sym_dev || !streams_host || !out_dev || !len_dev || !payload_dev || !offsets_dev || !ws) return LINR_EINVAL;
    const int64_t S = chunk_symbols;
    int rc = rc_check_streams(streams_host, n_streams, out_bytes);
    if (rc) return rc;
    int64_t total_cap = 0, n_chunks = 0;
    std::vector<int32_t> first((size_t)n_streams + 1);
    for (int32_t i = 0; i < n_streams; ++i) {
        const linr_rc_stream& d = streams_host[i];
        const int64_t k = linr_stream_chunk_count(d.n, S);
        if (k > 1 && d.cap < 2 * d.n + 64 * k) return LINR_EINVAL;          // the chunks' regions, 2 n_c + 64 each, lie inside the stream's
        first[(size_t)i] = (int32_t)n_chunks;
        n_chunks += k;
        total_cap += d.cap + 5 * (k - 1);                                    // the final bytes: at most the regions and a full header
        if (total_cap > payload_bytes || n_chunks >= INT32_MAX) return LINR_EINVAL;
    }
    first[(size_t)n_streams] = (int32_t)n_chunks;
    const RcChunkWs w = rc_chunk_ws(n_streams, n_chunks);
    if (ws_bytes < w.total) return LINR_EINVAL;
    if (((uintptr_t)out_dev & 7) || ((uintptr_t)ws & 15)) return LINR_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    linr_rc_stream* tab = (linr_rc_stream*)(base + w.tab);
    linr_rc_stream* ctab = (linr_rc_stream*)(base + w.ctab);
    int32_t* first_d = (int32_t*)(base + w.first);
    int32_t* owner = (int32_t*)(base + w.owner);
    int64_t* clen = (int64_t*)(base + w.clen);
    int64_t* cnt = (int64_t*)(base + w.cnt);
    RcSum* val = (RcSum*)(base + w.val);
    RcSum* pre = (RcSum*)(base + w.pre);
    if ((rc = rc_upload_table(streams_host, n_streams, tab, s))) return rc;
    for (int32_t i = 0; i <= n_streams; i += RC_FIRST_BATCH) {
        RcFirstBatch b;
        const int32_t m = std::min<int32_t>(RC_FIRST_BATCH, n_streams + 1 - i);
        std::copy(first.begin() + i, first.begin() + i + m, b.v);
        std::fill(b.v + m, b.v + RC_FIRST_BATCH, 0);
        rc_first_k<<<dim3(linr_grid(RC_FIRST_BATCH, LINR_BLOCK)), dim3(LINR_BLOCK), 0, s>>>(b, m, first_d + i);
        if ((rc = linr_launch_rc())) return rc;
    }
    const dim3 per_chunk(linr_grid(n_chunks + 1, LINR_BLOCK)), per_stream(linr_grid((int64_t)n_streams + 1, LINR_BLOCK));
    rc_chunk_table_k<<<per_chunk, dim3(LINR_BLOCK), 0, s>>>(tab, first_d, n_streams, (int32_t)n_chunks, S, ctab, owner);
    if ((rc = linr_launch_rc())) return rc;
    rc_encode_k<<<dim3((unsigned)n_chunks), dim3(LINR_WAVE), 0, s>>>(c1_dev, sym_dev, ctab, out_dev, clen);
    if ((rc = linr_launch_rc())) return rc;
    rc_chunk_sum_k<<<per_chunk, dim3(LINR_BLOCK), 0, s>>>(clen, owner, first_d, (int32_t)n_chunks, val);
    if ((rc = linr_launch_rc())) return rc;
    size_t cb = w.cub_bytes;
    if ((rc = linr_hip_rc(hipcub::DeviceScan::ExclusiveScan(base + w.cub, cb, val, pre, RcSumOp(), RcSum{0, 0, 0}, (int)(n_chunks + 1), s)))) return rc;
    rc_stream_len_k<<<per_stream, dim3(LINR_BLOCK), 0, s>>>(pre, first_d, n_streams, len_dev, cnt);
    if ((rc = linr_launch_rc())) return rc;
    cb = w.cub_bytes;
    if ((rc = linr_hip_rc(hipcub::DeviceScan::ExclusiveSum(base + w.cub, cb, cnt, offsets_dev, n_streams + 1, s)))) return rc;
    rc_pack_chunks_k<<<dim3((unsigned)n_chunks), dim3(LINR_BLOCK), 0, s>>>(out_dev, ctab, clen, owner, first_d, pre, len_dev, offsets_dev, payload_dev);
    return linr_launch_rc();
}
