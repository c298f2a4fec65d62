// Frame input parsed on the device: the body of an ASCII PLY -> int32 xyz[n][3] (the contract of linr_ply_parse_ascii, csrc/ply.cpp,
// fast path only), and the records of a binary PLY -> the same.  The text of a loot frame is 17 MB and is wanted on the device anyway.
//   lines   a byte starts vertex r when it is no blank, only blanks lie between it and the previous '\n' (or the start of the text)
//           and it is the r-th such byte.  Blank runs have no bounded length, so this is a two-state scan, no look-back: per 16-byte
//           chunk and per entry state ("a token was already seen on this line" or not) the exit state and the number of line starts
//           (PlySum, 8 bytes; the two counts differ by at most 1).  One exclusive hipcub scan composes the summaries - computed from
//           the text as the scan reads it - with an associative, non-commutative operator; ply_lines_k re-walks every chunk from its
//           known entry state and writes line_off[r] for r < n_rows.  Both read the text as one 16-byte load per lane; the last,
//           partial chunk is read byte by byte and never at or past text + len.
//   parse   lane = vertex: the lane walks its line from line_off[r], every read bounded by len.  [+-] digits [. digits] with at most
//           15 digits is mant / 10^f; rounded to nearest, ties to even, in integers - exactly what the host's double division
//           followed by nearbyint gives.  Anything else raises a flag (integer atomicOr / atomicMin on status, the rare path) and
//           the caller takes that frame to the host parser.  The 64 lines of a wave are one contiguous span of the text.
//   binary  lane = vertex over records of `stride` bytes; the three fields assembled from byte loads (records are unaligned), either
//           byte order, converted exactly to double and rounded with rint.
// Offsets are int32: len <= 2^31 - 1.  No LDS, no float atomics, nothing allocated; the kernels belong to no linr_prof_* /
// linr_debug_poison class (all 24 are taken, as for csrc/ply_format.hip).
#include "common.h"
#include <hipcub/hipcub.hpp>

namespace {

constexpr int PLY_CHUNK = 16;

// blank inside a line: ' ', '\t', '\v', '\f', '\r' ('\n' ends the line)
__host__ __device__ __forceinline__ bool ply_blank(unsigned c) { return c == ' ' || (c >= 9u && c <= 13u && c != '\n'); }

// a chunk's effect on the line state: entered with "no token on this line yet" (0) it leaves in state exit0 after count0 line starts,
// entered with "token seen" (1) in state exit1 after count0 - diff (diff is 0 or 1: only the first line start can depend on the entry)
struct alignas(8) PlySum {
    int32_t count0;
    uint8_t exit0, exit1, diff, pad;
};

struct PlyCompose {          // a, then b
    __host__ __device__ __forceinline__ PlySum operator()(const PlySum& a, const PlySum& b) const {
        const int32_t c0 = a.count0 + b.count0 - (a.exit0 ? b.diff : 0);
        const int32_t c1 = a.count0 - a.diff + b.count0 - (a.exit1 ? b.diff : 0);
        PlySum r;
        r.count0 = c0;
        r.exit0 = a.exit0 ? b.exit1 : b.exit0;
        r.exit1 = a.exit1 ? b.exit1 : b.exit0;
        r.diff = (uint8_t)(c0 - c1);
        r.pad = 0;
        return r;
    }
};

// chunk i of the text: 16 bytes as four words, fewer (nb) in the last chunk, whose bytes are loaded one by one
struct PlyChunk {
    uint32_t w[4];
    int nb;
    __host__ __device__ __forceinline__ unsigned byte(int k) const { return (w[k >> 2] >> (8 * (k & 3))) & 0xffu; }
};

__host__ __device__ __forceinline__ PlyChunk ply_load_chunk(const char* __restrict__ text, int64_t len, int64_t i) {
    PlyChunk c;
    const int64_t base = i * PLY_CHUNK;
    if (base + PLY_CHUNK <= len) {
        const uint4 v = *reinterpret_cast<const uint4*>(text + base);          // text is 16-byte aligned
        c.w[0] = v.x, c.w[1] = v.y, c.w[2] = v.z, c.w[3] = v.w;
        c.nb = PLY_CHUNK;
    } else {
        c.w[0] = c.w[1] = c.w[2] = c.w[3] = 0u;
        c.nb = (int)(len - base);
#pragma unroll
        for (int k = 0; k < PLY_CHUNK; ++k)
            if (k < c.nb) c.w[k >> 2] |= (uint32_t)(unsigned char)text[base + k] << (8 * (k & 3));
    }
    return c;
}

// the scan's input: item i is the summary of chunk i
struct PlyChunkSum {
    const char* text;
    int64_t len;
    __host__ __device__ __forceinline__ PlySum operator()(int32_t i) const {
        const PlyChunk c = ply_load_chunk(text, len, i);
        int s0 = 0, s1 = 1;
        int32_t n0 = 0, n1 = 0;
#pragma unroll
        for (int k = 0; k < PLY_CHUNK; ++k) {
            if (k < c.nb) {
                const unsigned b = c.byte(k);
                if (b == '\n') {
                    s0 = s1 = 0;
                } else if (!ply_blank(b)) {
                    n0 += !s0, n1 += !s1;
                    s0 = s1 = 1;
                }
            }
        }
        PlySum r;
        r.count0 = n0;
        r.exit0 = (uint8_t)s0, r.exit1 = (uint8_t)s1, r.diff = (uint8_t)(n0 - n1), r.pad = 0;
        return r;
    }
};

using PlySumIter = hipcub::TransformInputIterator<PlySum, PlyChunkSum, hipcub::CountingInputIterator<int32_t>>;

hipError_t ply_sum_scan(void* temp, size_t& temp_bytes, const char* text, int64_t len, int32_t nchunks, PlySum* pre, hipStream_t s) {
    PlySumIter in(hipcub::CountingInputIterator<int32_t>(0), PlyChunkSum{text, len});
    const PlySum identity = {0, 0, 1, 0, 0};
    return hipcub::DeviceScan::ExclusiveScan(temp, temp_bytes, in, pre, PlyCompose(), identity, nchunks, s);
}

__host__ __device__ __forceinline__ void ply_raise(int64_t* status, int64_t flag, int64_t row) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicOr(reinterpret_cast<unsigned long long*>(status), (unsigned long long)flag);
    atomicMin(reinterpret_cast<unsigned long long*>(status) + 1, (unsigned long long)row);          // rows are >= 0
#else
    status[0] |= flag;
    status[1] = row < status[1] ? row : status[1];
#endif
}

// chunk i re-walked from its entry state pre[i]: the offsets of the line starts r < n_rows.  The thread of the last chunk knows how
// many non-empty lines the text has: *total = min(that, n_rows), and LINR_PLY_SHORT when there are fewer than n_rows.
__host__ __device__ __forceinline__ void ply_lines_chunk(const char* __restrict__ text, int64_t len, int32_t nchunks, int32_t i,
                                                         const PlySum* __restrict__ pre, int64_t n_rows, int32_t* __restrict__ line_off,
                                                         int32_t* __restrict__ total, int64_t* __restrict__ status) {
    const PlySum p = pre[i];
    int state = p.exit0;
    int64_t r = p.count0;
    const bool last = i == nchunks - 1;
    if (r >= n_rows && !last) return;          // everything behind the n_rows-th line is ignored
    if (r < n_rows) {
        const PlyChunk c = ply_load_chunk(text, len, i);
#pragma unroll
        for (int k = 0; k < PLY_CHUNK; ++k) {
            if (k < c.nb) {
                const unsigned b = c.byte(k);
                if (b == '\n') {
                    state = 0;
                } else if (!ply_blank(b)) {
                    if (!state) {
                        if (r < n_rows) line_off[r] = i * PLY_CHUNK + k;
                        ++r;
                    }
                    state = 1;
                }
            }
        }
    }
    if (last) {
        *total = (int32_t)(r < n_rows ? r : n_rows);
        if (r < n_rows) ply_raise(status, LINR_PLY_SHORT, r);
    }
}

struct PlyCols { int32_t n_cols, c[3]; };

// vertex r: its line from line_off[r]; every read is bounded by len
__host__ __device__ __forceinline__ void ply_parse_row(const char* __restrict__ text, int32_t len, int64_t r, int32_t p, PlyCols cols,
                                                       int32_t* __restrict__ xyz, int64_t* __restrict__ status) {
    int32_t v[3] = {0, 0, 0};
    for (int32_t c = 0; c < cols.n_cols; ++c) {
        while (p < len && ply_blank((unsigned char)text[p])) ++p;
        if (p >= len || text[p] == '\n') return ply_raise(status, LINR_PLY_COLUMNS, r);          // the line (or the text) ended early
        bool neg = false;
        if (text[p] == '-' || text[p] == '+') neg = text[p] == '-', ++p;
        uint64_t mant = 0;
        int digits = 0, frac = 0;
        while (p < len && (unsigned)(text[p] - '0') < 10u && digits < 15) mant = mant * 10 + (unsigned)(text[p] - '0'), ++p, ++digits;
        if (p < len && text[p] == '.' && digits < 15) {
            ++p;
            while (p < len && (unsigned)(text[p] - '0') < 10u && digits < 15)
                mant = mant * 10 + (unsigned)(text[p] - '0'), ++p, ++digits, ++frac;
        }
        if (!(digits > 0 && (p == len || text[p] == '\n' || ply_blank((unsigned char)text[p]))))
            return ply_raise(status, LINR_PLY_TOKEN, r);          // exponent, more digits, inf, nan, a word: the host decides
        if (c == cols.c[0] || c == cols.c[1] || c == cols.c[2]) {
            uint64_t q = mant;
            if (frac) {          // mant / 10^frac to the nearest integer, ties to even
                uint64_t pw = 10;
                for (int k = 1; k < frac; ++k) pw *= 10;
                const uint64_t rem = mant % pw;
                q = mant / pw;
                q += (2 * rem > pw || (2 * rem == pw && (q & 1u))) ? 1u : 0u;
            }
            if (q > (neg ? 2147483648ull : 2147483647ull)) return ply_raise(status, LINR_PLY_RANGE, r);
            const int32_t val = (int32_t)(neg ? 0u - (uint32_t)q : (uint32_t)q);
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (c == cols.c[j]) v[j] = val;
        }
    }
    for (; p < len && text[p] != '\n'; ++p)          // nothing but blanks up to the end of the line
        if (!ply_blank((unsigned char)text[p])) return ply_raise(status, LINR_PLY_COLUMNS, r);
#pragma unroll
    for (int j = 0; j < 3; ++j) xyz[r * 3 + j] = v[j];
}

struct PlyFields { int32_t off[3], type[3]; };

__host__ __device__ __forceinline__ int ply_type_bytes(int32_t t) { return t < 2 ? 1 : t < 4 ? 2 : t < 7 ? 4 : 8; }

#ifdef __HIP_DEVICE_COMPILE__
// type codes of ply._PLY_TYPES: 0 i1, 1 u1, 2 i2, 3 u2, 4 i4, 5 u4, 6 f4, 7 f8
__device__ __forceinline__ void ply_gather_row(const uint8_t* __restrict__ rec, int64_t r, int32_t stride, PlyFields f, bool big,
                                               int32_t* __restrict__ xyz, int64_t* __restrict__ status) {
    int32_t v[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const uint8_t* p = rec + r * stride + f.off[j];
        const int nb = ply_type_bytes(f.type[j]);
        uint64_t u = 0;
        for (int k = 0; k < nb; ++k) u |= (uint64_t)p[k] << (8 * (big ? nb - 1 - k : k));
        double d;
        switch (f.type[j]) {
            case 0: d = (double)(int8_t)u; break;
            case 1: d = (double)(uint8_t)u; break;
            case 2: d = (double)(int16_t)u; break;
            case 3: d = (double)(uint16_t)u; break;
            case 4: d = (double)(int32_t)u; break;
            case 5: d = (double)(uint32_t)u; break;
            case 6: d = (double)__uint_as_float((uint32_t)u); break;
            default: d = __longlong_as_double((long long)u); break;
        }
        d = rint(d);          // ties to even
        if (!(d >= -2147483648.0 && d <= 2147483647.0)) return ply_raise(status, LINR_PLY_RANGE, r);          // NaN fails both
        v[j] = (int32_t)d;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) xyz[r * 3 + j] = v[j];
}
#endif

__global__ void ply_status_init_k(int64_t* __restrict__ status, int64_t flags, int64_t first_row) {
    status[0] = flags;
    status[1] = first_row;
}

__global__ __launch_bounds__(LINR_BLOCK) void ply_lines_k(const char* __restrict__ text, int64_t len, int32_t nchunks,
                                                          const PlySum* __restrict__ pre, int64_t n_rows, int32_t* __restrict__ line_off,
                                                          int32_t* __restrict__ total, int64_t* __restrict__ status) {
    const int32_t i = (int32_t)(blockIdx.x * LINR_BLOCK + threadIdx.x);
    if (i < nchunks) ply_lines_chunk(text, len, nchunks, i, pre, n_rows, line_off, total, status);
}

__global__ __launch_bounds__(LINR_BLOCK) void ply_parse_k(const char* __restrict__ text, int32_t len, const int32_t* __restrict__ line_off,
                                                          const int32_t* __restrict__ total, PlyCols cols, int32_t* __restrict__ xyz,
                                                          int64_t* __restrict__ status) {
    const int64_t r = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (r < *total) ply_parse_row(text, len, r, line_off[r], cols, xyz, status);
}

__global__ __launch_bounds__(LINR_BLOCK) void ply_gather_k(const uint8_t* __restrict__ rec, int64_t n_rows, int32_t stride, PlyFields f,
                                                           int32_t big, int32_t* __restrict__ xyz, int64_t* __restrict__ status) {
#ifdef __HIP_DEVICE_COMPILE__
    const int64_t r = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (r < n_rows) ply_gather_row(rec, r, stride, f, big != 0, xyz, status);
#endif
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace: pre [nchunks] | line_off [rows] | total | the scan's scratch.  A non-empty line is at least 2 bytes with its newline, so
// no text has more than len / 2 + 1 of them, however many are announced.
struct PlyParsePlan { int32_t nchunks; size_t pre_bytes, off_bytes, cub_bytes, total; };

bool ply_parse_plan(size_t len, int64_t n_rows, PlyParsePlan& p) {
    if (len > (size_t)INT32_MAX || n_rows < 0) return false;
    p.nchunks = (int32_t)((len + PLY_CHUNK - 1) / PLY_CHUNK);
    const int64_t most = (int64_t)(len / 2 + 1), rows = n_rows < most ? n_rows : most;
    size_t cb = 0;
    (void)ply_sum_scan(nullptr, cb, nullptr, (int64_t)len, p.nchunks > 0 ? p.nchunks : 1, nullptr, nullptr);
    p.pre_bytes = up256((size_t)p.nchunks * sizeof(PlySum));
    p.off_bytes = up256((size_t)rows * 4);
    p.cub_bytes = up256(cb);
    p.total = p.pre_bytes + p.off_bytes + 256 + p.cub_bytes;
    return true;
}

}  // namespace

extern "C" size_t linr_ply_parse_ws_bytes(size_t len, int64_t n_rows) {
    PlyParsePlan p;
    return ply_parse_plan(len, n_rows, p) ? p.total : 0;
}

extern "C" int linr_ply_parse_ascii_device(const char* text, size_t len, int64_t n_rows, int32_t n_cols, int32_t cx, int32_t cy,
                                           int32_t cz, int32_t* xyz, void* ws, size_t ws_bytes, int64_t* status, void* stream) {
    if (n_rows < 0 || n_cols < 3 || n_cols > 64 || len > (size_t)INT32_MAX) return LINR_EINVAL;
    const PlyCols cols = {n_cols, {cx, cy, cz}};
    for (int j = 0; j < 3; ++j)
        if (cols.c[j] < 0 || cols.c[j] >= n_cols) return LINR_EINVAL;
    if (n_rows == 0) return 0;
    if ((!text && len) || !xyz || !ws || !status) return LINR_EINVAL;
    PlyParsePlan p;
    if (!ply_parse_plan(len, n_rows, p)) return LINR_EINVAL;
    if (ws_bytes < p.total) return LINR_ENOSPC;
    if (!linr_aligned16(text) || (((uintptr_t)ws) & 255u) || (((uintptr_t)status) & 7u)) return LINR_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (len == 0) {          // no line at all
        ply_status_init_k<<<1, 1, 0, s>>>(status, LINR_PLY_SHORT, 0);
        return linr_launch_rc();
    }
    PlySum* pre = (PlySum*)ws;
    int32_t* line_off = (int32_t*)((char*)ws + p.pre_bytes);
    int32_t* total = (int32_t*)((char*)ws + p.pre_bytes + p.off_bytes);
    ply_status_init_k<<<1, 1, 0, s>>>(status, 0, n_rows);
    size_t cb = p.cub_bytes;
    int rc = linr_hip_rc(ply_sum_scan((char*)ws + p.pre_bytes + p.off_bytes + 256, cb, text, (int64_t)len, p.nchunks, pre, s));
    if (rc) return rc;
    ply_lines_k<<<linr_grid(p.nchunks, LINR_BLOCK), LINR_BLOCK, 0, s>>>(text, (int64_t)len, p.nchunks, pre, n_rows, line_off, total, status);
    if ((rc = linr_launch_rc())) return rc;
    const int64_t most = (int64_t)(len / 2 + 1), rows = n_rows < most ? n_rows : most;          // *total <= rows
    ply_parse_k<<<linr_grid(rows, LINR_BLOCK), LINR_BLOCK, 0, s>>>(text, (int32_t)len, line_off, total, cols, xyz, status);
    return linr_launch_rc();
}

extern "C" int linr_ply_gather_binary(const uint8_t* rec, int64_t n_rows, int32_t stride, const int32_t off[3], const int32_t type[3],
                                      int32_t big_endian, int32_t* xyz, int64_t* status, void* stream) {
    if (n_rows < 0 || stride <= 0 || !off || !type) return LINR_EINVAL;
    PlyFields f;
    for (int j = 0; j < 3; ++j) {
        if (type[j] < 0 || type[j] > 7 || off[j] < 0 || (int64_t)off[j] + ply_type_bytes(type[j]) > stride) return LINR_EINVAL;
        f.off[j] = off[j], f.type[j] = type[j];
    }
    if (n_rows == 0) return 0;
    if (!rec || !xyz || !status) return LINR_EINVAL;
    if ((((uintptr_t)xyz) & 3u) || (((uintptr_t)status) & 7u)) return LINR_EALIGN;
    const int64_t blocks = (n_rows + LINR_BLOCK - 1) / LINR_BLOCK;
    if (blocks > INT32_MAX) return LINR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    ply_status_init_k<<<1, 1, 0, s>>>(status, 0, n_rows);
    ply_gather_k<<<(unsigned)blocks, LINR_BLOCK, 0, s>>>(rec, n_rows, stride, f, big_endian, xyz, status);
    return linr_launch_rc();
}
