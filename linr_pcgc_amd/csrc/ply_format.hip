// Frame output formatted on the device: int32 xyz[n][3] -> the body of an ASCII PLY, one line "%d %d %d\n" per vertex, the bytes
// np.savetxt(fmt='%d') writes for int32 (datautils/custom_dataset.py:37-58).  The decoded coordinates already live on the device and
// their text is about as large as they are, so the formatter costs the bus nothing; it runs while the host threads decode ranges.
//   length  a row's byte count: three digit counts, a '-' per negative value, two blanks and the newline (6 .. 36)
//   scan    one exclusive scan (hipcub) over n + 1 lengths - computed from xyz as the scan reads them, item n is 0 - gives every
//           row's byte offset and, as item n, the length of the text
//   emit    lane = vertex: the lane writes its line at its offset, digit by digit.  The 64 lines of a wave are one contiguous span
//           of the text, so the byte stores of a wave merge in L2 (profiles/ply_format.txt: the emit against the copy it feeds).
// Offsets are int32: n <= LINR_PLY_FORMAT_MAX_ROWS keeps 36 n below 2^31.  No LDS; the kernels belong to no linr_prof_* /
// linr_debug_poison class (all 24 are taken, as for csrc/ac_codes.hip).
#include "common.h"
#include <hipcub/hipcub.hpp>

namespace {

// |v| as uint32: 0 - (uint32)v is 2^31 for INT_MIN, no special case
__host__ __device__ __forceinline__ uint32_t ply_mag(int32_t v) { return v < 0 ? 0u - (uint32_t)v : (uint32_t)v; }

__host__ __device__ __forceinline__ int ply_digits(uint32_t m) {
    return 1 + (m >= 10u) + (m >= 100u) + (m >= 1000u) + (m >= 10000u) + (m >= 100000u) + (m >= 1000000u) + (m >= 10000000u) +
           (m >= 100000000u) + (m >= 1000000000u);
}

// the scan's input: item i < n is the length of line i, item n is 0 (rows at and past n are never read)
struct PlyRowLen {
    const int32_t* xyz;
    int32_t n;
    __host__ __device__ __forceinline__ int32_t operator()(int32_t i) const {
        if (i >= n) return 0;
        int32_t len = 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int32_t v = xyz[(int64_t)i * 3 + c];
            len += ply_digits(ply_mag(v)) + (v < 0);
        }
        return len;
    }
};

using PlyLenIter = hipcub::TransformInputIterator<int32_t, PlyRowLen, hipcub::CountingInputIterator<int32_t>>;

hipError_t ply_scan(void* temp, size_t& temp_bytes, const int32_t* xyz, int32_t n, int32_t* off, hipStream_t s) {
    PlyLenIter in(hipcub::CountingInputIterator<int32_t>(0), PlyRowLen{xyz, n});
    return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, in, off, n + 1, s);
}

// off [n + 1] from the scan: off[i] = first byte of line i, off[n] = the length of the text
__global__ __launch_bounds__(LINR_BLOCK) void ply_emit_k(const int32_t* __restrict__ xyz, int32_t n, const int32_t* __restrict__ off,
                                                         char* __restrict__ text, int64_t* __restrict__ text_len) {
    const int32_t i = (int32_t)(blockIdx.x * LINR_BLOCK + threadIdx.x);
    if (i == 0) *text_len = off[n];
    if (i >= n) return;
    char* p = text + off[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int32_t v = xyz[(int64_t)i * 3 + c];
        uint32_t m = ply_mag(v);
        const int d = ply_digits(m);
        if (v < 0) *p++ = '-';
        for (int k = d - 1; k >= 0; --k) {          // least significant digit last
            p[k] = (char)('0' + m % 10u);
            m /= 10u;
        }
        p += d;
        *p++ = c < 2 ? ' ' : '\n';
    }
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

struct PlyPlan { size_t off_bytes, cub_bytes, total; };

bool ply_plan(int64_t n, PlyPlan& p) {
    if (n <= 0 || n > LINR_PLY_FORMAT_MAX_ROWS) return false;
    size_t cb = 0;
    (void)ply_scan(nullptr, cb, nullptr, (int32_t)n, nullptr, nullptr);
    p.off_bytes = up256((size_t)(n + 1) * 4);
    p.cub_bytes = up256(cb);
    p.total = p.off_bytes + p.cub_bytes;
    return true;
}

}  // namespace

extern "C" size_t linr_ply_format_text_bytes(int64_t n) {
    return n > 0 && n <= LINR_PLY_FORMAT_MAX_ROWS ? (size_t)n * LINR_PLY_FORMAT_MAX_LINE : 0;
}

extern "C" size_t linr_ply_format_ws_bytes(int64_t n) {
    PlyPlan p;
    return ply_plan(n, p) ? p.total : 0;
}

extern "C" int linr_ply_format_ascii(const int32_t* xyz, int64_t n, char* text, size_t text_cap, void* ws, size_t ws_bytes,
                                     int64_t* text_len, void* stream) {
    if (n < 0 || n > LINR_PLY_FORMAT_MAX_ROWS) return LINR_EINVAL;
    if (n == 0) return 0;
    if (!xyz || !text || !ws || !text_len) return LINR_EINVAL;
    PlyPlan p;
    if (!ply_plan(n, p)) return LINR_EINVAL;
    if (text_cap < linr_ply_format_text_bytes(n) || ws_bytes < p.total) return LINR_ENOSPC;
    if ((((uintptr_t)xyz) & 3u) || (((uintptr_t)ws) & 255u) || (((uintptr_t)text_len) & 7u)) return LINR_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    int32_t* off = (int32_t*)ws;
    size_t cb = p.cub_bytes;
    const int rc = linr_hip_rc(ply_scan((char*)ws + p.off_bytes, cb, xyz, (int32_t)n, off, s));
    if (rc) return rc;
    ply_emit_k<<<linr_grid(n, LINR_BLOCK), LINR_BLOCK, 0, s>>>(xyz, (int32_t)n, off, text, text_len);
    return linr_launch_rc();
}
