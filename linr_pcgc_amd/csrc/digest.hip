// Geometry digests on the device (linr_coords_digest_segments): the order-independent 64-bit digest of csrc/digest_body.h over
// row segments of a coordinate list - the octree levels of an encoder's frame, the children of a decoder scale - where the
// coordinates already are.  Two launches and no atomics:
//   coords_digest_k         grid (tiles, segments), 256 lanes: a lane strides over its segment's rows (one 12-byte load per row) and
//                           sums their terms; the wave sums by lane exchange, the 4 waves through LDS (written, barrier, read); ONE
//                           partial per workgroup into the workspace, partial[segment][tile] (a workgroup without rows writes 0)
//   coords_digest_finish_k  grid (segments), one wave: sums the segment's partials and applies the finalisation
// The kernel boundary orders the partials, and integer sums that wrap do not depend on the order they are taken in, so every
// grid shape gives the digest of the host loop (linr_coords_digest_host).  The segment table and the origins travel as kernel
// arguments (1,288 bytes): the host arrays are free on return and nothing is uploaded.
#include "common.h"
#include "digest_body.h"
#include "prof.h"

namespace {

constexpr int DG_BLOCK = 256;                       // rows of one workgroup per pass
constexpr int DG_MAX_TILES = 256;                   // workgroups per segment at most: a pass of the grid is 65,536 rows of a segment

struct DgTab {
    int64_t off[LINR_DECODE_MAX_FRAMES + 1];        // segment j = rows [off[j], off[j + 1])
    int32_t org[LINR_DECODE_MAX_FRAMES][3];
};

struct __attribute__((packed, aligned(4))) DgRow { int32_t x, y, z; };

__device__ __forceinline__ uint64_t dg_wave_sum(uint64_t x) {
#pragma unroll
    for (int d = LINR_WAVE / 2; d >= 1; d >>= 1) x += __shfl_xor((unsigned long long)x, d, LINR_WAVE);
    return x;
}

// partial: [gridDim.y][gridDim.x]
__global__ __launch_bounds__(DG_BLOCK) void coords_digest_k(const int32_t* __restrict__ coords, DgTab tab, uint64_t* __restrict__ partial) {
    __shared__ uint64_t s_sum[DG_BLOCK / LINR_WAVE];
    const int tid = threadIdx.x;
    const int seg = blockIdx.y;
    const int64_t hi = tab.off[seg + 1];
    const int32_t ox = tab.org[seg][0], oy = tab.org[seg][1], oz = tab.org[seg][2];
    const int64_t step = (int64_t)gridDim.x * DG_BLOCK;
    uint64_t sum = 0;
    int64_t r = tab.off[seg] + (int64_t)blockIdx.x * DG_BLOCK + tid;
    for (; r + 3 * step < hi; r += 4 * step) {              // four rows in flight: the mixing chain of a row waits for its load
        DgRow v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const DgRow*>(coords + 3 * (r + j * step));
#pragma unroll
        for (int j = 0; j < 4; ++j) sum += dg_row(v[j].x, v[j].y, v[j].z, ox, oy, oz);
    }
    for (; r < hi; r += step) {
        const DgRow v = *reinterpret_cast<const DgRow*>(coords + 3 * r);
        sum += dg_row(v.x, v.y, v.z, ox, oy, oz);
    }
    // all 64 lanes of every wave are here
    sum = dg_wave_sum(sum);
    if ((tid & (LINR_WAVE - 1)) == 0) s_sum[tid / LINR_WAVE] = sum;
    __syncthreads();
    if (tid == 0) {
        sum = s_sum[0];
#pragma unroll
        for (int w = 1; w < DG_BLOCK / LINR_WAVE; ++w) sum += s_sum[w];
        partial[(int64_t)seg * gridDim.x + blockIdx.x] = sum;
    }
}

// one wave per segment
__global__ __launch_bounds__(LINR_WAVE) void coords_digest_finish_k(const uint64_t* __restrict__ partial, int tiles, DgTab tab,
                                                                    uint64_t* __restrict__ digest) {
    const int seg = blockIdx.x;
    uint64_t sum = 0;
    for (int i = threadIdx.x; i < tiles; i += LINR_WAVE) sum += partial[(int64_t)seg * tiles + i];
    sum = dg_wave_sum(sum);
    if (threadIdx.x == 0) digest[seg] = dg_finish(sum, (uint64_t)(tab.off[seg + 1] - tab.off[seg]));
}

}  // namespace

extern "C" size_t linr_coords_digest_ws_bytes(int32_t n_seg) {
    if (n_seg < 1 || n_seg > LINR_DECODE_MAX_FRAMES) return 0;
    return (size_t)n_seg * DG_MAX_TILES * sizeof(uint64_t);
}

extern "C" int linr_coords_digest_segments(const int32_t* coords_dev, const int64_t* seg_off_h, int32_t n_seg, const int32_t* origins_h,
                                           uint64_t* digest_dev, void* ws, size_t ws_bytes, void* stream) {
    if (!seg_off_h || !digest_dev || !ws || n_seg < 1 || n_seg > LINR_DECODE_MAX_FRAMES || seg_off_h[0] < 0) return LINR_EINVAL;
    int64_t longest = 0;
    for (int i = 0; i < n_seg; ++i) {
        const int64_t len = seg_off_h[i + 1] - seg_off_h[i];
        if (len < 0) return LINR_EINVAL;
        longest = len > longest ? len : longest;
    }
    if (!coords_dev && longest > 0) return LINR_EINVAL;
    if ((((uintptr_t)coords_dev) & 3u) || (((uintptr_t)digest_dev) & 7u) || (((uintptr_t)ws) & 7u)) return LINR_EALIGN;
    if (ws_bytes < linr_coords_digest_ws_bytes(n_seg)) return LINR_ENOSPC;
    DgTab tab;
    for (int i = 0; i <= LINR_DECODE_MAX_FRAMES; ++i) tab.off[i] = seg_off_h[i < n_seg ? i : n_seg];
    for (int i = 0; i < LINR_DECODE_MAX_FRAMES; ++i)
        for (int a = 0; a < 3; ++a) tab.org[i][a] = (origins_h && i < n_seg) ? origins_h[3 * i + a] : 0;
    int64_t tiles = (longest + DG_BLOCK - 1) / DG_BLOCK;
    tiles = tiles < 1 ? 1 : (tiles > DG_MAX_TILES ? DG_MAX_TILES : tiles);
    hipStream_t s = (hipStream_t)stream;
    uint64_t* partial = (uint64_t*)ws;
    linr_poison_hook(s, PK_DECODE);
    coords_digest_k<<<dim3((unsigned)tiles, (unsigned)n_seg), DG_BLOCK, 0, s>>>(coords_dev, tab, partial);
    coords_digest_finish_k<<<n_seg, LINR_WAVE, 0, s>>>(partial, (int)tiles, tab, digest_dev);
    return linr_launch_rc();
}
