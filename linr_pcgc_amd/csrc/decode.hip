// The staged decoder.  The 8 decode stages of a frame object (decode_stages: stage forward, D2H, range decoders, H2D, occupancy
// column - or, in its device mode, stage forward and rc_decode_k of csrc/ac_device_dec.hip, with no host round trip; exported as
// linr_net_decode_stages for a frame's scales), and one scale of the decoder as ONE call (decoder.decode_one_frame's loop body, decoder.py:153-176): the kernel map of
// the coarser level's coordinates, the 7-neighbour features read off it, the 8 stages and the next level's coordinates
// (octree_level.upper_layer, models/module_utils.py:117-127: the children 2 p + (dx, dy, dz) of every occupied octant, sorted
// x-major).  Between two scales the caller only allocates the next workspace, so a frame's decode holds the Python GIL for a few
// hundred microseconds instead of ~7 ms.  linr_decode_scale does it for one frame and linr_decode_scale_batch for the frames of a GOP
// in lock step; they share everything between their argument checks and the child expansion (scale_middle: the workspace layout, the
// stage plan, the device decoders' upload, scale_prologue, decode_stages) and differ in the kernel map (one list / segments) and in the
// child expansion (radix sort / prefix sums).  linr_decode_opts picks chunked streams, the host threads and the device decoders.
// The _wide twins of the four scale entries take the model's hidden_channel_conv: 16 / 32 size the arena for, and run the stages on,
// the wide forwards of csrc/wide_fwd.hip; the plain entries are the twins at 8.
#include "common.h"
#include "layout.h"
#include "prof.h"
#include "ac_device_dec.h"
#include <hipcub/hipcub.hpp>
#include <vector>

#define TRY(e) do { int rc_ = (e); if (rc_) return rc_; } while (0)

// decoded byte column -> float column k of the occupancy matrix [rows][8] (outside the namespace: it keeps the name that kernel
// traces have known it by)
__global__ __launch_bounds__(LINR_BLOCK) void occ_col_from_u8_k(const uint8_t* __restrict__ sym, int64_t n, float* __restrict__ occ_col) {
    const int64_t r = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (r < n) occ_col[r * 8] = (float)sym[r];
}

namespace {

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// the child expansion's part of the workspace: byte offsets into it
struct SortWs { size_t cnt, pos, keys0, keys1, cub, total, cub_bytes; };       // one frame: count, scan, keys, radix sort
struct ChildWs { size_t cnt, sum, bounds, cub, total, cub_bytes; };            // frames in lock step: pair counts, one scan
ChildWs child_layout(int64_t n);

size_t cub_bytes_for(int64_t n) {
    size_t a = 0, b = 0;
    // the scan runs over n + 1 items (linr_decode_scale), the sort over at most 8 n keys: reserve for exactly those calls
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, a, (const int32_t*)nullptr, (int32_t*)nullptr, (int)((n > 0 ? n : 1) + 1));
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)(8 * (n > 0 ? n : 1)), 0, 63);
    return a > b ? a : b;
}

SortWs sort_layout(int64_t n) {
    SortWs w;
    size_t cur = 0;
    auto take = [&](size_t bytes) { size_t o = cur; cur += up256(bytes); return o; };
    w.cnt = take((size_t)(n + 1) * 4);
    w.pos = take((size_t)(n + 1) * 4);
    w.keys0 = take((size_t)8 * n * 8);
    w.keys1 = take((size_t)8 * n * 8);
    w.cub_bytes = cub_bytes_for(n);
    w.cub = take(w.cub_bytes);
    w.total = cur;
    return w;
}

// byte offsets of one decoder scale of n rows into the caller's workspace; the region `child` is laid out by sort (linr_decode_scale)
// or by scan (linr_decode_scale_batch), whichever layout() was asked for: `is_scan` says which member is set
struct ScaleWs {
    size_t nbr, lo, mask, feat, occ, probs, sdev, kws, child, arena, total;
    size_t sbytes, tab;             // device decoders only (behind everything else): the scale's stream bytes, the entry table
    int64_t ld;
    size_t arena_bytes;
    bool is_scan;
    union { SortWs sort; ChildWs scan; };
};

// stream_bytes >= 0: with the device decoders' two regions - the stream bytes padded to 256 bytes (at least one such block, so this
// layout is the host decoders' plus 512 bytes or more) plus one 256-byte window, so that every aligned window a wave could ask for
// lies inside, and n_entries table entries
// hidden: 8, or 16 / 32 for the arena of the wide forwards (csrc/wide_fwd.hip)
ScaleWs layout(int64_t n, int block_layers, int bf16, bool scan, int hidden, int64_t stream_bytes = -1, int64_t n_entries = 0) {
    ScaleWs w;
    w.ld = (n + 63) / 64 * 64;
    size_t cur = 0;
    auto take = [&](size_t bytes) { size_t o = cur; cur += up256(bytes); return o; };
    w.nbr = take((size_t)27 * w.ld * 4);
    w.lo = take((size_t)9 * w.ld * 4);
    w.mask = take((size_t)w.ld * 4);
    w.feat = take((size_t)n * 7 * 4);
    w.occ = take((size_t)(n + 1) * 8 * 4);
    w.probs = take((size_t)8 * n * 4);
    w.sdev = take((size_t)n);
    w.kws = take(linr_kmap_workspace_bytes(n));
    w.is_scan = scan;
    if (scan) w.scan = child_layout(n); else w.sort = sort_layout(n);
    w.child = take(scan ? w.scan.total : w.sort.total);
    w.arena_bytes = hidden != 8 ? linr_net_wide_arena_bytes(n, hidden, block_layers, bf16)
                                : bf16 ? linr_net_bf16_arena_bytes(n, block_layers) : linr_net_arena_bytes(n, block_layers);
    w.arena = take(w.arena_bytes);
    w.sbytes = w.tab = cur;
    if (stream_bytes >= 0) {
        w.sbytes = take(up256((size_t)(stream_bytes > 0 ? stream_bytes : 1)) + 256);
        w.tab = take(sizeof(linr_rc_dec_entry) * (size_t)n_entries);
    }
    w.total = cur;
    return w;
}

// the frame object of one decoder scale (its host arrays live beside it)
struct ScaleFrame { linr_frame f; int64_t row_off[2]; int32_t sidx[1]; };

// Everything of a decoder scale in front of its stages: the kernel map of the n rows of `coord` (padding columns of nbr / lo / mask:
// no neighbour) - of one list, or with seg_off_h of n_seg lists back to back whose rows never see each other -, its compressed form,
// the scale context's features, the zeroed occupancy and the one-scale frame over them.
int scale_prologue(const int32_t* coord, int64_t n, const int64_t* seg_off_h, int n_seg, int scale_idx, int model_scale_num,
                   int block_layers, char* base, const ScaleWs& w, ScaleFrame& sf, hipStream_t s) {
    int32_t* nbr = (int32_t*)(base + w.nbr);
    int32_t* lo = (int32_t*)(base + w.lo);
    uint32_t* mask = (uint32_t*)(base + w.mask);
    float* feat = (float*)(base + w.feat);
    float* occ_buf = (float*)(base + w.occ);
    TRY(linr_hip_rc(hipMemsetAsync(nbr, 0xFF, (size_t)27 * w.ld * 4, s)));
    TRY(linr_hip_rc(hipMemsetAsync(lo, 0, w.mask + (size_t)w.ld * 4 - w.lo, s)));            // lo and mask are adjacent
    if (seg_off_h) {
        TRY(linr_kmap_build_segments(coord, seg_off_h, n_seg, nbr, w.ld, base + w.kws, linr_kmap_workspace_bytes(n), s));
    } else {
        linr_poison_hook(s, PK_DECODE);
        TRY(linr_kmap_build(coord, n, nbr, w.ld, 0, base + w.kws, linr_kmap_workspace_bytes(n), s));
    }
    TRY(linr_kmap_compress(nbr, w.ld, n, lo, mask, w.ld, s));
    TRY(linr_kmap_offset_feat(nbr, w.ld, 0, n, feat, s));
    TRY(linr_hip_rc(hipMemsetAsync(occ_buf, 0, (size_t)(n + 1) * 8 * 4, s)));
    sf.row_off[0] = 0; sf.row_off[1] = n; sf.sidx[0] = scale_idx;
    linr_frame& f = sf.f;
    f.rows = n; f.n_scales = 1; f.model_scale_num = model_scale_num; f.block_layers = block_layers; f.flags = LINR_FRAME_OCC_PADDED;
    f.row_off_h = sf.row_off; f.scale_idx_h = sf.sidx; f.nbr = nbr; f.nbr_ld = w.ld; f.nbr_lo = lo; f.nbr_mask = mask;
    f.offset_feat = feat; f.occ = occ_buf + 8; f.nbr8t = nullptr;     // zero row in front of the occupancy (LINR_FRAME_OCC_PADDED)
    return 0;
}

// cnt[r] = occupied octants of row r (cnt[n] = 0 closes the scan)
__global__ __launch_bounds__(LINR_BLOCK) void child_count_k(const float* __restrict__ occ, int64_t n, int32_t* __restrict__ cnt) {
    const int64_t r = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (r > n) return;
    int c = 0;
    if (r < n) {
        const float4 a = *reinterpret_cast<const float4*>(occ + r * 8);
        const float4 b = *reinterpret_cast<const float4*>(occ + r * 8 + 4);
        c = (a.x != 0.f) + (a.y != 0.f) + (a.z != 0.f) + (a.w != 0.f) + (b.x != 0.f) + (b.y != 0.f) + (b.z != 0.f) + (b.w != 0.f);
    }
    cnt[r] = c;
}

// key of child 2 p + (dx, dy, dz), octant index 4 dx + 2 dy + dz (module_utils.py:90-91), x-major with B bits per axis
__global__ __launch_bounds__(LINR_BLOCK) void child_keys_k(const int32_t* __restrict__ coord, const float* __restrict__ occ,
                                                           const int32_t* __restrict__ pos, int64_t n, int bits,
                                                           uint64_t* __restrict__ keys) {
    const int64_t r = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (r >= n) return;
    const uint64_t x = 2u * (uint32_t)coord[3 * r], y = 2u * (uint32_t)coord[3 * r + 1], z = 2u * (uint32_t)coord[3 * r + 2];
    int o = pos[r];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (occ[r * 8 + k] != 0.f)
            keys[o++] = ((x + (uint64_t)(k >> 2)) << (2 * bits)) | ((y + (uint64_t)((k >> 1) & 1)) << bits) | (z + (uint64_t)(k & 1));
}

__global__ __launch_bounds__(LINR_BLOCK) void keys_to_coord_k(const uint64_t* __restrict__ keys, const int32_t* __restrict__ total,
                                                              int bits, int32_t* __restrict__ xyz, int64_t cap) {
    const int64_t i = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    const int64_t m = *total < cap ? *total : cap;
    if (i >= m) return;
    const uint64_t k = keys[i], msk = ((uint64_t)1 << bits) - 1;
    xyz[3 * i] = (int32_t)(k >> (2 * bits));
    xyz[3 * i + 1] = (int32_t)((k >> bits) & msk);
    xyz[3 * i + 2] = (int32_t)(k & msk);
}

// The range decoders of the 8 stages: entry e of stage k decodes n[e] symbols from in[e] / len[e] against p[e] into s[e], the
// entries [first[k], first[k + 1]).  Without chunks (chunk_symbols 0) an entry is a segment's whole stream k; with them a stream of
// more than chunk_symbols symbols is cut by the checked parser (linr_stream_split_chunks) and every chunk is an entry of its own, its
// rows those behind the chunks in front of it.  An empty segment is left out with its streams unread.
#define RC_THREAD_SYMBOLS 65536
struct StagePlan {
    std::vector<const float*> p;
    std::vector<uint8_t*> s;
    std::vector<const uint8_t*> in;
    std::vector<int64_t> n, len;
    std::vector<int64_t> row;       // the entry's first row
    std::vector<int32_t> stream;    // the stream it lies in: 8 * segment + stage
    int64_t first[9];
    int64_t symbols[8];             // of stage k
    bool chunked;
};

int plan_stages(const int64_t* seg_off_h, int n_seg, const uint8_t* const* streams_h, const int64_t* stream_len_h, int64_t chunk_symbols,
                const float* p_pinned, uint8_t* s_pinned, StagePlan& plan) {
    std::vector<const uint8_t*> cp;
    std::vector<int64_t> cl;
    plan.chunked = chunk_symbols > 0;
    for (int k = 0; k < 8; ++k) {
        plan.first[k] = (int64_t)plan.n.size();
        plan.symbols[k] = 0;
        for (int i = 0; i < n_seg; ++i) {
            const int64_t r0 = seg_off_h[i], n = seg_off_h[i + 1] - r0;
            if (n <= 0) continue;
            const int64_t nc = linr_stream_chunk_count(n, chunk_symbols);
            if (nc < 0) return (int)nc;
            cp.resize((size_t)nc);
            cl.resize((size_t)nc);
            const int64_t got = linr_stream_split_chunks(streams_h[i * 8 + k], stream_len_h[i * 8 + k], n, chunk_symbols, cp.data(),
                                                         cl.data(), nc);
            if (got < 0) return (int)got;
            plan.symbols[k] += n;
            for (int64_t j = 0; j < nc; ++j) {
                const int64_t a = j * chunk_symbols;              // (one chunk: a = 0 whatever chunk_symbols is)
                if (p_pinned) {                                   // (the device decoders address rows, not host buffers)
                    plan.p.push_back(p_pinned + r0 + a);
                    plan.s.push_back(s_pinned + r0 + a);
                }
                plan.row.push_back(r0 + a);
                plan.stream.push_back((int32_t)(i * 8 + k));
                plan.n.push_back(nc == 1 ? n : (n - a < chunk_symbols ? n - a : chunk_symbols));
                plan.in.push_back(cp[(size_t)j]);
                plan.len.push_back(cl[(size_t)j]);
            }
        }
    }
    plan.first[8] = (int64_t)plan.n.size();
    return 0;
}

// The 8 decode stages of the frame object f, whose rows are n_seg segments (seg_off_h, HOST) with 8 streams each.  The stage's forward
// checks f (linr_frame_layout) before seg_off_h is read, so that may be f's own row_off_h: a caller that has checked its segments
// itself hands in the plan it made of them (`ready`), otherwise the plan is made behind the first forward.  The range decoders return
// the first failing entry's code (in order on this thread with n_threads 1); they decode the entries behind it, too, but those bytes
// stay in s_pinned: the call returns before anything more is launched.
// Device mode (dev != NULL, with `ready`): the entries of `ready` are in dev->tab and their bytes in dev->bytes on the device, and
// stage k is the forward followed by rc_decode_k over the stage's entries, which write column k of the occupancy from the
// probabilities where the forward left them: no copy, no host thread and NO synchronisation - the caller's child count is the one.
struct DeviceStages { const uint8_t* bytes; const linr_rc_dec_entry* tab; };

int decode_stages(const linr_frame* f, const float* params, const uint8_t* codes, float min_param, float max_param, void* arena,
                  size_t arena_bytes, const int64_t* seg_off_h, int n_seg, const uint8_t* const* streams_h,
                  const int64_t* stream_len_h, float* probs, float* p_pinned, uint8_t* s_pinned, uint8_t* s_dev, int n_threads,
                  const StagePlan* ready, hipStream_t s, const DeviceStages* dev = nullptr, int hidden = 8) {
    const int64_t R = f->rows;
    if (R == 0) return 0;
    float* occ = const_cast<float*>(f->occ);
    StagePlan own;
    for (int k = 0; k < 8; ++k) {
        // the stage's forward, one of four: width 8 or the channel-blocked widths, fp32 parameters or the uint8 codes
        if (hidden != 8 && codes) TRY(linr_net_forward_wide_bf16(f, codes, min_param, max_param, hidden, arena, arena_bytes, k, k + 1, probs, nullptr, s));
        else if (hidden != 8) TRY(linr_net_forward_wide(f, params, hidden, arena, arena_bytes, k, k + 1, probs, nullptr, s));
        else if (codes) TRY(linr_net_forward_bf16(f, codes, min_param, max_param, arena, arena_bytes, k, k + 1, probs, nullptr, s));
        else TRY(linr_net_forward(f, params, (float*)arena, arena_bytes, k, k + 1, probs, nullptr, s));
        if (dev) {
            linr_poison_hook(s, PK_DECODE);
            TRY(linr_rc_dec_launch(probs + (int64_t)k * R, dev->bytes, dev->tab + ready->first[k], (int32_t)(ready->first[k + 1] - ready->first[k]),
                                   occ + k, 8, nullptr, s));
            continue;
        }
        TRY(linr_hip_rc(hipMemcpyAsync(p_pinned, probs + (int64_t)k * R, (size_t)R * sizeof(float), hipMemcpyDeviceToHost, s)));
        TRY(linr_hip_rc(hipStreamSynchronize(s)));
        if (!ready) {
            TRY(plan_stages(seg_off_h, n_seg, streams_h, stream_len_h, 0, p_pinned, s_pinned, own));
            ready = &own;
        }
        const int64_t e = ready->first[k];
        // The batch entry starts its threads anew in every call, at some tens of microseconds each, so chunks get a thread per
        // RC_THREAD_SYMBOLS symbols of the stage (about 0.2 ms of decoding), not one per chunk: small scales stay on this thread.
        // (Without chunks the caller's count holds, as ever.)
        int threads = n_threads;
        if (ready->chunked && threads > 1 + ready->symbols[k] / RC_THREAD_SYMBOLS) threads = (int)(1 + ready->symbols[k] / RC_THREAD_SYMBOLS);
        TRY(linr_ac_decode_binary_batch(ready->p.data() + e, ready->n.data() + e, ready->in.data() + e, ready->len.data() + e,
                                        (int32_t)(ready->first[k + 1] - e), ready->s.data() + e, threads));
        TRY(linr_hip_rc(hipMemcpyAsync(s_dev, s_pinned, (size_t)R, hipMemcpyHostToDevice, s)));
        occ_col_from_u8_k<<<linr_grid(R, LINR_BLOCK), LINR_BLOCK, 0, s>>>(s_dev, R, occ + k);
        TRY(linr_launch_rc());
    }
    if (dev) return 0;
    return linr_hip_rc(hipStreamSynchronize(s));       // s_pinned / p_pinned may be reused by the caller right away
}

// The device decoders' side of a scale: the bytes of the plan's streams back to back in stream order, every entry of the
// plan as a table entry over them, checked stage by stage as linr_rc_decode_probs checks its table.  Host work only.
struct DevicePlan {
    std::vector<uint8_t> bytes;
    std::vector<linr_rc_dec_entry> ent;
};

int plan_device(const StagePlan& plan, int n_seg, const int64_t* seg_off_h, const uint8_t* const* streams_h, const int64_t* stream_len_h,
                int64_t rows, DevicePlan& d) {
    std::vector<int64_t> off((size_t)n_seg * 8 + 1, 0);
    for (int i = 0; i < n_seg; ++i)
        for (int k = 0; k < 8; ++k) {
            const size_t x = (size_t)i * 8 + k;
            const bool live = seg_off_h[i + 1] > seg_off_h[i];          // an empty segment's streams stay unread
            if (live && (stream_len_h[x] < 0 || (stream_len_h[x] > 0 && !streams_h[x]))) return LINR_EINVAL;
            off[x + 1] = off[x] + (live ? stream_len_h[x] : 0);
        }
    d.bytes.resize((size_t)off.back());
    for (size_t x = 0; x + 1 < off.size(); ++x)
        if (off[x + 1] > off[x]) memcpy(d.bytes.data() + off[x], streams_h[x], (size_t)(off[x + 1] - off[x]));
    d.ent.resize(plan.n.size());
    for (size_t e = 0; e < plan.n.size(); ++e) {
        const size_t x = (size_t)plan.stream[e];
        const int64_t in_off = off[x] + (plan.len[e] > 0 ? plan.in[e] - streams_h[x] : 0);
        d.ent[e] = linr_rc_dec_entry{plan.row[e], plan.n[e], in_off, plan.len[e], plan.row[e]};
    }
    if (plan.n.size() >= (size_t)INT32_MAX) return LINR_EINVAL;
    for (int k = 0; k < 8; ++k)
        TRY(linr_rc_dec_check(d.ent.data() + plan.first[k], (int32_t)(plan.first[k + 1] - plan.first[k]), rows, off.back(), rows));
    return 0;
}

// a stream synchronised when the scope is left early: the staging copy of the stream bytes must outlive its upload
struct SyncOnExit {
    hipStream_t s; bool armed;
    ~SyncOnExit() { if (armed) (void)hipStreamSynchronize(s); }
};

}  // namespace

extern "C" int linr_net_decode_stages(const linr_frame* f, const float* params, const uint8_t* codes, float min_param,
                                      float max_param, void* arena, size_t arena_bytes, const uint8_t* const* streams_h,
                                      const int64_t* stream_len_h, float* probs, float* p_pinned, uint8_t* s_pinned,
                                      uint8_t* s_dev, void* stream) {
    if (!f || !arena || !streams_h || !stream_len_h || !probs || !p_pinned || !s_pinned || !s_dev || !f->occ) return LINR_EINVAL;
    if (!codes && !params) return LINR_EINVAL;
    return decode_stages(f, params, codes, min_param, max_param, arena, arena_bytes, f->row_off_h, f->n_scales, streams_h, stream_len_h,
                         probs, p_pinned, s_pinned, s_dev, 1, nullptr, (hipStream_t)stream);
}

namespace {

int upload_device(const DevicePlan& keep, const DeviceStages& dev, hipStream_t s) {
    linr_poison_hook(s, PK_DECODE);
    if (!keep.bytes.empty())
        TRY(linr_hip_rc(hipMemcpyAsync(const_cast<uint8_t*>(dev.bytes), keep.bytes.data(), keep.bytes.size(), hipMemcpyHostToDevice, s)));
    return linr_rc_dec_upload(keep.ent.data(), (int32_t)keep.ent.size(), const_cast<linr_rc_dec_entry*>(dev.tab), s);
}

// What a scale entry hands the middle that both share: its n rows as n_seg segments (linr_decode_scale: its one, sf.row_off),
// the model, the streams, the caller's buffers and its options.  `segmented` (linr_decode_scale_batch): the kernel map of segments
// and the child region laid out for the scan; otherwise the kernel map of one list and the region of the sort.
struct ScaleArgs {
    const int32_t* coord; int64_t n; const int64_t* seg_off_h; int32_t n_seg; bool segmented;
    int32_t scale_idx, model_scale_num, block_layers, hidden;
    const float* params; const uint8_t* codes; float min_param, max_param;
    const uint8_t* const* streams_h; const int64_t* stream_len_h;
    void* ws; size_t ws_bytes; float* p_pinned; uint8_t* s_pinned;
    const linr_decode_opts* opts;
    hipStream_t s;
};

// What the middle leaves its entry for the child expansion (w, sf) and what has to live until the entry returns: `keep` owns the
// staging copy of the device decoders' stream bytes, and `guard` - the last member, so the first to go - synchronises before that
// copy is freed when the scale is left early.
struct ScaleRun {
    ScaleWs w; ScaleFrame sf; StagePlan plan; DevicePlan keep; SyncOnExit guard;
    explicit ScaleRun(hipStream_t s) : guard{s, false} {}
};

// A scale between its entry's own argument checks and its child expansion (n > 0): the remaining checks, the workspace layout, the
// plan of the 8 stages (a malformed chunk header is refused here, in front of the first launch), for the device decoders the plan's
// bytes and table into the workspace (laid out for exactly them: LINR_ENOSPC when ws_bytes does not reach) under the guard, the
// prologue and the stages.
int scale_middle(const ScaleArgs& a, ScaleRun& r) {
    static const linr_decode_opts plain = {0, 1, 0};
    const linr_decode_opts& o = a.opts ? *a.opts : plain;
    const bool device = o.device != 0;           // (then p_pinned, s_pinned and n_threads are unused)
    if (!a.coord || (!a.params && !a.codes) || !a.streams_h || !a.stream_len_h || !a.ws) return LINR_EINVAL;
    if (!device && (!a.p_pinned || !a.s_pinned)) return LINR_EINVAL;
    if (((uintptr_t)a.ws) & 255u) return LINR_EALIGN;
    const int bf16 = a.codes ? 1 : 0;
    r.w = layout(a.n, a.block_layers, bf16, a.segmented, a.hidden);
    if (a.ws_bytes < r.w.total) return LINR_ENOSPC;
    char* base = (char*)a.ws;
    float* p_pinned = device ? nullptr : a.p_pinned;
    uint8_t* s_pinned = device ? nullptr : a.s_pinned;
    TRY(plan_stages(a.seg_off_h, a.n_seg, a.streams_h, a.stream_len_h, o.chunk_symbols, p_pinned, s_pinned, r.plan));
    DeviceStages dev{nullptr, nullptr};
    if (device) {
        TRY(plan_device(r.plan, a.n_seg, a.seg_off_h, a.streams_h, a.stream_len_h, a.n, r.keep));
        r.w = layout(a.n, a.block_layers, bf16, a.segmented, a.hidden, (int64_t)r.keep.bytes.size(), (int64_t)r.keep.ent.size());
        if (a.ws_bytes < r.w.total) return LINR_ENOSPC;
        dev.bytes = (const uint8_t*)(base + r.w.sbytes);
        dev.tab = (const linr_rc_dec_entry*)(base + r.w.tab);
        r.guard.armed = true;
        TRY(upload_device(r.keep, dev, a.s));
    }
    TRY(scale_prologue(a.coord, a.n, a.segmented ? a.seg_off_h : nullptr, a.segmented ? a.n_seg : 0, a.scale_idx, a.model_scale_num,
                       a.block_layers, base, r.w, r.sf, a.s));
    return decode_stages(&r.sf.f, a.params, a.codes, a.min_param, a.max_param, base + r.w.arena, r.w.arena_bytes, a.seg_off_h, a.n_seg,
                         a.streams_h, a.stream_len_h, (float*)(base + r.w.probs), p_pinned, s_pinned, (uint8_t*)(base + r.w.sdev),
                         device ? 1 : o.n_threads, &r.plan, a.s, device ? &dev : nullptr, a.hidden);
}

// stream_bytes_total -1: the host decoders' layout; >= 0: the device decoders' (0 for anything else)
inline bool width_ok(int hidden) { return hidden == 8 || hidden == 16 || hidden == 32; }

size_t scale_ws_bytes(int64_t n, int32_t block_layers, int32_t bf16, bool scan, int hidden, int64_t stream_bytes_total, int64_t n_entries) {
    if (stream_bytes_total < -1 || (stream_bytes_total >= 0 && n_entries < 0) || !width_ok(hidden)) return 0;
    const ScaleWs w = layout(n, block_layers, bf16 ? 1 : 0, scan, hidden, stream_bytes_total, n_entries);
    if (hidden != 8 && w.arena_bytes == 0) return 0;          // (a depth the wide forwards do not have)
    return w.total + 256;
}

}  // namespace

extern "C" size_t linr_decode_scale_wide_ws_bytes(int64_t n, int32_t block_layers, int32_t bf16, int64_t stream_bytes_total, int64_t n_entries,
                                                  int32_t hidden) {
    if (n < 0 || block_layers < 1) return 0;
    return scale_ws_bytes(n, block_layers, bf16, false, hidden, stream_bytes_total, n_entries);
}

extern "C" size_t linr_decode_scale_ws_bytes(int64_t n, int32_t block_layers, int32_t bf16, int64_t stream_bytes_total, int64_t n_entries) {
    return linr_decode_scale_wide_ws_bytes(n, block_layers, bf16, stream_bytes_total, n_entries, 8);
}

extern "C" int linr_decode_scale_wide(const int32_t* coord, int64_t n, int32_t scale_idx, int32_t model_scale_num, int32_t block_layers,
                                      int32_t child_bits, const float* params, const uint8_t* codes, float min_param, float max_param,
                                      const uint8_t* const* streams_h, const int64_t* stream_len_h, void* ws, size_t ws_bytes,
                                      float* p_pinned, uint8_t* s_pinned, int32_t* child_xyz, int64_t child_cap, int64_t* child_n_h,
                                      const linr_decode_opts* opts, int32_t hidden, void* stream) {
    if (n < 0 || !child_n_h || child_bits < 1 || child_bits > 21 || block_layers < 1 || !width_ok(hidden)) return LINR_EINVAL;
    *child_n_h = 0;
    if (n == 0) return 0;
    // (one row looser than linr_rows_fit32, which the executor's frame check then applies to the frame built in the prologue)
    if (!child_xyz || child_cap < 0 || n >= ((int64_t)1 << 27)) return LINR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    ScaleRun r(s);
    r.sf.row_off[0] = 0; r.sf.row_off[1] = n;          // the one segment
    const ScaleArgs a{coord, n, r.sf.row_off, 1, false, scale_idx, model_scale_num, block_layers, hidden, params, codes, min_param, max_param,
                      streams_h, stream_len_h, ws, ws_bytes, p_pinned, s_pinned, opts, s};
    TRY(scale_middle(a, r));
    // upper_layer: children of the occupied octants, sorted x-major
    const SortWs& w = r.w.sort;
    const float* occ = r.sf.f.occ;
    char* cbase = (char*)ws + r.w.child;
    int32_t* cnt = (int32_t*)(cbase + w.cnt);
    int32_t* pos = (int32_t*)(cbase + w.pos);
    uint64_t* keys0 = (uint64_t*)(cbase + w.keys0);
    uint64_t* keys1 = (uint64_t*)(cbase + w.keys1);
    linr_poison_hook(s, PK_DECODE);
    child_count_k<<<linr_grid(n + 1, LINR_BLOCK), LINR_BLOCK, 0, s>>>(occ, n, cnt);
    size_t cb = w.cub_bytes;
    TRY(linr_hip_rc(hipcub::DeviceScan::ExclusiveSum(cbase + w.cub, cb, cnt, pos, (int)(n + 1), s)));
    int32_t total = 0;
    TRY(linr_hip_rc(hipMemcpyAsync(&total, pos + n, sizeof(int32_t), hipMemcpyDeviceToHost, s)));
    child_keys_k<<<linr_grid(n, LINR_BLOCK), LINR_BLOCK, 0, s>>>(coord, occ, pos, n, child_bits, keys0);
    TRY(linr_hip_rc(hipStreamSynchronize(s)));                  // `total` is on the host now
    r.guard.armed = false;
    if (total > child_cap) return LINR_ENOSPC;
    if (total > 0) {
        cb = w.cub_bytes;
        TRY(linr_hip_rc(hipcub::DeviceRadixSort::SortKeys(cbase + w.cub, cb, keys0, keys1, (int)total, 0, 3 * child_bits, s)));
        keys_to_coord_k<<<linr_grid(total, LINR_BLOCK), LINR_BLOCK, 0, s>>>(keys1, pos + n, child_bits, child_xyz, child_cap);
    }
    *child_n_h = total;
    return linr_launch_rc();
}

extern "C" int linr_decode_scale(const int32_t* coord, int64_t n, int32_t scale_idx, int32_t model_scale_num, int32_t block_layers,
                                 int32_t child_bits, const float* params, const uint8_t* codes, float min_param, float max_param,
                                 const uint8_t* const* streams_h, const int64_t* stream_len_h, void* ws, size_t ws_bytes,
                                 float* p_pinned, uint8_t* s_pinned, int32_t* child_xyz, int64_t child_cap, int64_t* child_n_h,
                                 const linr_decode_opts* opts, void* stream) {
    return linr_decode_scale_wide(coord, n, scale_idx, model_scale_num, block_layers, child_bits, params, codes, min_param, max_param,
                                  streams_h, stream_len_h, ws, ws_bytes, p_pinned, s_pinned, child_xyz, child_cap, child_n_h, opts, 8, stream);
}

// ---- the same for the frames of a GOP in lock step: one scale of n_frames frames per call, children without a sort ------------------
// (decoder.decode_one_frame's loop body, decoder.py:153-176, and octree_level.upper_layer, models/module_utils.py:117-127, for all
// frames of a group at once.)  The rows of the group are sorted by (frame, x, y, z), so the children are, too, once every row knows
// where its own go: with c_q[r] = the children of row r in the (dx, dy) pair q = 2 dx + dy, S_q their exclusive prefix sums and
// T = S_0 + S_1 + S_2 + S_3, the children of the (frame, x) run [xs, xe) start at T[xs]; inside it come all dx = 0 children, then
// all dx = 1; inside a dx half the (frame, x, y) runs [ys, ye) in order, each with its dy = 0 children first; inside a (dx, dy)
// pair the rows in z order, dz = 0 before dz = 1.
namespace {

struct alignas(16) Cnt4 { int32_t q[4]; };
struct Cnt4Sum {
    __host__ __device__ __forceinline__ Cnt4 operator()(const Cnt4& a, const Cnt4& b) const {
        return Cnt4{{a.q[0] + b.q[0], a.q[1] + b.q[1], a.q[2] + b.q[2], a.q[3] + b.q[3]}};
    }
};

ChildWs child_layout(int64_t n) {
    ChildWs w;
    size_t cur = 0;
    auto take = [&](size_t bytes) { size_t o = cur; cur += up256(bytes); return o; };
    w.cnt = take((size_t)(n + 1) * sizeof(Cnt4));
    w.sum = take((size_t)(n + 1) * sizeof(Cnt4));
    w.bounds = take((size_t)(LINR_DECODE_MAX_FRAMES + 1) * 4);
    w.cub_bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveScan(nullptr, w.cub_bytes, (const Cnt4*)nullptr, (Cnt4*)nullptr, Cnt4Sum(), Cnt4{{0, 0, 0, 0}},
                                            (int)(n + 1));
    w.cub = take(w.cub_bytes);
    w.total = cur;
    return w;
}

// cnt[r].q[2 dx + dy] = occupied octants 4 dx + 2 dy, 4 dx + 2 dy + 1 of row r (cnt[n] = 0 closes the scan)
__global__ __launch_bounds__(LINR_BLOCK) void child_pair_count_k(const float* __restrict__ occ, int64_t n, Cnt4* __restrict__ cnt) {
    const int64_t r = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (r > n) return;
    Cnt4 c = {{0, 0, 0, 0}};
    if (r < n) {
        const float4 a = *reinterpret_cast<const float4*>(occ + r * 8);
        const float4 b = *reinterpret_cast<const float4*>(occ + r * 8 + 4);
        c.q[0] = (a.x != 0.f) + (a.y != 0.f);
        c.q[1] = (a.z != 0.f) + (a.w != 0.f);
        c.q[2] = (b.x != 0.f) + (b.y != 0.f);
        c.q[3] = (b.z != 0.f) + (b.w != 0.f);
    }
    cnt[r] = c;
}

// out[i] = T[first row of segment i], i <= n_seg: the segments' child offsets (the last one is the total)
__global__ void child_bounds_k(const Cnt4* __restrict__ S, LinrSegTab tab, int n_seg, int32_t* __restrict__ out) {
    const int i = threadIdx.x;
    if (i > n_seg) return;
    int32_t row = 0;
#pragma unroll
    for (int j = 0; j <= LINR_DECODE_MAX_FRAMES; ++j) row = j == i ? tab.off[j] : row;
    const Cnt4 s = S[row];
    out[i] = s.q[0] + s.q[1] + s.q[2] + s.q[3];
}

struct __attribute__((packed, aligned(4))) Xyz { int32_t x, y, z; };
struct __attribute__((packed, aligned(4))) Xyz2 { Xyz a, b; };

// lane = row: the bounds of the row's (frame, x) and (frame, x, y) runs by searches in the coordinates, then its children
__global__ __launch_bounds__(LINR_BLOCK) void children_scatter_k(const int32_t* __restrict__ coord, const float* __restrict__ occ,
                                                                 const Cnt4* __restrict__ S, int64_t n, LinrSegTab tab,
                                                                 int32_t* __restrict__ child, int64_t cap) {
    const int64_t r64 = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (r64 >= n) return;
    const int32_t r = (int32_t)r64;
    int32_t s0, s1;
    linr_seg_bounds(tab, r, s0, s1);
    const int32_t X = coord[3 * r64], Y = coord[3 * r64 + 1], Z = coord[3 * r64 + 2];
    int32_t lo = s0, hi = r;                 // xs: first row of the segment with x >= X
    while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (coord[3 * (int64_t)mid] < X) lo = mid + 1; else hi = mid; }
    const int32_t xs = lo;
    lo = r + 1; hi = s1;                     // xe: first row behind r with x > X (or the segment's end)
    while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (coord[3 * (int64_t)mid] <= X) lo = mid + 1; else hi = mid; }
    const int32_t xe = lo;
    lo = xs; hi = r;                         // ys: first row of the x run with y >= Y
    while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (coord[3 * (int64_t)mid + 1] < Y) lo = mid + 1; else hi = mid; }
    const int32_t ys = lo;
    lo = r + 1; hi = xe;                     // ye: first row behind r in the x run with y > Y (or the run's end)
    while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (coord[3 * (int64_t)mid + 1] <= Y) lo = mid + 1; else hi = mid; }
    const int32_t ye = lo;
    const Cnt4 Sxs = S[xs], Sxe = S[xe], Sys = S[ys], Sye = S[ye], Sr = S[r];
    const float4 oa = *reinterpret_cast<const float4*>(occ + r64 * 8);
    const float4 ob = *reinterpret_cast<const float4*>(occ + r64 * 8 + 4);
    const bool o[8] = {oa.x != 0.f, oa.y != 0.f, oa.z != 0.f, oa.w != 0.f, ob.x != 0.f, ob.y != 0.f, ob.z != 0.f, ob.w != 0.f};
    const int32_t t_xs = Sxs.q[0] + Sxs.q[1] + Sxs.q[2] + Sxs.q[3];
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
        const int32_t half = t_xs + (dx ? (Sxe.q[0] - Sxs.q[0]) + (Sxe.q[1] - Sxs.q[1]) : 0) + (Sys.q[2 * dx] - Sxs.q[2 * dx]) +
                             (Sys.q[2 * dx + 1] - Sxs.q[2 * dx + 1]);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int q = 2 * dx + dy;
            const int64_t pos = half + (dy ? Sye.q[2 * dx] - Sys.q[2 * dx] : 0) + (Sr.q[q] - Sys.q[q]);
            const bool o0 = o[2 * q], o1 = o[2 * q + 1];
            const Xyz c0 = {2 * X + dx, 2 * Y + dy, 2 * Z}, c1 = {2 * X + dx, 2 * Y + dy, 2 * Z + 1};
            if (o0 && o1 && pos + 1 < cap) {
                *reinterpret_cast<Xyz2*>(child + 3 * pos) = Xyz2{c0, c1};
            } else {
                if (o0 && pos < cap) *reinterpret_cast<Xyz*>(child + 3 * pos) = c0;
                if (o1 && pos + (o0 ? 1 : 0) < cap) *reinterpret_cast<Xyz*>(child + 3 * (pos + (o0 ? 1 : 0))) = c1;
            }
        }
    }
}

// the body of linr_children_segments behind its argument checks (n > 0)
int children_segments(const int32_t* coord, const float* occ, const LinrSegTab& tab, int64_t n, int n_seg, int32_t* child_xyz,
                      int64_t child_cap, int64_t* child_off_h, char* base, const ChildWs& w, hipStream_t s) {
    Cnt4* cnt = (Cnt4*)(base + w.cnt);
    Cnt4* sum = (Cnt4*)(base + w.sum);
    int32_t* bounds = (int32_t*)(base + w.bounds);
    linr_poison_hook(s, PK_DECODE);
    child_pair_count_k<<<linr_grid(n + 1, LINR_BLOCK), LINR_BLOCK, 0, s>>>(occ, n, cnt);
    size_t cb = w.cub_bytes;
    int rc = linr_hip_rc(hipcub::DeviceScan::ExclusiveScan(base + w.cub, cb, cnt, sum, Cnt4Sum(), Cnt4{{0, 0, 0, 0}}, (int)(n + 1), s));
    if (rc) return rc;
    child_bounds_k<<<1, 128, 0, s>>>(sum, tab, n_seg, bounds);
    int32_t bounds_h[LINR_DECODE_MAX_FRAMES + 1];
    rc = linr_hip_rc(hipMemcpyAsync(bounds_h, bounds, (size_t)(n_seg + 1) * 4, hipMemcpyDeviceToHost, s));
    if (rc) return rc;
    children_scatter_k<<<linr_grid(n, LINR_BLOCK), LINR_BLOCK, 0, s>>>(coord, occ, sum, n, tab, child_xyz, child_cap);
    rc = linr_launch_rc();
    if (rc) return rc;
    rc = linr_hip_rc(hipStreamSynchronize(s));                  // the offsets are on the host now
    if (rc) return rc;
    for (int i = 0; i <= n_seg; ++i) child_off_h[i] = bounds_h[i];
    return bounds_h[n_seg] > child_cap ? LINR_ENOSPC : 0;
}

}  // namespace

extern "C" size_t linr_children_segments_ws_bytes(int64_t n) { return n < 0 || n >= ((int64_t)1 << 26) ? 0 : child_layout(n).total; }

extern "C" int linr_children_segments(const int32_t* coords, const float* occ, const int64_t* seg_off_h, int32_t n_seg,
                                      int32_t* child_xyz, int64_t child_cap, int64_t* child_off_h, void* ws, size_t ws_bytes,
                                      void* stream) {
    LinrSegTab tab;
    int64_t n = 0;
    const int rc = linr_seg_tab(seg_off_h, n_seg, &tab, &n);
    if (rc) return rc;
    if (!child_off_h || child_cap < 0 || n >= ((int64_t)1 << 26)) return LINR_EINVAL;
    for (int i = 0; i <= n_seg; ++i) child_off_h[i] = 0;
    if (n == 0) return 0;
    if (!coords || !occ || !child_xyz || !ws) return LINR_EINVAL;
    if ((((uintptr_t)ws) & 255u) || !linr_aligned16(occ)) return LINR_EALIGN;
    const ChildWs w = child_layout(n);
    if (ws_bytes < w.total) return LINR_ENOSPC;
    return children_segments(coords, occ, tab, n, n_seg, child_xyz, child_cap, child_off_h, (char*)ws, w, (hipStream_t)stream);
}

extern "C" size_t linr_decode_scale_batch_wide_ws_bytes(int64_t n_total, int32_t n_frames, int32_t block_layers, int32_t bf16,
                                                        int64_t stream_bytes_total, int64_t n_entries, int32_t hidden) {
    if (n_total < 0 || n_total >= ((int64_t)1 << 26) || n_frames < 1 || n_frames > LINR_DECODE_MAX_FRAMES || block_layers < 1) return 0;
    return scale_ws_bytes(n_total, block_layers, bf16, true, hidden, stream_bytes_total, n_entries);
}

extern "C" size_t linr_decode_scale_batch_ws_bytes(int64_t n_total, int32_t n_frames, int32_t block_layers, int32_t bf16,
                                                   int64_t stream_bytes_total, int64_t n_entries) {
    return linr_decode_scale_batch_wide_ws_bytes(n_total, n_frames, block_layers, bf16, stream_bytes_total, n_entries, 8);
}

extern "C" int linr_decode_scale_batch_wide(const int32_t* coord, const int64_t* seg_off_h, int32_t n_frames, int32_t scale_idx,
                                            int32_t model_scale_num, int32_t block_layers, const float* params, const uint8_t* codes,
                                            float min_param, float max_param, const uint8_t* const* streams_h, const int64_t* stream_len_h,
                                            void* ws, size_t ws_bytes, float* p_pinned, uint8_t* s_pinned, int32_t* child_xyz,
                                            int64_t child_cap, int64_t* child_off_h, const linr_decode_opts* opts, int32_t hidden,
                                            void* stream) {
    LinrSegTab tab;
    int64_t n = 0;
    const int rc = linr_seg_tab(seg_off_h, n_frames, &tab, &n);
    if (rc) return rc;
    if (!child_off_h || block_layers < 1 || child_cap < 0 || !width_ok(hidden)) return LINR_EINVAL;
    const int64_t ld = (n + 63) / 64 * 64;
    if (!linr_cmap_fits32(ld) || !linr_rows_fit32(n)) return LINR_EINVAL;
    for (int i = 0; i <= n_frames; ++i) child_off_h[i] = 0;
    if (n == 0) return 0;
    if (!child_xyz) return LINR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    ScaleRun r(s);
    const ScaleArgs a{coord, n, seg_off_h, n_frames, true, scale_idx, model_scale_num, block_layers, hidden, params, codes, min_param, max_param,
                      streams_h, stream_len_h, ws, ws_bytes, p_pinned, s_pinned, opts, s};
    TRY(scale_middle(a, r));
    // (children_segments synchronises when it succeeds; the guard covers the ways out in front of that)
    return children_segments(coord, r.sf.f.occ, tab, n, n_frames, child_xyz, child_cap, child_off_h, (char*)ws + r.w.child, r.w.scan, s);
}

extern "C" int linr_decode_scale_batch(const int32_t* coord, const int64_t* seg_off_h, int32_t n_frames, int32_t scale_idx,
                                       int32_t model_scale_num, int32_t block_layers, const float* params, const uint8_t* codes,
                                       float min_param, float max_param, const uint8_t* const* streams_h, const int64_t* stream_len_h,
                                       void* ws, size_t ws_bytes, float* p_pinned, uint8_t* s_pinned, int32_t* child_xyz,
                                       int64_t child_cap, int64_t* child_off_h, const linr_decode_opts* opts, void* stream) {
    return linr_decode_scale_batch_wide(coord, seg_off_h, n_frames, scale_idx, model_scale_num, block_layers, params, codes, min_param,
                                        max_param, streams_h, stream_len_h, ws, ws_bytes, p_pinned, s_pinned, child_xyz, child_cap,
                                        child_off_h, opts, 8, stream);
}

// ---- sorted unique coordinate list, optionally of the parents (coords >> shift); one octree level as one call ------------------------
// torch.unique(dim=0) of custom_dataset.py:271-282 (the input cloud, shift 0) and of octree_level.forward (models/module_utils.py:
// 92,103: parent = unique(floor(child / 2)), shift 1): compact x-major keys (x << 2b | y << b | z with b = the bits a coordinate
// needs, so the radix sort runs over 3 b bits, not 63), radix sort, unique, decode.  Before these entries the host mirror spent ~30
// small torch launches per octree level on it (tools/stage_split.py: 2.5 ms per loot10 frame).
namespace {
// K = uint32_t when the compact key fits (3 b <= 32: every level of a 10-bit cloud, the parent levels of an 11-bit one), else uint64_t
template <typename K>
__global__ __launch_bounds__(LINR_BLOCK) void su_keys_k(const int32_t* __restrict__ c, int64_t n, const int32_t* __restrict__ origin, int shift,
                                                        int b, K* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int ox = origin ? origin[0] : 0, oy = origin ? origin[1] : 0, oz = origin ? origin[2] : 0;
    const uint64_t x = (uint64_t)((c[3 * i] - ox) >> shift), y = (uint64_t)((c[3 * i + 1] - oy) >> shift), z = (uint64_t)((c[3 * i + 2] - oz) >> shift);
    keys[i] = (K)((x << (2 * b)) | (y << b) | z);
}
template <typename K>
__global__ __launch_bounds__(LINR_BLOCK) void su_decode_k(const K* __restrict__ keys, const int* __restrict__ num, int64_t cap, int b,
                                                          int32_t* __restrict__ out, int64_t* __restrict__ count) {
    const int64_t m = *num < cap ? *num : cap;
    const int64_t i = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (i == 0) *count = m;
    if (i >= m) return;
    const uint64_t k = keys[i], mk = ((uint64_t)1 << b) - 1;
    out[3 * i] = (int32_t)(k >> (2 * b));
    out[3 * i + 1] = (int32_t)((k >> b) & mk);
    out[3 * i + 2] = (int32_t)(k & mk);
}
// child occupancy from the sorted compact CHILD keys (b bits per coordinate) and the sorted unique compact PARENT keys (b - 1 bits):
// octree_occ_k of kmap.hip with the parent count read on the device
template <typename KC, typename KP>
__global__ __launch_bounds__(LINR_BLOCK) void su_occ_k(const KC* __restrict__ ck, int64_t m, const KP* __restrict__ pk,
                                                       const int* __restrict__ num, int b, float* __restrict__ occ) {
    const int64_t n = *num;
    const int64_t idx = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x;
    if (idx >= 4 * n) return;
    const int q = (int)(idx & 3);
    const int64_t j = idx >> 2;
    const int dx = q >> 1, dy = q & 1, pb = b - 1;
    const uint64_t k = pk[j], mk = ((uint64_t)1 << pb) - 1;
    const uint64_t px = k >> (2 * pb), py = (k >> pb) & mk, pz = k & mk;
    const uint64_t key0 = ((2 * px + dx) << (2 * b)) | ((2 * py + dy) << b) | (2 * pz);
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((uint64_t)ck[mid] < key0) lo = mid + 1; else hi = mid;
    }
    const bool h0 = lo < m && (uint64_t)ck[lo] == key0;
    if (h0) ++lo;
    const bool h1 = lo < m && (uint64_t)ck[lo] == key0 + 1;
    occ[j * 8 + 4 * dx + 2 * dy] = h0 ? 1.0f : 0.0f;
    occ[j * 8 + 4 * dx + 2 * dy + 1] = h1 ? 1.0f : 0.0f;
}
size_t su_cub_bytes(int64_t n) {
    size_t a = 0, b = 0, c = 0, d = 0;
    const int m = (int)(n > 0 ? n : 1);
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr, m, 0, 60);
    (void)hipcub::DeviceSelect::Unique(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int*)nullptr, m);
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, c, (const uint32_t*)nullptr, (uint32_t*)nullptr, m, 0, 32);
    (void)hipcub::DeviceSelect::Unique(nullptr, d, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int*)nullptr, m);
    a = a > b ? a : b;
    c = c > d ? c : d;
    return a > c ? a : c;
}
// keys of (coords >> shift) into k0, sorted into k1, unique back into k0, *num = how many
template <typename K>
int su_sort_unique(const int32_t* coords, int64_t n, const int32_t* origin, int shift, int b, K* k0, K* k1, int* num, void* cub, size_t cb,
                   hipStream_t s) {
    su_keys_k<K><<<linr_grid(n, LINR_BLOCK), LINR_BLOCK, 0, s>>>(coords, n, origin, shift, b, k0);
    int rc = linr_hip_rc(hipcub::DeviceRadixSort::SortKeys(cub, cb, k0, k1, (int)n, 0, 3 * b, s));
    if (rc) return rc;
    return linr_hip_rc(hipcub::DeviceSelect::Unique(cub, cb, k1, k0, num, (int)n, s));
}
template <typename K>
int su_unique_coords(const int32_t* coords, int64_t n, const int32_t* origin, int shift, int b, char* base, size_t kb, int32_t* out,
                     int64_t* count, hipStream_t s) {
    K* k0 = (K*)base;
    K* k1 = (K*)(base + kb);
    int* num = (int*)(base + 3 * kb);
    int rc = su_sort_unique<K>(coords, n, origin, shift, b, k0, k1, num, base + 3 * kb + 256, su_cub_bytes(n), s);
    if (rc) return rc;
    su_decode_k<K><<<linr_grid(n, LINR_BLOCK), LINR_BLOCK, 0, s>>>(k0, num, n, b, out, count);
    return linr_launch_rc();
}
template <typename KC, typename KP>
int su_level(const int32_t* child, int64_t m, int b, char* base, size_t kb, int32_t* parent, float* occ, int64_t* count, hipStream_t s) {
    KP* k0 = (KP*)base;
    KP* k1 = (KP*)(base + kb);
    KC* ck = (KC*)(base + 2 * kb);
    int* num = (int*)(base + 3 * kb);
    su_keys_k<KC><<<linr_grid(m, LINR_BLOCK), LINR_BLOCK, 0, s>>>(child, m, nullptr, 0, b, ck);
    int rc = su_sort_unique<KP>(child, m, nullptr, 1, b - 1, k0, k1, num, base + 3 * kb + 256, su_cub_bytes(m), s);
    if (rc) return rc;
    su_decode_k<KP><<<linr_grid(m, LINR_BLOCK), LINR_BLOCK, 0, s>>>(k0, num, m, b - 1, parent, count);
    su_occ_k<KC, KP><<<linr_grid(4 * m, LINR_BLOCK), LINR_BLOCK, 0, s>>>(ck, m, k0, num, b, occ);
    return linr_launch_rc();
}
}  // namespace

extern "C" size_t linr_sort_unique_workspace_bytes(int64_t n) {
    if (n < 0) n = 0;
    return 3 * up256((size_t)n * 8) + 256 + up256(su_cub_bytes(n));
}

// coords: int32 [n,3], every (coordinate - origin) in [0, 2^coord_bits), coord_bits <= 20, any order, duplicates allowed; origin:
// device int32 [3] subtracted from every row first (the frame's coord_data_min, custom_dataset.py:276-279) or nullptr.  out: int32 [n,3]
// (room for n rows); *count (device int64) = number of distinct rows of (coords >> shift), written to out in x-major order.
extern "C" int linr_coords_sort_unique(const int32_t* coords, int64_t n, const int32_t* origin, int32_t shift, int32_t coord_bits, int32_t* out,
                                       int64_t* count, void* ws, size_t ws_bytes, void* stream) {
    if (n < 0 || shift < 0 || shift > 19 || coord_bits < 1 || coord_bits > 20 || n > INT32_MAX) return LINR_EINVAL;
    if (!count) return LINR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return linr_hip_rc(hipMemsetAsync(count, 0, sizeof(int64_t), s));
    if (!coords || !out || !ws) return LINR_EINVAL;
    if (ws_bytes < linr_sort_unique_workspace_bytes(n)) return LINR_ENOSPC;
    if (((uintptr_t)ws) & 255u) return LINR_EALIGN;
    const int b = coord_bits - shift > 1 ? coord_bits - shift : 1;
    const size_t kb = up256((size_t)n * 8);
    if (3 * b <= 32) return su_unique_coords<uint32_t>(coords, n, origin, shift, b, (char*)ws, kb, out, count, s);
    return su_unique_coords<uint64_t>(coords, n, origin, shift, b, (char*)ws, kb, out, count, s);
}

// One octree level (octree_level.forward, models/module_utils.py:86-110) as one call: child int32 [m,3] sorted x-major and unique,
// coordinates in [0, 2^coord_bits); parent [m,3] / occ [m,8] have room for m rows; *count (device int64) = the number of parents.
extern "C" int linr_octree_level(const int32_t* child, int64_t m, int32_t coord_bits, int32_t* parent, float* occ, int64_t* count, void* ws,
                                 size_t ws_bytes, void* stream) {
    if (m < 0 || coord_bits < 1 || coord_bits > 20 || m > INT32_MAX) return LINR_EINVAL;
    if (!count) return LINR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) return linr_hip_rc(hipMemsetAsync(count, 0, sizeof(int64_t), s));
    if (!child || !parent || !occ || !ws) return LINR_EINVAL;
    if (ws_bytes < linr_sort_unique_workspace_bytes(m)) return LINR_ENOSPC;
    if (((uintptr_t)ws) & 255u) return LINR_EALIGN;
    const int b = coord_bits > 1 ? coord_bits : 2;
    const size_t kb = up256((size_t)m * 8);
    if (3 * b <= 32) return su_level<uint32_t, uint32_t>(child, m, b, (char*)ws, kb, parent, occ, count, s);
    if (3 * (b - 1) <= 32) return su_level<uint64_t, uint32_t>(child, m, b, (char*)ws, kb, parent, occ, count, s);
    return su_level<uint64_t, uint64_t>(child, m, b, (char*)ws, kb, parent, occ, count, s);
}

// Per-axis minimum and maximum of a coordinate list: out[0..2] = min, out[3..5] = max (device int32 [6]); what custom_dataset.py:
// 276-279 computes with tensor reductions (torch's int64 column reductions cost 0.32 ms each on a 784 k-point frame).
namespace {
__global__ __launch_bounds__(LINR_BLOCK) void minmax_init_k(int32_t* out) {
    if (threadIdx.x < 3) out[threadIdx.x] = INT32_MAX;
    else if (threadIdx.x < 6) out[threadIdx.x] = INT32_MIN;
}
// The flat int32 stream read coalesced: with a grid whose thread count is a multiple of 3 every thread stays on one axis.  Per block
// one LDS reduction, then 6 global atomics (integer min / max: the order of the atomics does not matter).
__global__ __launch_bounds__(LINR_BLOCK) void minmax_k(const int32_t* __restrict__ c, int64_t n3, int32_t* __restrict__ out) {
    __shared__ int s_lo[3], s_hi[3];
    if (threadIdx.x < 3) { s_lo[threadIdx.x] = INT32_MAX; s_hi[threadIdx.x] = INT32_MIN; }
    __syncthreads();
    const int64_t t0 = (int64_t)blockIdx.x * LINR_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * LINR_BLOCK;      // stride % 3 == 0
    int lo = INT32_MAX, hi = INT32_MIN;
    for (int64_t i = t0; i < n3; i += stride) { const int v = c[i]; lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
    const int a = (int)(t0 % 3);
    if (lo <= hi) { atomicMin(&s_lo[a], lo); atomicMax(&s_hi[a], hi); }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(out + threadIdx.x, s_lo[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(out + threadIdx.x, s_hi[threadIdx.x - 3]);
}
}  // namespace

extern "C" int linr_coords_minmax(const int32_t* coords, int64_t n, int32_t* out, void* stream) {
    if (n < 1 || !coords || !out) return LINR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    minmax_init_k<<<1, LINR_BLOCK, 0, s>>>(out);
    int64_t blocks = (3 * n + LINR_BLOCK * 16 - 1) / (LINR_BLOCK * 16);
    blocks = (blocks < 768 ? blocks : 768);
    blocks = (blocks + 2) / 3 * 3;          // thread count a multiple of 3: one axis per thread
    minmax_k<<<(unsigned)blocks, LINR_BLOCK, 0, s>>>(coords, 3 * n, out);
    return linr_launch_rc();
}
