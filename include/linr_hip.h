/* linr_hip.h - C-ABI of the MI355X (gfx950) coding-network engine for LINR-PCGC.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference (100 % Python) reaches its
 * native code through MinkowskiEngine 0.5.4 and torchac 0.9.3 wheels; each entry point below names the
 * reference call site(s) it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _h (host); the caller (PyTorch's caching
 *     allocator) owns all memory; nothing is allocated, freed or retained across calls.  The library keeps no mutable
 *     global state on the data path: calls on different streams may run from different host threads (the GOP decoder
 *     does).  The two optional process-wide aids - the live kernel timing of linr_prof_* (mutex-guarded) and the
 *     on-chip poison test hook of linr_debug_poison (an atomic mask) - are off by default.
 *   - `stream` is a hipStream_t passed as void*; all work is stream-ordered, no host synchronisation.
 *   - return value: 0 on success, >0 = hipError_t, <0 = argument error (LINR_E*).  No exceptions cross.
 *   - feature matrices are row-major float32 [rows, ld] with an explicit leading dimension `*_ld` so that a
 *     channel slice (ME.cat / merge_two_frames) is a pointer offset, not a copy.
 *   - the kernel map is int32 nbr[27][ld]: nbr[k*ld + j] = row of coord[j] + delta_k or -1, with
 *     k = (dx+1) + 3*(dy+1) + 9*(dz+1)  (MinkowskiEngine hypercube region, first axis fastest).
 */
#ifndef LINR_HIP_H
#define LINR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LINR_ABI_VERSION 27
#define LINR_API __attribute__((visibility("default")))

#define LINR_EINVAL   (-1)   /* bad argument (null pointer, negative size, unsupported channel count) */
#define LINR_ENOSPC   (-2)   /* workspace / arena / output buffer too small */
#define LINR_EALIGN   (-3)   /* pointer or leading dimension violates the documented alignment */

/* epilogue / mode flags */
#define LINR_RELU      1u    /* out = max(out, 0)                                   (MinkowskiReLU, nn.ReLU) */
#define LINR_ACCUM     2u    /* out += result instead of out = result               (gradient fan-in)        */
#define LINR_RELU_MASK 4u    /* result *= (act > 0): backward of a ReLU whose OUTPUT is `act`                */
#define LINR_NO_BIAS   8u
#define LINR_PAD_ROW  16u    /* the gathered operand has a readable all-zero row at index -1 (in - in_ld):
                                absent neighbours are read from it instead of being branched around      */
#define LINR_MUL_BF16 16u    /* the wide 3x3x3 convolutions only (linr_spconv_wide, linr_spconv_wgrad_wide, _wide2;
                                they take no LINR_PAD_ROW): the PRODUCTS on bf16 matrix instructions - operands rounded to
                                bf16 (nearest even) at the multiply, fp32 sums; memory and everything else stay fp32    */

LINR_API int linr_abi_version(void);
/* number of float parameters of LINR_PCGC_Model(scale_num, hidden=8, block_layers, outstage=8, instage=1)
 * in parameters() order (models/model_core.py:31-35, models/upsample.py:43-76; block_layers = main.py:521, the
 * Inception layers of block_in's ResNetBlock, 1..4 - the outter blocks always have one, upsample.py:72-76).
 * 54,712 for scale_num = 7, block_layers = 1.  This count and the whole-network entry points (linr_net_*) are the
 * hidden_channel_conv = 8 model (main.py:520 default): their kernels are specialised for 8-wide rows.  Widths 16 / 32 run on
 * the channel-blocked executor: the op-level entries below on 8-wide channel blocks.  Its inference forward and its decoder scales
 * are C entries, too (linr_param_count_wide, linr_net_forward_wide[_bf16], linr_decode_scale[_batch]_wide), and so is its training
 * step (linr_net_train_step_wide and its split entries): the host mirror (linr_pcgc_amd/wide_net.py) is their cross-check. */
LINR_API int64_t linr_param_count(int32_t scale_num, int32_t block_layers);

/* ---- kernel map -------------------------------------------------------------------------------------------
 * Replaces MinkowskiEngine's CoordinateManager insert + kernel-map generation that every ME.SparseTensor /
 * MinkowskiConvolution call triggers (models/function_utils.py:13-18,58-69,92-93; models/upsample.py:20-23,
 * 90-97; models/resnet.py:15-51).  coords: int32 [n,3], unique, sorted by the x-major ravel key (the order
 * qscTensor guarantees, models/module_utils.py:246-256), each coordinate in [0, 2^20).
 * Writes nbr[k*ld + row_base + j] = row_base + (index of neighbour) or -1 for j < n.
 * ws: at least linr_kmap_workspace_bytes(n) bytes, 8-byte aligned. */
LINR_API size_t linr_kmap_workspace_bytes(int64_t n);
LINR_API int linr_kmap_build(const int32_t* coords, int64_t n, int32_t* nbr, int64_t ld, int64_t row_base,
                    void* ws, size_t ws_bytes, void* stream);
/* The same map for the lists of n_seg frames, back to back, with ONE key launch and ONE search launch (the lock-step GOP decoder,
 * linr_decode_scale_batch): coords int32 [N,3] = n_seg sorted unique x-major lists; seg_off_h (HOST) [n_seg + 1] rises from 0 to N
 * (empty segments allowed), 1 <= n_seg <= LINR_DECODE_MAX_FRAMES.  A row looks its neighbours up inside its own segment only, so two
 * frames with equal or adjacent coordinates never see each other; entries are global rows or -1, bitwise what n_seg calls of
 * linr_kmap_build with row_base = seg_off_h[f] write.  ws: linr_kmap_workspace_bytes(N) bytes, 8-byte aligned. */
#define LINR_DECODE_MAX_FRAMES 64
LINR_API int linr_kmap_build_segments(const int32_t* coords, const int64_t* seg_off_h, int32_t n_seg, int32_t* nbr, int64_t ld,
                             void* ws, size_t ws_bytes, void* stream);
/* Compressed form of the same map for x-major sorted coordinates: the dz = -1,0,+1 neighbours of a (dx,dy) column are
 * consecutive rows, so lo[q*ld + j] = row of the first present neighbour of column q = (dx+1)+3(dy+1) and bit
 * q*3 + (dz+1) of mask[j] says which are present: 40 B/row instead of 108.  Rows of nbr must hold global row ids. */
LINR_API int linr_kmap_compress(const int32_t* nbr, int64_t nbr_ld, int64_t n, int32_t* lo, uint32_t* mask, int64_t ld,
                       void* stream);
/* The 7-neighbour occupancy features of the scale context (qscTensor.set_offset_tensor, models/module_utils.py:201-224,
 * offsets of glob_params.py:3) read off the kernel map: out[j*7 + i] = 1.0f if neighbour i of voxel row_base + j exists.
 * Replaces 7 QuickSearchCoord.search calls per scale in decoder.decode_one_frame (decoder.py:160-166). */
LINR_API int linr_kmap_offset_feat(const int32_t* nbr, int64_t ld, int64_t row_base, int64_t n, float* out, void* stream);
/* Child occupancy of an octree level (octree_level.forward, models/module_utils.py:86-110; the 8 x [N,1] `occ_lst` of
 * datautils/custom_dataset.py:201-206): child [m,3] int32 sorted x-major and unique, parent [n,3] = the sorted unique
 * floor(child / 2); writes occ[j*8 + 4dx+2dy+dz] = 1.0f iff child 2*parent[j]+(dx,dy,dz) exists.  Same sorted-key binary
 * search as the kernel map; ws: linr_kmap_workspace_bytes(m) bytes, 8-byte aligned. */
LINR_API int linr_octree_occupancy(const int32_t* child, int64_t m, const int32_t* parent, int64_t n, float* occ, void* ws,
                          size_t ws_bytes, void* stream);
/* Sorted unique coordinate list, optionally of the parents: the torch.unique(dim=0) of datautils/custom_dataset.py:271-282 (the
 * input cloud: shift 0) and of octree_level.forward (models/module_utils.py:92,103: parent = unique(floor(child / 2)): shift 1) as one
 * call - compact x-major keys of ((coords - origin) >> shift), radix sort over 3 (coord_bits - shift) bits, unique, decode.  coords:
 * int32 [n,3] with (coords - origin) in [0, 2^coord_bits), coord_bits <= 20, any order, duplicates allowed; origin: DEVICE int32 [3]
 * or NULL (zero); out: int32 [n,3] (room for n rows); *count: DEVICE int64 =
 * number of distinct rows written.  ws: at least linr_sort_unique_workspace_bytes(n) bytes, 256-byte aligned. */
LINR_API size_t linr_sort_unique_workspace_bytes(int64_t n);
LINR_API int linr_coords_sort_unique(const int32_t* coords, int64_t n, const int32_t* origin, int32_t shift, int32_t coord_bits, int32_t* out,
                                     int64_t* count, void* ws, size_t ws_bytes, void* stream);
/* Per-axis minimum / maximum of a coordinate list (the coord_data_min of custom_dataset.py:276-279 and the span that fixes the
 * octree depth): coords int32 [n,3], n >= 1; out: DEVICE int32 [6] = min x, y, z, max x, y, z. */
LINR_API int linr_coords_minmax(const int32_t* coords, int64_t n, int32_t* out, void* stream);
/* One octree level as one call (octree_level.forward, models/module_utils.py:86-110: parents AND their child occupancy; the dataset
 * calls it once per scale, datautils/custom_dataset.py:289-344): child int32 [m,3] sorted x-major and unique, coordinates in
 * [0, 2^coord_bits); parent [m,3] and occ [m,8] have room for m rows, *count (DEVICE int64) = the number of parents written.
 * ws: linr_sort_unique_workspace_bytes(m) bytes, 256-byte aligned. */
LINR_API int linr_octree_level(const int32_t* child, int64_t m, int32_t coord_bits, int32_t* parent, float* occ, int64_t* count, void* ws,
                               size_t ws_bytes, void* stream);
/* ALL octree levels of a frame as one call, without a sort (csrc/octree.hip; the loop of datautils/custom_dataset.py:289-344 over
 * octree_level.forward, models/module_utils.py:86-110): the parents of a sorted unique child list are the set bits of a bitmap over
 * their compact x-major keys, read in word order.  child: int32 [m,3] sorted x-major and unique, coordinates in [0, 2^coord_bits),
 * 2 <= coord_bits <= 20 (not validated: rows that break this give meaningless output, but no kernel writes outside its buffers);
 * m_dev: NULL, or a DEVICE int64 holding the live row
 * count (<= m: the count linr_coords_sort_unique left on the device - no host read between the two calls).  Level l = 0 ..
 * linr_octree_levels_count(coord_bits, max_levels) - 1 has child coordinates of coord_bits - l bits; its parents (int32 rows) and their
 * child occupancy (float32 [.,8], column 4 dx + 2 dy + dz) are written BACK TO BACK into parents / occ, level after level, each
 * buffer with room for linr_octree_levels_rows(m, coord_bits, max_levels) rows; counts: DEVICE int64 [levels] = rows of every level
 * (the caller reads them once, behind the call, and slices).  Bit-identical to linr_octree_level applied level by level.
 * Two kinds of level, planned from (m, coord_bits) alone, level by level: a DENSE level is the bitmap above - 2^(3 pb) bits, pb = the
 * bits of the parents' coordinates - and is taken for pb <= 10 while the bitmap has at most 12 32-bit words per possible row (or at
 * most 2^19 words); every other level is SPARSE: head-of-parent flags over the sorted child rows, one scan, the rank of every parent
 * from lower bounds in the child keys - work and workspace follow the rows, whatever the depth.
 * ws: linr_octree_levels_workspace_bytes(m, coord_bits, max_levels) bytes, 256-byte aligned: at most 24 (m + 1) bytes (two key lists
 * of 8 bytes per row, flags and scan of 4 each) + for the dense levels 4 bytes per word of every bitmap and 8 per word of the largest
 * (its counts and scan) + 1 MB (the scan's own scratch, alignment). */
LINR_API int32_t linr_octree_levels_count(int32_t coord_bits, int32_t max_levels);
LINR_API int64_t linr_octree_levels_rows(int64_t m, int32_t coord_bits, int32_t max_levels);
LINR_API size_t linr_octree_levels_workspace_bytes(int64_t m, int32_t coord_bits, int32_t max_levels);
LINR_API int linr_octree_levels(const int32_t* child, int64_t m, const int64_t* m_dev, int32_t coord_bits, int32_t max_levels,
                                int32_t* parents, float* occ, int64_t* counts, void* ws, size_t ws_bytes, void* stream);
/* sets *bad (device int32, pre-zeroed by the caller) to non-zero if coords are not sorted/unique/in range */
LINR_API int linr_kmap_validate(const int32_t* coords, int64_t n, int32_t* bad, void* stream);

/* ---- sparse 3x3x3 convolution on a fixed coordinate set ------------------------------------------------------
 * Replaces ME.MinkowskiConvolution(kernel_size=3, stride=1, bias=True).forward and its autograd backward
 * (call sites: models/upsample.py:17-23,90-97,153,171,210; models/resnet.py:15-51,56-57).
 * W: [27][cin][cout] (the ME `.kernel` tensor), bias: [cout] (`.bias` is [1,cout]).
 * fwd:        out[j, :cout] = bias + sum_k in[nbr[k][j], :cin] @ W[k]  (+ res[j, :cout]) (ReLU)
 * bwd_data:   gin[i, :cin] (+)= sum_k gout[nbr[26-k][i], :cout] @ W[k]^T   (* (act[i] > 0))
 * bwd_weight: gW[k] (+)= sum_j in[nbr[k][j]]^T gout[j] ; gb (+)= sum_j gout[j]   (deterministic two-pass)
 * cin in 1..8, cout in {4, 8}.  `res`/`act` may be NULL when their flag is absent. */
LINR_API int linr_spconv_fwd(const float* in, int32_t in_ld, const int32_t* nbr, int64_t nbr_ld, int64_t n,
                    const float* W, const float* bias, int32_t cin, int32_t cout,
                    const float* res, int32_t res_ld, float* out, int32_t out_ld, uint32_t flags, void* stream);
LINR_API int linr_spconv_bwd_data(const float* gout, int32_t gout_ld, const int32_t* nbr, int64_t nbr_ld, int64_t n,
                         const float* W, int32_t cin, int32_t cout,
                         const float* act, int32_t act_ld, float* gin, int32_t gin_ld, uint32_t flags,
                         void* stream);
LINR_API size_t linr_spconv_bwd_weight_workspace_bytes(int64_t n, int32_t cin, int32_t cout);
LINR_API int linr_spconv_bwd_weight(const float* in, int32_t in_ld, const float* gout, int32_t gout_ld,
                           const int32_t* nbr, int64_t nbr_ld, int64_t n, int32_t cin, int32_t cout,
                           float* gW, float* gb, uint32_t flags, void* ws, size_t ws_bytes, void* stream);

/* The same convolution on the COMPRESSED kernel map (linr_kmap_compress) and the matrix cores
 * (v_mfma_f32_4x4x1_16b_f32 with broadcast weights: 64 rows x 4 output channels x 1 input channel per instruction, no
 * padding; K = 1 keeps every product a single-rounding fmaf in the order of the conv family (the three dz taps of a (dx,dy)
 * column back to back, column by column inside an x-slab - LINR_TAP in csrc/common.h; channel ascending), so results are
 * bit-identical to linr_spconv_fwd / _bwd_data).  This is what the network executor launches.  Requirements: `in`
 * 16-byte aligned with in_ld in {4, 8} and a zero row at index -1 (LINR_PAD_ROW contract), cout (fwd) / cin (bwd) in {4, 8}.
 * bwd != 0 selects backward-data with `in` = output gradient, `out` = input gradient. */
LINR_API int linr_spconv_cmap(int32_t bwd, const float* in, int32_t in_ld, const int32_t* lo, const uint32_t* mask,
                     int64_t ld, int64_t n, const float* W, const float* bias, int32_t cin, int32_t cout,
                     const float* res, int32_t res_ld, const float* act, int32_t act_ld, float* out, int32_t out_ld,
                     uint32_t flags, void* stream);
/* The same convolution for channel-BLOCKED activations wider than 8 (--hidden_channel_conv 16 / 32, main.py:520; models/upsample.py:
 * 38-76, models/resnet.py:12-51): a C-wide matrix is C / 8 blocks [rows][8], each with its zero row in front.  ONE gather of all
 * input blocks per tap feeds every output channel (csrc/wide.hip).  in_h / out_h / res_h / act_h: HOST arrays of device pointers to
 * the blocks.  fwd: gathers ceil(cin / 8) blocks (cin < 8: channels >= cin of the one block are ignored), produces cout / 8 blocks;
 * bwd: gathers the output gradient's cout / 8 blocks at the mirrored taps, produces cin / 8 blocks.  cin, cout <= 32 (8, 16, 32;
 * cin < 8 forward only).  W [27][cin][cout], bias [cout] or NULL; flags: LINR_RELU, LINR_ACCUM, LINR_RELU_MASK, LINR_MUL_BF16.
 * LINR_MUL_BF16 (csrc/wide_mul.hip; training option 'bf16-mul'): out = bias + sum rb(x) rb(W), backward-data gx = sum rb(g) rb(W), rb =
 * round to nearest even to bf16 of the fp32 value in memory, products exact, sums fp32; bias, residual, LINR_ACCUM, masks, ReLU and the
 * pointwise side path `pw` are computed in fp32 on the unrounded values, as without the flag.
 * pw (NULL or mode 0: none): a pointwise layer of the wide Inception layer (models/resnet.py:55-60) fused into the epilogue - pw->mode:
 *   1 forward conv0_0 (C -> h = C / 2): out2 = relu(in @ W10 + b10) of the row itself (conv1_0)
 *   2 forward conv1_1 (h -> h): out2 = (the produced row) @ W12 + b12 + aux (conv1_2 and the residual's upper half)
 *   3 backward of the block's tail convolution (C <- C): out2 = ((produced upper half) @ W12^T) * (aux > 0), aux = M
 *   4 backward of conv0_0 (C <- h): produced += aux @ W10^T in front of the ReLU mask, aux = the gradient of H1
 * W [cin_pw][cout_pw] (ME layout), b or NULL; aux_h / out2_h: HOST arrays of h / 8 block pointers; C in {16, 32}.  The fmaf chains are
 * those of linr_linear_wide: the fused and the two-launch forms give the same bits. */
typedef struct {
    int32_t mode;
    const float* W;
    const float* b;
    const float* const* aux_h;
    float* const* out2_h;
} linr_wide_pw;
LINR_API int linr_spconv_wide(int32_t bwd, const float* const* in_h, const int32_t* lo, const uint32_t* mask, int64_t ld, int64_t n,
                              const float* W, const float* bias, int32_t cin, int32_t cout, const float* const* res_h,
                              const float* const* act_h, float* const* out_h, uint32_t flags, const linr_wide_pw* pw, void* stream);
/* Weight gradient of that convolution: gW [27][cin][cout], gb [cout] (may be NULL) from the ceil(cin / 8) input blocks in_h (zero row in
 * front) and the cout / 8 output-gradient blocks g_h: one launch whose groups are the input blocks - the gathered, LDS-transposed rows
 * of a block multiply the tiles of ALL gradient blocks (cout 8 / 16 / 32 with the tiled table; else block pair by block pair) - into
 * `slab` (linr_spconv_wgrad_wide_slab_bytes(cin, cout) bytes), then ONE fixed-order reduction into the dense tensors.
 * nbr / tile8t: the frame's kernel map [27][ld] and its tiled copy (linr_kmap_tile8t).
 * flags: 0, or LINR_MUL_BF16, the only flag: gW = sum over rows of rb(x) rb(g) on bf16 matrix instructions with fp32 sums, gb = sum g
 * on the unrounded gradient; the same slab layout and reduction.  It needs the one-launch form (the tiled table, 16-byte aligned, cout
 * in {8, 16, 32}): LINR_EINVAL otherwise, and for any other bit. */
LINR_API size_t linr_spconv_wgrad_wide_slab_bytes(int32_t cin, int32_t cout);
LINR_API int linr_spconv_wgrad_wide(const float* const* in_h, int32_t cin, const float* const* g_h, int32_t cout, const int32_t* nbr,
                                    const int32_t* tile8t, int64_t ld, int64_t n, float* slab, float* gW, float* gb, uint32_t flags,
                                    void* stream);

/* Pointwise layers of the wide network on blocked activations (MinkowskiConvolution kernel_size 1: models/resnet.py:25-46 conv1_0,
 * conv1_2; the head's nn.Linear(C, 24): models/upsample.py:73-76) as ONE launch: out = [ReLU]([mask]((bias + in @ W) + res + old)).
 * in_h / out_h / res_h / act_h: HOST arrays of device pointers - blocked (channels / 8 matrices [n][8]) or, with *_blocked = 0, ONE
 * dense [n][channels] matrix (the head's 24 hidden units); res / act are laid out like out.  Weight element (ci, co) at
 * W[ci * ws_ci + co * ws_co] of a DENSE matrix: (ws_ci, ws_co) = (cout, 1) (ME layout) or (1, cin) (torch layout), nothing else;
 * backward-data = the same call with the roles of cin / cout and the two strides swapped (as linr_linear_bwd_data).  Shapes: blocked -> blocked with cin, cout in {8, 16, 32}; blocked (16, 32)
 * -> dense 24 and dense 24 -> blocked (16, 32).  flags: LINR_RELU, LINR_ACCUM, LINR_RELU_MASK, LINR_NO_BIAS. */
LINR_API int linr_linear_wide(const float* const* in_h, int32_t cin, int32_t in_blocked, const float* W, int32_t ws_ci, int32_t ws_co,
                              const float* bias, int32_t cout, int32_t out_blocked, const float* const* res_h, const float* const* act_h,
                              float* const* out_h, int64_t n, uint32_t flags, void* stream);
/* Their weight gradient: gW(ci, co) = sum_r x[r][ci] g[r][co] written at gW[ci * ws_ci + co * ws_co], gb[co] = sum_r g[r][co] (NULL:
 * skipped); LINR_ACCUM adds to the destinations.  All (input piece, gradient piece) pairs in one grouped launch + one fixed-order
 * reduction; ws: linr_linear_wgrad_wide_workspace_bytes(n, cin, cout) bytes.  Dense sides: up to 31 channels. */
LINR_API size_t linr_linear_wgrad_wide_workspace_bytes(int64_t n, int32_t cin, int32_t cout);
LINR_API int linr_linear_wgrad_wide(const float* const* in_h, int32_t cin, int32_t in_blocked, const float* const* g_h, int32_t cout,
                                    int32_t g_blocked, int64_t n, float* gW, int32_t ws_ci, int32_t ws_co, float* gb, uint32_t flags,
                                    void* ws, size_t ws_bytes, void* stream);

/* Deferred reductions: with gW = NULL linr_spconv_wgrad_wide / linr_linear_wgrad_wide only write their per-block partials (slab / ws stay
 * in use); linr_wide_reduce_many then sums up to any number of them, 32 per launch, in the same fixed order as the entries' own
 * reductions.  kind 0: a convolution (nblocks = linr_spconv_wgrad_wide_blocks(cout, tiled table given), gW [27][cin][cout], gb [cout] or
 * NULL; ws_ci > 0: the slab's row stride in floats when several convolutions share the rows); kind 1: a pointwise layer (nblocks = linr_linear_wgrad_wide_blocks(n), gW at the strides ws_ci / ws_co, gb or NULL). */
typedef struct {
    int32_t kind, nblocks, cin, cout, ws_ci, ws_co;
    const float* slab;
    float* gW;
    float* gb;
} linr_wide_reduce;
LINR_API int32_t linr_spconv_wgrad_wide_blocks(int32_t cout, int32_t tiled);
/* The weight gradients of TWO convolutions of the same shape h -> h (h in {8, 16}: conv0_1 and conv1_1 of a wide Inception layer) as one
 * launch - partials only: a slab row (2 (h / 8)^2 x 1736 floats; 256 rows) holds A's block pairs, then B's; reduce each with
 * linr_wide_reduce_many: kind 0, slab = the start of its part, nblocks 256, ws_ci = the row stride in floats.
 * flags: 0 or LINR_MUL_BF16 as in linr_spconv_wgrad_wide, any other bit LINR_EINVAL. */
LINR_API int linr_spconv_wgrad_wide2(const float* const* inA_h, const float* const* gA_h, const float* const* inB_h,
                                     const float* const* gB_h, int32_t h, const int32_t* tile8t, int64_t n, float* slab, uint32_t flags,
                                     void* stream);
LINR_API int32_t linr_linear_wgrad_wide_blocks(int64_t n);
LINR_API int linr_wide_reduce_many(const linr_wide_reduce* items_h, int32_t count, void* stream);

/* The occupancy head of the wide network behind the prune convolution (CNP.basic_module, models/upsample.py:137-161):
 * p = sigmoid(Linear(24, 1)(ReLU(Linear(C, 24)(c)))) and the stage's bits (model_core.py:72-81) in one launch.  c_h: HOST array of the
 * C / 8 blocks [n][8] (C = 16 / 32); w1 [24][C], b1 [24], w2 [24], b2 [1] (torch layouts); target: the occupancy column (stride
 * target_ld) or NULL; p [n]; bits_acc (double[1], += bits) or NULL; ws: linr_head_wide_workspace_bytes(n) bytes when bits are wanted. */
LINR_API size_t linr_head_wide_workspace_bytes(int64_t n);
/* (with bits_acc = NULL but target and ws given the stage's per-block partials stay in ws - linr_head_wide_workspace_bytes(n) / 8 doubles -
 * and linr_bits_finish adds the partials of any number of stages to bits_acc in one launch) */
LINR_API int linr_bits_finish(const double* partial, int64_t count, double* bits_acc, void* stream);
LINR_API int linr_head_wide_fwd(const float* const* c_h, int32_t C, const float* w1, const float* b1, const float* w2, const float* b2,
                                const float* target, int32_t target_ld, int64_t n, float* p, double* bits_acc, void* ws, size_t ws_bytes,
                                void* stream);
/* Backward of nstages (<= 8) such heads in ONE grouped launch: gc = d (gscale * bits) / d c per stage and the parameter gradients
 * grads[nstages][W1 (24 x C) | b1 (24) | w2 (24) | b2 (1)] (written, not accumulated; the inner_mlps of consecutive stages are
 * consecutive in the reference's parameter order).  c_h / gc_h: HOST arrays [nstages][C / 8] of block pointers (stage-major);
 * p_h / target_h / w1_h / b1_h / w2_h: [nstages].  slab: linr_head_wide_bwd_slab_bytes(C, nstages) bytes of scratch. */
LINR_API size_t linr_head_wide_bwd_slab_bytes(int32_t C, int32_t nstages);
LINR_API int linr_head_wide_bwd(const float* const* c_h, const float* const* p_h, const float* const* target_h, int32_t target_ld,
                                const float* const* w1_h, const float* const* b1_h, const float* const* w2_h, int32_t C, int32_t nstages,
                                float gscale, float* const* gc_h, int64_t n, float* slab, size_t slab_bytes, float* grads, void* stream);

/* Backward-weight of the same convolution as a stand-alone kernel (the executor uses it for the first convolutions of the outter
 * blocks, whose inputs need no gradient, and for the schedules without the fused backward below): lane = (offset, channel quad),
 * gathered quad x broadcast gradient tile on v_mfma_f32_4x4x1, row order fixed => reproducible.
 * Writes linr_spconv_wgrad_cmap_blocks() (= 512) per-block partials: slab[b][(27 cin + 1) cout], kernel gradient
 * [27][cin][cout] first, bias gradient [cout] last; their ascending sum over b is MinkowskiConvolution's kernel / bias
 * gradient (ME autograd of the call sites above).  `in`: [n][8] floats, 16-byte aligned, zero row at index -1.
 * tile8t: linr_kmap_tile8t's table or NULL.  With it the gathers are laid out like the convolutions' - lane = (tap of 4, row of
 * 8, quad): four 256-byte runs per instruction - into a wave-private LDS image that every (tap, quad) lane reads back
 * transposed (spconv_wgrad_t_k, the executor's choice); without it the indices come from nbr[27][ld] and every lane gathers its
 * own (tap, quad) (spconv_wgrad_mfma_k).  Same partial sums, bit for bit. */
LINR_API int64_t linr_spconv_wgrad_cmap_blocks(void);
LINR_API int linr_spconv_wgrad_cmap(const float* in, int32_t in_ld, const float* gout, int32_t gout_ld, const int32_t* nbr,
                           const int32_t* tile8t, int64_t ld, int64_t n, int32_t cin, int32_t cout, float* slab, void* stream);
/* Fixed-order sum over the rows of a [nblocks][elems] slab of per-block partials (the form linr_spconv_wgrad_cmap, _wgrad_dual44,
 * _bwd_fused, linr_occ_wgrad7 ... return): elements [0, split) to dstA, [split, elems) to dstB (either may be NULL);
 * LINR_ACCUM adds to the destination.  16 threads per element, slices added in order: bit-reproducible. */
LINR_API int linr_slab_reduce(const float* slab, int32_t nblocks, int32_t elems, int32_t split, float* dstA, float* dstB,
                     uint32_t flags, void* stream);
/* The tiled copy of the kernel map in the lane order of the transposing kernel: tile8t[g][t][u][j] = nbr[tap(4 j + t)][8 g + u]
 * (-1 for position 27, j = 7, beyond n), tap(p) = p / 9 + 3 * ((p / 3) % 3) + 9 * (p % 3): the conv family's slab-major tap
 * sequence, so that the four taps of one gather instruction are neighbours in memory.  tile8t: linr_kmap_tile8t_bytes(n) bytes,
 * 16-byte aligned. */
LINR_API size_t linr_kmap_tile8t_bytes(int64_t n);
LINR_API int linr_kmap_tile8t(const int32_t* nbr, int64_t ld, int64_t n, int32_t* tile8t, size_t tile8t_bytes, void* stream);
/* Backward of a convolution 8 -> 8 from ONE gather of the output gradient (csrc/fused_bwd.hip; what the executor launches for
 * the prune convolutions, the blocks' tail convolutions and block_in's first convolution, i.e. the autograd nodes of
 * upsample.py:20-23,88-97):  gin = backward-data of linr_spconv_cmap (bit-identical to it) and per-block partials of the
 * kernel / bias gradient, slab[b][27 * 64 + 8], b < nblocks (every row is written; their ascending sum over b is
 * MinkowskiConvolution's kernel / bias gradient).  gW[k] = sum_i in[i]^T gout[nbr(i, 26 - k)] - the rows backward-data gathers
 * anyway - is accumulated from a wave-private LDS image of the gathered rows.  gout: [n][8], 16-byte aligned, zero row at
 * index -1; in: [n][8] (the convolution's input); gin: [n][8], 16-byte aligned. */
LINR_API int linr_spconv_bwd_fused(const float* gout, const float* in, const int32_t* lo, const uint32_t* mask, int64_t ld,
                          int64_t n, const float* W, float* gin, float* slab, int32_t nblocks, void* stream);
/* Measurement aid for bench.py's roofline: while enabled, the launches of a training step inside linr_net_forward /
 * _backward / _train_step are bracketed by HIP event pairs on the stream they are launched on, by kernel class:
 *   0 fused backward 8->8 (conv_bwd_wgrad_k<0>)   1 conv 8->8 forward, plain epilogue   2 fused backward of the two 4->4 convs
 *   3 fused backward of conv0_0 8->4              4 prune conv + head forward           5 conv0_0 | conv1_0 forward
 *   6 both 4->4 convs forward                     7 shared occupancy conv               8 head backward
 *   9 first-conv / stand-alone weight gradients  10 pointwise weight gradients         11 scale context (forward, backward)
 *  12 sums, reduction, Adam                      13 stand-alone backward-data convolutions (schedules without the fused backward)
 * and of the bf16 training executor (linr_net_train_step_bf16; 14..16 are poison-only classes, see linr_debug_poison):
 *  17 fused backward 8->8 (bbwd_k<0>)            18 fused backward of the two 4->4 convs 19 fused backward of conv0_0 8->4
 *  20 forward convolutions (bconv_k)             21 head backward                       22 first-conv weight gradients
 *  23 scale context forward, sums, conversions, Adam
 * (the library's names for these numbers: enum ProfKind in csrc/prof.h)
 * linr_prof_mask selects the classes that are recorded (default: 0 and 1; an event pair costs a few microseconds of stream
 * time).  linr_prof_read waits for the recorded events and returns their summed elapsed time, the number of launches and the
 * number of row passes (a grouped launch over g layers counts g).  mode 1 = clear the records and start, 2 = resume,
 * 0 = stop (records are kept).  Mutex-guarded; 4096 launches in total. */
#define LINR_PROF_KINDS 24
LINR_API int linr_prof_mask(uint32_t mask);
/* Test hook (tests/test_gpu_parity.py::test_results_do_not_depend_on_leftover_onchip_state): every launch of
 * linr_net_forward / _backward / _train_step whose kernel class (the list above) has its bit set in kind_mask is preceded by a kernel that fills the LDS of every CU with 0xFFFFFFFF (a NaN
 * pattern) - results must not change: a kernel may not read on-chip state it did not write (on a GPU shared with another
 * process the leftovers are not one's own finite numbers). */
LINR_API int linr_debug_poison(uint32_t kind_mask);          /* bits 0..13: the classes above; 14: bf16 executor; 15: the decoder scales of csrc/decode.hip (linr_decode_scale, linr_decode_scale_batch, linr_children_segments) and linr_kmap_build_segments; 16: the entries of csrc/wide.hip.  The epoch kernels of linr_overfit_gop (csrc/overfit.hip) are in class 12 for every executor: no new class, the per-class launch counts of a single training step stay what they are */
LINR_API int linr_debug_poison_now(void* stream);           /* the same poisoning, once, on `stream` (in front of an op-level call) */
LINR_API int linr_prof_enable(int32_t mode);
LINR_API int linr_prof_read(int32_t kind, double* total_ms, int64_t* launches, int64_t* passes);

/* ---- pointwise layers ---------------------------------------------------------------------------------------
 * Replaces ME.MinkowskiConvolution(kernel_size=1) (models/resnet.py:31-37,45-51) and nn.Linear inside
 * PointwiseMLP (models/module_utils.py:42-81).  Element (ci,co) of the weight is W[ci*ws_ci + co*ws_co]:
 * ME kernel [cin][cout] -> (cout, 1); nn.Linear weight [cout][cin] -> (1, cin).
 * fwd: out = in @ W + bias (+res)(ReLU); bwd_data: gin (+)= gout @ W^T (*mask); bwd_weight: gW, gb. */
LINR_API int linr_linear_fwd(const float* in, int32_t in_ld, int64_t n, const float* W, int32_t ws_ci, int32_t ws_co,
                    const float* bias, int32_t cin, int32_t cout, const float* res, int32_t res_ld,
                    float* out, int32_t out_ld, uint32_t flags, void* stream);
LINR_API int linr_linear_bwd_data(const float* gout, int32_t gout_ld, int64_t n, const float* W, int32_t ws_ci,
                         int32_t ws_co, int32_t cin, int32_t cout, const float* act, int32_t act_ld,
                         float* gin, int32_t gin_ld, uint32_t flags, void* stream);
LINR_API size_t linr_linear_bwd_weight_workspace_bytes(int64_t n, int32_t cin, int32_t cout);
LINR_API int linr_linear_bwd_weight(const float* in, int32_t in_ld, const float* gout, int32_t gout_ld, int64_t n,
                           int32_t cin, int32_t cout, float* gW, int32_t ws_ci, int32_t ws_co, float* gb,
                           uint32_t flags, void* ws, size_t ws_bytes, void* stream);
/* dst[i] (+)= src[i] over n floats: the residual / gradient fan-in adds of the width-generic executor (linr_pcgc_amd/wide_net.py);
 * torch's `x + y` in models/resnet.py:59,161 and autograd's accumulation. */
LINR_API int linr_axpy(const float* src, int64_t n, float* dst, int32_t accumulate, void* stream);
/* dst (+)= src[0] + ... + src[count - 1] over n floats (count 1..8, n a multiple of 4, 16-byte aligned pointers; src_h: HOST array),
 * the sources added in list order: a gradient fan-in (e.g. x_glob's: upsample.py:206-214 under autograd) in one pass. */
LINR_API int linr_sum_many(const float* const* src_h, int32_t count, int64_t n, float* dst, int32_t accumulate, void* stream);

/* ---- occupancy head loss -------------------------------------------------------------------------------------
 * Replaces sigmoid + nn.BCELoss(reduction='sum') / ln 2 (models/upsample.py:160, models/model_core.py:14,76-81).
 * fwd: p[j] = sigmoid(z[j]); partial sums of -(t log p + (1-t) log(1-p))/ln2 (logs clamped at -100) are ADDED
 * into bits_acc (double[1], device) deterministically (fixed-order two-pass); t = target[j*target_ld].
 * bwd: gz[j] = gscale * d bits / d z[j] following torch's binary_cross_entropy_backward + sigmoid backward. */
LINR_API size_t linr_bce_workspace_bytes(int64_t n);
LINR_API int linr_bce_bits_fwd(const float* z, const float* target, int32_t target_ld, int64_t n, float* p,
                      double* bits_acc, void* ws, size_t ws_bytes, void* stream);
LINR_API int linr_bce_bits_bwd(const float* p, const float* target, int32_t target_ld, int64_t n, float gscale,
                      float* gz, void* stream);

/* ---- optimiser -----------------------------------------------------------------------------------------------
 * Replaces torch.optim.Adam(...).step() over 189 tensors (main.py:231-237,319) with one launch over the flat
 * parameter buffer.  step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t) are computed by the host in
 * double like torch does (hyper-parameters cross the ABI as double and are rounded to float once, like the
 * Python scalars torch passes to its kernels); L2 weight decay is folded into the gradient. */
LINR_API int linr_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                   double step_size, double bc2_sqrt, double beta1, double beta2, double eps, double weight_decay,
                   void* stream);

/* ---- whole-network executor ----------------------------------------------------------------------------------
 * One frame = all scales of one point cloud concatenated into a single row space (finest first); CNP weights are
 * shared by all scales, only the scale-context MLP differs (models/model_core.py:31-35).
 * Replaces LINR_PCGC_Model.logic_core/forward (models/model_core.py:38-81) + CNP.forward
 * (models/upsample.py:163-217) and the autograd backward that main.py:315-316 runs. */
#define LINR_FRAME_OCC_PADDED 1
typedef struct linr_frame {
    int64_t rows;                 /* total rows over all scales, < 2^27 - 1 (32-bit byte offsets of the gathers)  */
    int32_t n_scales;             /* scales present in this frame (<= model scale_num)                      */
    int32_t model_scale_num;      /* LINR_PCGC_Model scale_num (fixes the parameter layout)                 */
    int32_t block_layers;         /* Inception layers of block_in (main.py:521); 0 is read as 1              */
    int32_t flags;                /* 0, or LINR_FRAME_OCC_PADDED: `occ` is row 0 of a [rows + 1][8] buffer whose row -1 is all
                                   * zero - the executor then gathers the occupancy in place instead of keeping a padded
                                   * copy in its arena (one device copy per call less) */
    const int64_t* row_off_h;     /* HOST [n_scales+1] first row of each scale                              */
    const int32_t* scale_idx_h;   /* HOST [n_scales]  which scale embedding / scale MLP each scale uses     */
    const int32_t* nbr;           /* [27][nbr_ld] kernel map with global row ids                            */
    int64_t nbr_ld;               /* leading dimension of nbr (>= rows; a multiple of 4 enables 16-byte index loads) */
    const int32_t* nbr_lo;        /* [9][nbr_ld]  compressed kernel map (linr_kmap_compress): required by every network
                                   * entry (linr_net_*, fp32 and bf16), may be NULL for linr_sce_*, which do not read it */
    const uint32_t* nbr_mask;     /* [nbr_ld]     27-bit presence masks of the compressed map: required like nbr_lo  */
    const float*   offset_feat;   /* [rows][7]  7-neighbour occupancy (qscTensor.set_offset_tensor)         */
    const float*   occ;           /* [rows][8]  child occupancy ground truth (occ_lst concatenated)         */
    const int32_t* nbr8t;         /* linr_kmap_tile8t over nbr (the tiled copy in gather-lane order), or NULL             */
} linr_frame;

LINR_API size_t linr_net_arena_bytes(int64_t rows, int32_t block_layers);
/* stages [stage_begin, stage_end) of the 8-stage head; stage_begin == 0 also runs scale context + block_in.
 * The encoder calls (0, 8); the decoder calls (k, k+1) after writing decoded occupancy column k-1 into
 * frame->occ, which executes the identical launches => bitwise identical probabilities (models/upsample.py:249-295).
 * probs: [8][rows] (stage-major) or NULL.  bits_acc: double[1], accumulated into (caller zeroes). */
LINR_API int linr_net_forward(const linr_frame* f, const float* params, float* arena, size_t arena_bytes,
                     int32_t stage_begin, int32_t stage_end, float* probs, double* bits_acc, void* stream);
/* gradient of gscale * bits w.r.t. all parameters, ADDED into grads (flat, linr_param_count floats);
 * requires a preceding linr_net_forward(…, 0, 8, …) on the same arena. */
LINR_API int linr_net_backward(const linr_frame* f, const float* params, float* arena, size_t arena_bytes,
                      float gscale, float* grads, void* stream);

/* What one overfit iteration needs beyond frame, parameters, arena and stream: the argument of linr_net_train_step and
 * linr_net_train_step_bf16 (NULL in its place is LINR_EINVAL).  Device pointers unless marked HOST. */
typedef struct linr_step_args {
    float gscale;                   /* the loss is gscale * bits (main.py:314: 1 / point_num) */
    float* exp_avg;                 /* Adam's first moment, linr_param_count floats, updated */
    float* exp_avg_sq;              /* Adam's second moment, likewise */
    double lr;
    int64_t step;                   /* this update's 1-based count (>= 1) */
    const int64_t* scale_steps_h;   /* HOST [model_scale_num] update counts of the per-scale context MLPs INCLUDING this one, or NULL */
    double beta1, beta2, eps, weight_decay;     /* torch.optim.Adam's, L2 weight decay */
    double* bits_acc;               /* double[1], the step's bits are added into it (caller zeroes) */
    float* qparams;                 /* NULL: the plain step; else the quantisation-aware step evaluates the network at this fake-quantised
                                       image of params, which the call writes (linr_param_count floats, 16-byte aligned, not params) */
    int32_t bitdepth;               /* of the fake quantisation, 2..16; read only when qparams != NULL */
} linr_step_args;

/* One iteration of main.py:305-321 in a single call: forward (bits added into bits_acc), backward of
 * gscale * bits (gscale = 1/point_num), deterministic gradient reduction and the fused Adam update of `params`
 * (torch.optim.Adam with L2 weight decay; bias corrections computed in double).
 * args->scale_steps_h: HOST [model_scale_num] update counts of the per-scale context MLPs INCLUDING this update, or NULL.  With it the
 * update follows torch.optim.Adam (the reference pins torch 1.13.1, enviroment.yaml:30): an MLP whose count is 0 - no frame so far
 * contained its scale (custom_dataset.py:325), its .grad is still None - is skipped entirely; every other MLP is updated with
 * its own step count, with a zero gradient when this frame lacks the scale (optimizer.zero_grad() of main.py:320 leaves zero
 * tensors, so weight decay and moment decay keep acting).  A scale of this frame with count 0 is an error.  NULL updates every
 * parameter with `step`.  With args->qparams != NULL the forward and backward run at qparams = fake_quant(params) (see
 * linr_params_fake_quant below) while Adam - weight decay included - updates the fp32 master `params` with that gradient
 * (straight-through estimator): bits_acc receives the bits of the weights the codec would code with.  One launch more; the arena
 * layout is the same.  Every argument check comes before the first launch.  Nothing synchronises with the host. */
LINR_API int linr_net_train_step(const linr_frame* f, float* params, float* arena, size_t arena_bytes, const linr_step_args* args,
                        void* stream);

/* ---- quantisation-aware overfit (opt-in) --------------------------------------------------------------------------
 * The codec never codes geometry with the weights it trained: encode_one_gop quantises the flat parameter vector
 * (quant_uniform2, model_compression/model_size_est.py:72-91) and codes every frame with the DE-QUANTISED model
 * (encoder.py:101-103).  These entries, and linr_step_args.qparams of the training steps, let the overfit iteration
 * (main.py:305-321) see that step.
 *
 * linr_params_fake_quant: qparams = the de-quantised image of params, bit for bit what quant_uniform2 followed by the decoder's
 *   de-quantisation computes in fp32 on the CPU:  mn = min(params), mx = max(params), r = mx - mn, s = 2^bitdepth - 1,
 *   q = rint(((p - mn) / r) * s) (round half to even), qparams = (q / s) * r + mn, each of the six operations rounded to fp32 on
 *   its own.  params, qparams: device [n] floats, 16-byte aligned; codes: device [n] uint16 (8-byte aligned) that receive q, or
 *   NULL; minmax: two device floats that receive mn and mx, or NULL; bitdepth 2..16.  ONE launch, no host synchronisation.
 *   mx == mn: codes 0 and qparams = params (quant_uniform2 itself yields NaN there).  A NaN parameter takes no part in the minimum
 *   and maximum, stays NaN in qparams and has code 0; of a negative and a positive zero the negative one is the smaller.  Codes
 *   never leave [0, s].
 * linr_params_fake_quant_host: the same arithmetic as a plain loop over HOST pointers (no GPU needed).
 * linr_params_fake_quant_ranges: the same quantiser under K GIVEN ranges instead of the vector's own minimum and maximum (the
 *   encoder's range search, codec.encode_gop qrange_search=).  ranges_h: HOST [K][2] floats (lo, hi), lo <= hi, K in 1..16; they
 *   travel as a kernel argument, nothing is allocated.  For candidate k:  p' = p < lo ? lo : (p > hi ? hi : p)  (a NaN passes),
 *   then the arithmetic above with mn = lo, r = hi - lo (hi == lo: code 0 and p').  Outputs are rows of `stride` elements
 *   (stride >= n, a multiple of 4; the elements behind n are not touched): qparams device [K][stride] floats (16-byte aligned),
 *   codes device [K][stride] uint16 (8-byte aligned) or NULL, stats device int64 [K][4] (8-byte aligned) or NULL =
 *   {parameters below lo, parameters above hi, sum of the codes q, sum of |q - mu|} with mu = rint((float)sum_q / (float)n) as
 *   the model codec computes it: exact integers from which the host forms the codec's Laplace size estimate without reading a
 *   code back.  For (lo, hi) = (minimum, maximum) of params row k is bit for bit what linr_params_fake_quant writes.  ONE launch
 *   of K workgroups, no host synchronisation, no atomics; n == 0 launches nothing.  A bad K, stride, bound pair (lo > hi or NaN),
 *   pointer or alignment is refused before the launch.
 * linr_params_fake_quant_ranges_host: the same as a plain loop over HOST pointers (no GPU needed; no alignment asked). */
LINR_API int linr_params_fake_quant(const float* params, int64_t n, int32_t bitdepth, float* qparams, uint16_t* codes, float* minmax,
                                    void* stream);
LINR_API int linr_params_fake_quant_host(const float* params, int64_t n, int32_t bitdepth, float* qparams, uint16_t* codes,
                                         float* minmax);
LINR_API int linr_params_fake_quant_ranges(const float* params, int64_t n, int32_t bitdepth, const float* ranges_h, int32_t K,
                                           int64_t stride, float* qparams, uint16_t* codes, int64_t* stats, void* stream);
LINR_API int linr_params_fake_quant_ranges_host(const float* params, int64_t n, int32_t bitdepth, const float* ranges_h, int32_t K,
                                                int64_t stride, float* qparams, uint16_t* codes, int64_t* stats);

/* ---- bf16 / uint8-weight inference executor (BASELINE config[4]) ------------------------------------------------
 * The codec codes the geometry with the DE-QUANTISED model (encoder.py:101-103, decoder.py:87): w = q/255*(max-min)+min
 * for the uint8 codes q of quant_uniform2 (model_compression/model_size_est.py:72-91).  This entry takes the codes
 * themselves as the model (`codes`: device uint8 [linr_param_count], parameters() order; min_param / max_param: the two
 * floats of side_info.json) and de-quantises inside the kernels; features are bf16 (16-byte rows), every 3x3x3
 * convolution runs on v_mfma_f32_4x4x4_16b_bf16 with fp32 accumulation, biases / pointwise layers / MLPs stay fp32.
 * Inference only: same stage semantics as linr_net_forward (the encoder calls (0, 8), the decoder (k, k+1) after writing
 * occupancy column k-1 into frame->occ; both run identical per-row arithmetic => bit-identical probabilities).
 * probs: [8][rows] stage-major (required); bits_acc as in linr_net_forward.  Needs the compressed kernel map.
 * arena: linr_net_bf16_arena_bytes(rows, block_layers) bytes, 64-byte aligned; stages of one frame must share it.
 * Tolerance against the fp32 path on the same de-quantised weights (tests/test_gpu_bf16.py): logits |d| <= 5e-2,
 * bits within 1 %. */
LINR_API size_t linr_net_bf16_arena_bytes(int64_t rows, int32_t block_layers);
LINR_API int linr_net_forward_bf16(const linr_frame* f, const uint8_t* codes, float min_param, float max_param, void* arena,
                          size_t arena_bytes, int32_t stage_begin, int32_t stage_end, float* probs, double* bits_acc,
                          void* stream);

/* ---- bf16 / uint8-weight inference executor for hidden_channel_conv 16 / 32 (csrc/wide_bf16.hip) -------------------------------
 * BASELINE config[4]'s numerics (those of linr_net_forward_bf16) on the channel-blocked activations of the wide network: a C-wide matrix
 * is C / 8 bf16 blocks [1 + rows][8] (zero row in front), `*_bs` elements apart; the pointers passed are those of block 0's FIRST row.
 * The model is its uint8 codes (w = q / 255 * (max - min) + min in fp32); every 3x3x3 kernel is rounded to bf16 once, products are
 * accumulated in fp32; biases, conv1_0 / conv1_2, the scale context and head MLPs, sigmoid and the bits are fp32; every stored matrix
 * is bf16 and its consumers see the stored value; the prune convolution feeds the head MLP unrounded.  The schedule is Python
 * (WideNet.forward_bf16): the forward of models/model_core.py:38-81 / models/upsample.py:88-97,137-217 / models/resnet.py:12-60.
 *
 * linr_wide_bf16_prep (the de-quantisation of encoder.py:101-103's new_model, model_compression/model_size_est.py:72-91, inside the
 *   executor): pf [n_params] = the de-quantised fp32 parameters; img = the bf16 A-operand images of n_conv 3x3x3 convolutions.
 *   conv_tab (device, int64 [n_conv][4]): parameter offset of the kernel [27][cin][cout], cin, cout, offset of its image in img
 *   (8-byte elements, ascending; an image is linr_wide_bf16_image_elems(cin, cout) elements).  n_img: the total.  One launch.
 * linr_spconv_wide_bf16 (MinkowskiConvolution kernel_size 3, models/upsample.py:88-97, models/resnet.py:25-46): cin in 1..8 or 16 / 32,
 *   cout 8 / 16 / 32, one gather of every input block per tap.  epi 0: out = [ReLU](conv + bias + res) (then + res2: the extra skip
 *   rb(out + a) of models/resnet.py:160-161); epi 1 (conv0_0 + conv1_0): out blocks [0, cout / 8) = relu(conv), [cout / 8, cout / 4) =
 *   relu(in @ pw_w + pw_b) of the row itself (pw_w [cin][cout]); epi 2 (conv1_1 + conv1_2): out = rb(relu(conv)) @ pw_w + pw_b + res
 *   (pw_w [cout][cout], res = the Inception input's upper half) (then + res2).
 * linr_head_wide_bf16_fwd (CNP.basic_module, models/upsample.py:137-161): the prune convolution C -> C, then p = sigmoid(w2 . relu(w1 c +
 *   b1) + b2) (w1 [24][C]) on its fp32 output; with target (fp32 [rows][8], column t_col) the stage's per-256-row nats go to partial
 *   (linr_bits_finish sums them).
 * linr_sce_fwd_bf16 (models/model_core.py:48-53): x0 = the scale context, bf16 [1 + rows][8] (the pointer of the zero row, which is
 *   not written), on the parameters pf. */
LINR_API int64_t linr_wide_bf16_image_elems(int32_t cin, int32_t cout);
LINR_API int linr_wide_bf16_prep(const uint8_t* codes, int64_t n_params, float min_param, float max_param, const int64_t* conv_tab,
                                 int32_t n_conv, int64_t n_img, float* pf, void* img, void* stream);
LINR_API int linr_spconv_wide_bf16(int32_t epi, const uint16_t* in, int64_t in_bs, int32_t cin, const int32_t* lo, const uint32_t* mask,
                                   int64_t ld, int64_t n, const void* img, const float* bias, int32_t cout, const uint16_t* res, int64_t res_bs,
                                   const uint16_t* res2, int64_t res2_bs, const float* pw_w, const float* pw_b, int32_t relu, uint16_t* out,
                                   int64_t out_bs, void* stream);
LINR_API int linr_head_wide_bf16_fwd(const uint16_t* in, int64_t in_bs, int32_t C, const int32_t* lo, const uint32_t* mask, int64_t ld,
                                     int64_t n, const void* img, const float* bias, const float* w1, const float* b1, const float* w2,
                                     const float* b2, const float* target, int32_t t_col, float* p, double* partial, void* stream);
LINR_API int linr_sce_fwd_bf16(const float* pf, const linr_frame* f, uint16_t* x0_padded, void* stream);

/* ---- the inference forward of hidden_channel_conv 16 / 32 as one call (csrc/wide_fwd.hip) ---------------------------------------
 * LINR_PCGC_Model.logic_core / forward (models/model_core.py:38-81) + CNP.forward (models/upsample.py:163-217) at channels = 16 / 32:
 * the schedule of the host mirror (WideNet._forward with the pointwise layers fused; WideNet.forward_bf16) launch for launch through
 * the op-level entries above, with the arguments the mirror hands them - the probabilities and bits are the mirror's bit for bit.
 * linr_param_count_wide: the float parameters of LINR_PCGC_Model(scale_num, hidden, block_layers) in parameters() order (the scale
 *   context first, as at width 8; then block_in, the 8 inner_mlps Linear(hidden, 24) / Linear(24, 1), the 8 prune convolutions, the 7
 *   outter blocks); 0 for a hidden other than 16 / 32, a scale_num outside 1..16 or block_layers outside 1..4.
 * linr_net_wide_arena_bytes: the arena of one frame (any scale_num): per-role channel blocks that all blocks and stages reuse, the
 *   stages' bits partials and, for bf16 != 0, the de-quantised parameters, the prologue's convolution table and the weight images;
 *   0 for rows < 0 or over the row bound of linr_frame, and for a hidden / block_layers as above.
 * linr_net_forward_wide / _bf16: stages [stage_begin, stage_end) as linr_net_forward / linr_net_forward_bf16 run them.  stage_begin
 *   == 0 computes the scale context and block_in (bf16: the de-quantisation prologue first) and leaves x_glob (and the images) in the
 *   arena; stage_begin > 0 needs the preceding call on the same frame and arena to have done so, and reads the occupancy columns
 *   decoded so far from f->occ (LINR_FRAME_OCC_PADDED honoured; without it the fp32 forward gathers a padded copy it makes per call).
 *   probs [8][rows] stage-major or NULL; bits_acc double[1], accumulated into, or NULL.  arena: 64-byte aligned.  codes: the uint8
 *   codes of linr_param_count_wide parameters.  Checked in front of the first launch, in this order: a NULL f / params / codes /
 *   arena (LINR_EINVAL), the arena's alignment (LINR_EALIGN), hidden, the stage range (LINR_EINVAL), the arena's size (LINR_EINVAL
 *   where linr_net_wide_arena_bytes is 0, else LINR_ENOSPC), then the frame (linr_frame's structure, its matrices, nbr_ld).  rows
 *   == 0 returns 0 behind the checks.  The one kernel of its own (zero rows of the arena's blocks, the bf16 table) is in poison
 *   class 16. */
LINR_API int64_t linr_param_count_wide(int32_t scale_num, int32_t block_layers, int32_t hidden);
LINR_API size_t linr_net_wide_arena_bytes(int64_t rows, int32_t hidden, int32_t block_layers, int32_t bf16);
LINR_API int linr_net_forward_wide(const linr_frame* f, const float* params, int32_t hidden, void* arena, size_t arena_bytes,
                                   int32_t stage_begin, int32_t stage_end, float* probs, double* bits_acc, void* stream);
LINR_API int linr_net_forward_wide_bf16(const linr_frame* f, const uint8_t* codes, float min_param, float max_param, int32_t hidden,
                                        void* arena, size_t arena_bytes, int32_t stage_begin, int32_t stage_end, float* probs,
                                        double* bits_acc, void* stream);

/* ---- the training step of hidden_channel_conv 16 / 32 as C calls (csrc/wide_train.hip) ---------------------------------------------
 * The overfit iteration of main.py:305-321 at channels = 16 / 32: the teacher-forced forward (main.py:305-313, models/model_core.py:
 * 38-81), the autograd backward of main.py:315-316 and Adam of main.py:319 - the schedule of the host mirror (WideNet._forward(keep) /
 * _backward with the pointwise layers fused and the weight gradients of conv0_1 / conv1_1 paired) launch for launch through the
 * op-level entries above with the arguments the mirror hands them: bits, gradient and updated parameters are the mirror's bit for bit.
 * flags: 0, or LINR_MUL_BF16 = the products of every 3x3x3 convolution of the pass (forward, backward-data, weight gradient) on bf16
 *   matrix instructions (training option 'bf16-mul'); the forward and the backward of one step take the same flags.
 * linr_net_wide_train_arena_bytes: the arena of one frame (any scale_num): the tape - every activation in blocks of its own, since all
 *   of them stay live until the backward -, gradient blocks reused by role, the head and scale-context slabs, a 64 MiB region for the
 *   slabs of the deferred weight-gradient reductions (reduced in batches whenever it is full: every reduction is independent and keeps
 *   its fixed order), the bits partials and a gradient vector; 0 for rows < 0 or over the row bound of linr_frame, a hidden other than
 *   16 / 32, block_layers outside 1..4.  64-byte aligned; the library initialises whatever it reads of it.
 * linr_net_forward_train_wide (main.py:305-313): stages 0..8, the tape kept in the arena; bits_acc double[1], accumulated into, or NULL.
 * linr_net_backward_wide (main.py:315-316): WRITES d (gscale * bits) / d params into grads (linr_param_count_wide floats) - it does not
 *   add like linr_net_backward: the wide reductions write their destination, an adding form would need a second buffer and a pass
 *   over it.  Needs linr_net_forward_train_wide on the same frame, params, arena and flags before it.  The heads' gradient scale is
 *   (float)((double)gscale * log2 e).
 * linr_net_train_step_wide (main.py:305-321): forward, backward, Adam in one launch over the flat buffer; `args` as linr_net_train_step
 *   (scale_steps_h: an MLP whose count is 0 is skipped, every other one uses its own count, a scale of this frame with count 0 is an
 *   error; qparams: the fake quantisation runs in front, forward and backward read qparams, Adam - weight decay included - updates
 *   params).
 * Checked in front of the first launch, in this order: a NULL f / params / arena / args [/ grads] (LINR_EINVAL); the arena's alignment
 * (LINR_EALIGN); hidden; flags (LINR_EINVAL); the arena's size (LINR_EINVAL where linr_net_wide_train_arena_bytes is 0, else
 * LINR_ENOSPC); the step's arguments as linr_net_train_step checks them (step >= 1, the moments and bits_acc, qparams != params, its
 * alignment, bitdepth 2..16); the frame (linr_frame's structure, its matrices, nbr_ld, and nbr / nbr8t, which the weight-gradient
 * kernels read), then scale_steps_h against it.  rows == 0 returns 0 behind the checks and changes nothing.  No entry synchronises
 * with the host or keeps state in the library; the kernels of its own are in poison class 16. */
LINR_API size_t linr_net_wide_train_arena_bytes(int64_t rows, int32_t hidden, int32_t block_layers);
LINR_API int linr_net_forward_train_wide(const linr_frame* f, const float* params, int32_t hidden, void* arena, size_t arena_bytes,
                                         uint32_t flags, double* bits_acc, void* stream);
LINR_API int linr_net_backward_wide(const linr_frame* f, const float* params, int32_t hidden, void* arena, size_t arena_bytes,
                                    uint32_t flags, float gscale, float* grads, void* stream);
LINR_API int linr_net_train_step_wide(const linr_frame* f, float* params, int32_t hidden, void* arena, size_t arena_bytes,
                                      uint32_t flags, const linr_step_args* args, void* stream);

/* ---- bf16 training executor (BASELINE config[4]: "bf16 SparseConv"; beside the fp32 step above, never instead of it) --
 * The overfit iteration of main.py:305-321 - forward of models/model_core.py:38-81 / models/upsample.py:88-97,137-217 /
 * models/resnet.py:12-60, the autograd backward of main.py:315-316, Adam of main.py:231-237,319 - with bf16 feature AND gradient
 * rows ([1 + rows][8], 16-byte rows: one gather per tap), fp32 master parameters (`params`, updated by Adam in fp32), fp32
 * accumulation.  ONE rounding rule: every matrix written to memory is rounded to bf16 (RNE) and every consumer sees the stored
 * value; the 3x3x3 kernels are rounded to bf16 inside the kernels; biases, 1x1 convolutions, scale-context and head MLPs, sigmoid
 * and the bits are fp32 (bits accumulate in double).  oracle/network_bf16.py emulates these roundings with autograd; tolerances
 * are in tests/test_gpu_bf16_train.py.  The compressed kernel map only.
 * block_layers 1..4 of block_in (--block_layers, main.py:521; models/resnet.py:146-162): the depth is f->block_layers.  The extra
 * Inception layers run the same kernels one group at a time; the ResNetBlock's extra skip is ONE stored matrix S = bf16(I_last + A),
 * and the gradient arriving at every layer's input is rounded once, after its three contributions were summed in fp32 (the rule
 * above; tests/bf16_train_deep_ref.py emulates it with autograd, tolerances in tests/test_gpu_bf16_train_deep.py).
 * arena: linr_net_train_bf16_arena_bytes(rows, block_layers) bytes (0 for rows < 0 or a depth outside 1..4), 64-byte aligned,
 * shared by the calls of one step.
 * occ_bf16: NULL, or the frame's occupancy converted once by linr_occ_to_bf16 ([1 + rows][8] bf16, zero row in front; the
 * pointer passed is that of the ZERO row) - a frame's occupancy does not change over the epochs.
 * linr_net_forward_train_bf16: teacher-forced forward of all 8 stages, every activation the backward needs kept in the arena;
 *   probs [8][rows] stage-major or NULL; bits_acc double[1] (accumulated into) or NULL.
 * linr_net_backward_bf16: gradient of gscale * bits, ADDED into grads (fp32, linr_param_count floats); needs the forward above on
 *   the same arena.
 * linr_net_train_step_bf16: forward + backward + fixed-order reduction + Adam, `args` as linr_net_train_step; with args->qparams
 *   every kernel of the step, the weight images rounded to bf16 included, reads qparams, and Adam updates `params`. */
LINR_API size_t linr_net_train_bf16_arena_bytes(int64_t rows, int32_t block_layers);
LINR_API int linr_occ_to_bf16(const float* occ, int64_t rows, uint16_t* out_padded, void* stream);
LINR_API int linr_net_forward_train_bf16(const linr_frame* f, const float* params, void* arena, size_t arena_bytes,
                                const uint16_t* occ_bf16, float* probs, double* bits_acc, void* stream);
LINR_API int linr_net_backward_bf16(const linr_frame* f, const float* params, void* arena, size_t arena_bytes,
                           const uint16_t* occ_bf16, float gscale, float* grads, void* stream);
LINR_API int linr_net_train_step_bf16(const linr_frame* f, float* params, void* arena, size_t arena_bytes, const uint16_t* occ_bf16,
                             const linr_step_args* args, void* stream);
/* The backward of ONE convolution 8->8 of that executor as a stand-alone op (ME.MinkowskiConvolution's backward, models/resnet.py:15-51
 * under autograd): gin = bwd-data(gout; W) rounded to bf16 AND the kernel / bias gradient from one gather of gout.  gout / in / gin:
 * bf16 [n][8] whose row -1 exists (gout's must be zero); W fp32 [27][8][8] (rounded to bf16 in-kernel for backward-data);
 * slab: [nblocks][1736] floats = per-block partials [kernel 1728 | bias 8]; *rows_written of its rows are written (sum them). */
LINR_API int linr_spconv_bwd_fused_bf16(const uint16_t* gout, const uint16_t* in, const int32_t* lo, const uint32_t* mask, int64_t ld,
                               int64_t n, const float* W, uint16_t* gin, float* slab, int32_t nblocks, int32_t* rows_written,
                               void* stream);

/* ---- the overfit of a whole GOP as one call (opt-in; csrc/overfit.hip) ---------------------------------------------------------
 * main.py:297-437: `epochs` passes over the frames of a GOP in fixed order, one optimiser step and one StepLR step per frame
 * (main.py:305-321), the learning-rate clamp after each epoch (main.py:433-437), and the reference's checkpoint policy - keep the epoch
 * with the lowest mean loss (main.py:413-426,440-451).  Nothing of that depends on a value the host has to read: the learning rate and
 * the step counts follow from which frames hold which scales, the choice of the best epoch is a comparison of device values followed by a
 * conditional device copy.  So the whole GOP is queued at once and the stream is synchronised once, at its end.
 *
 * linr_overfit_plan (HOST only, no GPU call): the schedule.  frames_h: HOST [n_frames] pointers to linr_frame, of which n_scales,
 *   row_off_h, scale_idx_h are read (n_scales 1..16, every scale_idx_h in [0, model_scale_num)); the starting state (step = optimiser
 *   steps taken, sched_steps = StepLR steps taken, lr, scale_steps_h [model_scale_num] = updates of every per-scale context MLP so far,
 *   NULL = all zero); step_size >= 1, gamma, min_lr.  Step k = epoch * n_frames + frame receives lr_out[k] (the rate its update uses),
 *   step_out[k] (its 1-based count) and scale_steps_out[k * model_scale_num + s] (the counts of linr_step_args.scale_steps_h: a scale
 *   that has rows in the frame starts its counter, a started counter advances on every step - torch 1.13's optimizer.zero_grad() leaves
 *   zero tensors, see linr_net_train_step; a scale of a frame with zero rows is not present).  Behind every step: sched_steps += 1 and,
 *   when sched_steps % step_size == 0, lr *= gamma (one double multiply, the chainable StepLR form - a clamp persists).  Behind every epoch
 *   the state BEFORE the clamp goes to end_step / end_sched / end_lr [epochs] and end_scale_steps [epochs][model_scale_num], then
 *   lr = min_lr where lr < min_lr.  Any output may be NULL.  LINR_EINVAL: frames_h NULL, n_frames < 1, epochs < 0, model_scale_num
 *   outside 1..16, step_size < 1, a malformed frame.
 * linr_overfit_ws_bytes: the workspace of linr_overfit_gop - bits and point numbers [n_frames], losses [epochs], the flags and the
 *   snapshot of parameters and both moments (3 n_params floats); 0 for a negative argument.  16-byte aligned, uninitialised.
 * linr_overfit_gop: the overfit.  frames: HOST [args->n_frames]; args, result: HOST.  Checked in front of the first launch, in this
 *   order: NULL frames / args / result, params / exp_avg / exp_avg_sq / arena / ws (LINR_EINVAL); n_frames < 1; a NULL frame; epochs < 0,
 *   result->losses_h NULL with epochs > 0; qat_from outside [0, epochs]; qparams NULL with qat_from < epochs, bitdepth outside 2..16
 *   with qparams; step_size < 1, step < 0 or sched_steps < 0, a point_num that is not a positive finite number; an unknown executor; hidden (8 for
 *   LINR_OVERFIT_F32 / _BF16, 16 or 32 for _WIDE) and flags (0, or LINR_MUL_BF16 for _WIDE) (all LINR_EINVAL); frames that differ in
 *   model_scale_num or block_layers (LINR_EINVAL); params / ws alignment (LINR_EALIGN); ws_bytes (LINR_ENOSPC); then every frame with
 *   the arguments of its first step - and of its first quantisation-aware step - exactly as the executor's step entry checks them
 *   (the arena's size is LINR_ENOSPC there; a scale of a frame whose count would be 0 at its own step is LINR_EINVAL).
 *   Then, per epoch and frame, the executor's step (linr_net_train_step, _bf16, _wide: the same launches with the same arguments,
 *   gscale = (float)(1.0 / point_num), bits into the frame's slot), from epoch qat_from on with qparams; per epoch params_finite_k,
 *   epoch_close_k - losses[epoch] = (sum_j bits[j] / point_num[j]) / n_frames, summed in frame order in double, +inf when a parameter
 *   is not finite; the epoch is taken when it competes and its loss is below the best so far, so NaN and inf never win - and, with
 *   keep_best, snapshot_k (the conditional copy).  With keep_best and qat_from < epochs only epochs >= qat_from compete.  At the end
 *   the restore (on the device's own flag: only when an epoch was taken), ONE stream synchronisation, and `result`.
 *   No other host synchronisation, no state in the library.  A diverged overfit is no error code: its losses are inf, best_epoch -1.
 *   The three kernels are in profiler / poison class 12 (sums, reduction, Adam) for every executor. */
#define LINR_OVERFIT_F32  0          /* linr_net_train_step; hidden 8 */
#define LINR_OVERFIT_BF16 1          /* linr_net_train_step_bf16; hidden 8, the frames' block_layers 1..4 */
#define LINR_OVERFIT_WIDE 2          /* linr_net_train_step_wide; hidden 16 / 32, flags 0 or LINR_MUL_BF16 */
typedef struct linr_overfit_frame {
    const linr_frame* f;
    double point_num;               /* the frame's loss is bits / point_num (main.py:314) */
    const uint16_t* occ_bf16;       /* LINR_OVERFIT_BF16 only: as in linr_net_train_step_bf16, or NULL */
} linr_overfit_frame;
typedef struct linr_overfit_args {
    int32_t executor, hidden;
    uint32_t flags;
    int32_t n_frames;
    float* params;                  /* linr_param_count[_wide] floats, 16-byte aligned, updated */
    float* exp_avg;
    float* exp_avg_sq;
    double beta1, beta2, eps, weight_decay;          /* as in linr_step_args */
    double lr, min_lr, gamma;
    int64_t step_size;
    int64_t step, sched_steps;      /* the starting counters */
    const int64_t* scale_steps_h;   /* HOST [model_scale_num] or NULL (all zero) */
    int32_t epochs, keep_best;
    int32_t qat_from, bitdepth;     /* first quantisation-aware epoch (epochs: none); bitdepth is read with qparams */
    float* qparams;                 /* as in linr_step_args, or NULL */
    void* arena;                    /* the executor's arena for the largest frame, shared by all steps */
    size_t arena_bytes;
    void* ws;                       /* linr_overfit_ws_bytes(n_params, n_frames, epochs) bytes */
    size_t ws_bytes;
} linr_overfit_args;
typedef struct linr_overfit_result {          /* HOST; filled after the synchronisation */
    double* losses_h;               /* [epochs] */
    int32_t best_epoch;             /* -1: no finite competing epoch (or keep_best = 0) */
    double best_loss;               /* +inf then */
    /* the optimiser state that belongs to what is left in params: with keep_best and a best epoch that epoch's, before its clamp; else
     * the state after the last epoch's clamp */
    int64_t step, sched_steps;
    double lr;
    int64_t* scale_steps_h;         /* [model_scale_num] or NULL */
} linr_overfit_result;
LINR_API int linr_overfit_plan(const linr_frame* const* frames_h, int32_t n_frames, int32_t epochs, int32_t model_scale_num, int64_t step,
                               int64_t sched_steps, double lr, const int64_t* scale_steps_h, int64_t step_size, double gamma, double min_lr,
                               double* lr_out, int64_t* step_out, int64_t* scale_steps_out, int64_t* end_step, int64_t* end_sched,
                               double* end_lr, int64_t* end_scale_steps);
LINR_API size_t linr_overfit_ws_bytes(int64_t n_params, int32_t n_frames, int32_t epochs);
LINR_API int linr_overfit_gop(const linr_overfit_frame* frames, const linr_overfit_args* args, linr_overfit_result* result, void* stream);

/* ---- averaged weights (opt-in; csrc/params_avg.hip, csrc/params_avg_host.cpp) ----------------------------------------------------
 * What is coded after an overfit is the LAST iterate of an optimiser that still takes steps about one quantiser step wide.  These
 * entries keep K exponential averages of the iterates beside the training, so that the encoder may code one of them instead - where a
 * measured rate says so (codec.search_average); a decoder de-quantises whatever vector model.bin holds.
 *
 * linr_params_average: one update of all K averages,  avg[k][i] = fma(w_k, params[i] - avg[k][i], avg[k][i])  for i < n: the
 *   difference rounded to fp32 on its own, then one fused multiply-add - an exponential average with decay d_k = 1 - (double)w_k.
 *   Started from zero and updated T times, avg[k] * (1 / (1 - d_k^T)) is the debiased average (formed by the caller: one multiply per
 *   element, not hot).  params: device [n] floats, 16-byte aligned, read ONCE for all rows; weights_h: HOST [K] floats, each in
 *   (0, 1], K in 1..4, they travel as a kernel argument; avg: device [K][stride] floats, 16-byte aligned, stride >= n and a multiple
 *   of 4 (the elements behind n are not touched).  ONE launch, 16-byte accesses and a scalar tail, no atomics, no host
 *   synchronisation, no state in the library; profiler / poison class 12.  NaN and inf in params propagate into every row.
 *   n == 0 launches nothing.  Refused before the launch: n < 0, K, a NULL weights_h, a weight outside (0, 1] or NaN, stride, a NULL
 *   params / avg (LINR_EINVAL, in this order), then alignment (LINR_EALIGN).
 * linr_params_average_host: the same as a plain loop over HOST pointers (std::fmaf; no GPU needed, no alignment asked) - the
 *   definition of the arithmetic.
 * linr_overfit_gop_avg: linr_overfit_gop with the averaging launch queued behind EVERY training step (all executors: it reads
 *   args->params, the fp32 master).  avg->avg: device [n_avg][stride]; the first n_params floats of every row are zeroed by the
 *   call, so after it row k holds the average of all epochs * n_frames iterates (whatever epoch is kept).  avg is checked as
 *   linr_params_average checks its arguments, behind every check of linr_overfit_gop and in front of the first launch.  Training is
 *   untouched: parameters, moments, losses and `result` are those of linr_overfit_gop.  avg == NULL: linr_overfit_gop to the letter. */
typedef struct linr_overfit_avg {
    int32_t n_avg;                  /* 1..4 */
    float weight[4];                /* w_k = 1 - decay_k, each in (0, 1]; the first n_avg are read */
    float* avg;                     /* device [n_avg][stride], 16-byte aligned */
    int64_t stride;                 /* >= n_params, a multiple of 4 */
} linr_overfit_avg;
LINR_API int linr_params_average(const float* params, int64_t n, const float* weights_h, int32_t K, int64_t stride, float* avg, void* stream);
LINR_API int linr_params_average_host(const float* params_h, int64_t n, const float* weights_h, int32_t K, int64_t stride, float* avg_h);
LINR_API int linr_overfit_gop_avg(const linr_overfit_frame* frames, const linr_overfit_args* args, const linr_overfit_avg* avg,
                                  linr_overfit_result* result, void* stream);

/* Staged DECODE of one frame object (decoder.decode_one_frame, decoder.py:153-176 + CNP.decode, models/upsample.py:249-295) as
 * ONE call: for stage k = 0..7 { linr_net_forward[_bf16](k, k+1); probabilities of the stage -> pinned host buffer; the range
 * decoder on every scale's stream k (linr_ac_decode_binary, host); decoded symbols -> column k of f->occ } - the loop the
 * reference runs in Python with 16 .cpu() round trips per scale.  The call returns after the last stage (it synchronises
 * the stream once per stage by construction) and does not hold the Python GIL, so a host thread per frame scales.
 * streams_h / stream_len_h: HOST arrays [f->n_scales][8] of the per-stage streams (pack_bitstream payloads) and their byte
 * lengths; f->occ must be writable device memory (the frame's occupancy, zeroed by the caller; LINR_FRAME_OCC_PADDED honoured);
 * probs [8][rows] device scratch (holds all 8 stages' probabilities afterwards); p_pinned [rows] floats and s_pinned [rows]
 * bytes of page-locked host memory; s_dev [rows] bytes of device scratch.  codes == NULL: fp32 executor with `params`;
 * otherwise the bf16 / uint8-weight executor with codes, min_param, max_param (then `arena` is a linr_net_bf16_arena_bytes one).
 * A scale without rows is skipped, its streams unread.  A stream the range decoder refuses ends the call with the code of the first
 * such scale, before anything more is launched.  (csrc/decode.hip: decode_stages, the loop the decoder scales below share.) */
LINR_API int linr_net_decode_stages(const linr_frame* f, const float* params, const uint8_t* codes, float min_param,
                           float max_param, void* arena, size_t arena_bytes, const uint8_t* const* streams_h,
                           const int64_t* stream_len_h, float* probs, float* p_pinned, uint8_t* s_pinned, uint8_t* s_dev,
                           void* stream);

/* One scale of the decoder as one call - the body of decoder.decode_one_frame's loop (decoder.py:153-176): kernel map of the
 * level's coordinates, the 7-neighbour features read off it (instead of qscTensor.set_offset_tensor's 7 searches), the 8 decode
 * stages of linr_net_decode_stages, and octree_level.upper_layer (models/module_utils.py:117-127): the coordinates of the next finer
 * level = children 2 p + (dx, dy, dz) of every decoded octant 4 dx + 2 dy + dz, sorted x-major (radix sort of child_bits-bit-per-
 * axis keys).  coord: DEVICE int32 [n][3], sorted x-major, unique, n < 2^27; streams_h / stream_len_h: the 8 stage streams of this
 * scale (HOST); ws: DEVICE workspace of linr_decode_scale_ws_bytes bytes, 256-byte aligned; p_pinned / s_pinned: pinned HOST
 * buffers of n floats / n bytes; child_xyz: DEVICE int32 [child_cap][3] (8 n is always enough); *child_n_h receives the number of
 * children.  params (fp32 executor) or codes + min / max (bf16 / uint8-weight executor).  Synchronises the stream.  Between two
 * scales the caller only allocates the next workspace.  Arguments are checked before the first launch: LINR_EINVAL, then
 * LINR_EALIGN, then LINR_ENOSPC (short ws; more than child_cap children: after the stages, nothing is written past the cap);
 * n = 0 returns 0 with *child_n_h = 0 whatever the pointers are.
 *
 * linr_decode_scale_batch, the lock-step GOP decoder: the same for n_frames frames (1..LINR_DECODE_MAX_FRAMES) per call, with
 * N = seg_off_h[n_frames] rows (N < 2^26) and without a sort.  A row's arithmetic depends neither on the tiling nor on the rows
 * that share its launch, so the frames' levels, back to back, are one row space with one scale index as long as the kernel map
 * never links two frames (linr_kmap_build_segments); a stage then costs one launch set, one copy each way and n_frames range
 * decoders.  streams_h / stream_len_h: HOST [n_frames][8] (an empty frame's are not read); p_pinned / s_pinned: N floats / N bytes;
 * child_xyz: [child_cap][3] (8 N is always enough), frames back to back; child_off_h: HOST [n_frames + 1], the frames' child
 * offsets, zeroed before the pointer checks.  Everything else as above.  Both entries share everything between their argument
 * checks and the child expansion (csrc/decode.hip: scale_middle); they differ in the kernel-map call and the child expansion.
 * Their kernels belong to poison class 15 and to no linr_prof_* class.
 *
 * linr_children_segments, the batch entry's child expansion on its own: coords int32 [N,3] and occ fp32 [N][8] (0 / non-zero,
 * octant 4 dx + 2 dy + dz) of n_seg frames back to back, every frame sorted x-major, seg_off_h (HOST) [n_seg + 1] from 0 to N,
 * N < 2^26.  Writes the children 2 p + (dx, dy, dz) of every occupied octant to child_xyz [child_cap][3], x-major sorted within a
 * frame, frames back to back, and child_off_h (HOST) [n_seg + 1].  The parents are sorted already, so a child's position is a
 * closed form of four prefix sums over the rows (counts of the (dx, dy) pairs) and of the bounds of the row's (frame, x) and
 * (frame, x, y) runs: one scan, one scatter, no sort, no atomics.  LINR_ENOSPC when there are more than child_cap children (nothing
 * is written past the cap).  ws: linr_children_segments_ws_bytes(N) bytes, 256-byte aligned.  Synchronises the stream (one host
 * read of the n_seg + 1 offsets).
 *
 * Options of a scale (opts == NULL: {0, 1, 0}):
 * chunk_symbols = S > 0: CHUNKED stage streams (linr_stream_split_chunks below; side_info.json's stream_chunk).  A stream of n > S
 *   symbols is a header and k = ceil(n / S) chunks, and every chunk is decoded as an entry of its own: chunk j gives rows
 *   [j S, min((j + 1) S, n)) of its frame.  Every stream's header is parsed and checked before the first launch: LINR_EINVAL for a
 *   truncated length, one of more than 5 bytes, lengths that exceed the stream, or an S that is no multiple of 64 in 64..2^24.
 * n_threads: the host threads of a stage's range decoders (linr_ac_decode_binary_batch): at most one per entry of the stage - so a
 *   frame's plain stream is decoded on the calling thread - and with chunks at most one per 65,536 symbols of the stage, because
 *   the threads are started anew in every call.
 * device != 0 (opt-in): the range decoders on the DEVICE (linr_rc_decode_probs below).  The bytes of the scale's 8 streams of every
 *   frame are uploaded once (stream order, from a staging copy the call owns: the caller's stream arrays are free on return), and
 *   stage k is the stage's forward followed by rc_decode_k over the stage's entries, which write column k of the occupancy - no
 *   copy down, no host thread, and ONE synchronisation per scale, where the call reads the child count.  p_pinned, s_pinned and
 *   n_threads are unused.  The decoded geometry is that of the host path on every stream (the decoders agree on any bytes).
 *
 * Workspace (linr_decode_scale_ws_bytes / linr_decode_scale_batch_ws_bytes; bf16 = codes != NULL): stream_bytes_total = -1 is the
 * host decoders' layout (n_entries is ignored).  stream_bytes_total >= 0 is the device decoders': the same plus a region for the
 * stream bytes (stream_bytes_total = the sum of the 8 (x n_frames) stream lengths; padded to 256 bytes, at least 256, plus one
 * 256-byte window: the device layout is the host layout plus 512 bytes or more)
 * and one for the table (n_entries = the chunks of all 8 stages: the sum over frames and stages of linr_stream_chunk_count(rows of
 * the frame, chunk_symbols), empty frames excluded; more is allowed); a device scale whose ws_bytes is below what its plan needs is
 * LINR_ENOSPC.  0 for any other negative stream_bytes_total, a negative n_entries of the device layout, or rows / frames out of
 * range. */
typedef struct linr_decode_opts {
    int64_t chunk_symbols;   /* 0: plain stage streams; S: chunked (multiple of 64 in 64..2^24) */
    int32_t n_threads;       /* host range decoders of a stage; ignored when device != 0 */
    int32_t device;          /* 0: host range decoders (p_pinned / s_pinned required); 1: rc_decode_k, pinned buffers unused, may be NULL */
} linr_decode_opts;
LINR_API size_t linr_decode_scale_ws_bytes(int64_t n, int32_t block_layers, int32_t bf16, int64_t stream_bytes_total, int64_t n_entries);
LINR_API int linr_decode_scale(const int32_t* coord, int64_t n, int32_t scale_idx, int32_t model_scale_num, int32_t block_layers,
                      int32_t child_bits, const float* params, const uint8_t* codes, float min_param, float max_param,
                      const uint8_t* const* streams_h, const int64_t* stream_len_h, void* ws, size_t ws_bytes,
                      float* p_pinned, uint8_t* s_pinned, int32_t* child_xyz, int64_t child_cap, int64_t* child_n_h,
                      const linr_decode_opts* opts, void* stream);
LINR_API size_t linr_decode_scale_batch_ws_bytes(int64_t n_total, int32_t n_frames, int32_t block_layers, int32_t bf16,
                                        int64_t stream_bytes_total, int64_t n_entries);
LINR_API int linr_decode_scale_batch(const int32_t* coord, const int64_t* seg_off_h, int32_t n_frames, int32_t scale_idx,
                            int32_t model_scale_num, int32_t block_layers, const float* params, const uint8_t* codes,
                            float min_param, float max_param, const uint8_t* const* streams_h, const int64_t* stream_len_h,
                            void* ws, size_t ws_bytes, float* p_pinned, uint8_t* s_pinned, int32_t* child_xyz, int64_t child_cap,
                            int64_t* child_off_h, const linr_decode_opts* opts, void* stream);
/* The same four for a model of hidden_channel_conv = `hidden`: 16 / 32 run the stages on linr_net_forward_wide[_bf16] (params /
 * codes: linr_param_count_wide elements), 8 is the entries above; anything else is LINR_EINVAL (a size of 0).  Everything else -
 * the workspace layout but for the arena, the options, the checks and their order - is shared (csrc/decode.hip: scale_middle).
 * `hidden` belongs in linr_decode_opts: it moves there at the next ABI bump, and these four go. */
LINR_API size_t linr_decode_scale_wide_ws_bytes(int64_t n, int32_t block_layers, int32_t bf16, int64_t stream_bytes_total,
                                                int64_t n_entries, int32_t hidden);
LINR_API int linr_decode_scale_wide(const int32_t* coord, int64_t n, int32_t scale_idx, int32_t model_scale_num, int32_t block_layers,
                           int32_t child_bits, const float* params, const uint8_t* codes, float min_param, float max_param,
                           const uint8_t* const* streams_h, const int64_t* stream_len_h, void* ws, size_t ws_bytes,
                           float* p_pinned, uint8_t* s_pinned, int32_t* child_xyz, int64_t child_cap, int64_t* child_n_h,
                           const linr_decode_opts* opts, int32_t hidden, void* stream);
LINR_API size_t linr_decode_scale_batch_wide_ws_bytes(int64_t n_total, int32_t n_frames, int32_t block_layers, int32_t bf16,
                                                      int64_t stream_bytes_total, int64_t n_entries, int32_t hidden);
LINR_API int linr_decode_scale_batch_wide(const int32_t* coord, const int64_t* seg_off_h, int32_t n_frames, int32_t scale_idx,
                                 int32_t model_scale_num, int32_t block_layers, const float* params, const uint8_t* codes,
                                 float min_param, float max_param, const uint8_t* const* streams_h, const int64_t* stream_len_h,
                                 void* ws, size_t ws_bytes, float* p_pinned, uint8_t* s_pinned, int32_t* child_xyz, int64_t child_cap,
                                 int64_t* child_off_h, const linr_decode_opts* opts, int32_t hidden, void* stream);
LINR_API size_t linr_children_segments_ws_bytes(int64_t n);
LINR_API int linr_children_segments(const int32_t* coords, const float* occ, const int64_t* seg_off_h, int32_t n_seg, int32_t* child_xyz,
                           int64_t child_cap, int64_t* child_off_h, void* ws, size_t ws_bytes, void* stream);

/* ---- the executor's fused layers as stand-alone ops ------------------------------------------------------------
 * What linr_net_forward / _backward launch for one layer, callable (and testable) on its own.  All of them work on the
 * compressed kernel map (linr_kmap_compress) and follow the LINR_PAD_ROW contract: every matrix that a kernel GATHERS
 * from (named below) needs a readable all-zero row at index -1 and 16-byte aligned rows.
 *
 * Scale context (LINR_PCGC_Model.logic_core, models/model_core.py:48-53): x0[r] = W2 relu(W1 [emb_s | offset_feat[r]] + b1) + b2
 * with the weights of row r's scale; `f` supplies rows, row_off_h, scale_idx_h, model_scale_num, block_layers (parameter
 * layout) and offset_feat.  mix [rows][16], hid [rows][16], x0 [rows][8].  bwd: ghid = (W2^T gx0) * (hid > 0). */
LINR_API int linr_sce_fwd(const float* params, const linr_frame* f, float* mix, float* hid, float* x0, void* stream);
LINR_API int linr_sce_bwd(const float* params, const linr_frame* f, const float* gx0, const float* hid, float* ghid,
                 void* stream);
/* The complete backward of the scale context (model_core.py:48-53 under autograd) as one call: d loss / d (scale_emb, every scale MLP
 * of the frame) into grads[0 .. linr_sce_param_count(model_scale_num)) - these parameters lead the flat parameter order
 * (scale_emb, scale_mlp.{s}.{0,2}) whatever the width of the rest of the network, so `params` / `grads` may be the flat buffers of a
 * hidden_channel_conv 16 / 32 model.  gx0 [rows][8], hid [rows][16] as kept by linr_sce_fwd (whose mix may be NULL); scales the frame
 * does not contain get zero gradients.  slab: linr_sce_bwd_params_slab_bytes(model_scale_num) bytes of scratch. */
LINR_API int64_t linr_sce_param_count(int32_t model_scale_num);
LINR_API size_t linr_sce_bwd_params_slab_bytes(int32_t model_scale_num);
LINR_API int linr_sce_bwd_params(const float* params, const linr_frame* f, const float* gx0, const float* hid, float* slab,
                                 size_t slab_bytes, float* grads, void* stream);

/* Occupancy head of one stage = CNP.basic_module + the stage's BCE term (models/upsample.py:137-161,
 * models/model_core.py:76-81): c = conv3(prior; Wp, bp) (gathers `prior` [n][8]), z = w2 . relu(W1 c + b1) + b2,
 * p = sigmoid(z); if bits_acc != NULL the stage's bits (target = occupancy column, stride target_ld) are ADDED into it
 * (fixed-order block partials in ws).  bwd: gc = d(gscale * bits)/dc and the head-MLP gradients
 * ghead[241] = [gW1 24x8 | gb1 24 | gw2 24 | gb2 1] (parameters() order of inner_mlps.k.0), deterministic.
 * ws: linr_head_workspace_bytes(n) bytes, 16-byte aligned. */
LINR_API size_t linr_head_workspace_bytes(int64_t n);
LINR_API int linr_head_fwd(const float* prior, const int32_t* lo, const uint32_t* mask, int64_t ld, int64_t n,
                  const float* Wp, const float* bp, const float* w1, const float* b1, const float* w2, const float* b2,
                  const float* target, int32_t target_ld, float* c_out, float* p_out, double* bits_acc, void* ws,
                  size_t ws_bytes, void* stream);
LINR_API int linr_head_bwd(const float* c, const float* p, const float* target, int32_t target_ld, const float* w1,
                  const float* b1, const float* w2, float gscale, float* gc, int64_t n, float* ghead, void* ws,
                  size_t ws_bytes, void* stream);

/* One InceptionResNet layer (models/resnet.py:55-60) in two launches: H = [relu(conv0_0(x)) | relu(conv1_0(x))],
 * M = relu(conv1_1(H[:,4:8])), I = [conv0_1(H[:,0:4]) | conv1_2(M)] + x.  x, H are gathered.  All [n][8] except M [n][4].
 * bwd_data: from gI (gathered) the launches of the backward data chain: gM = (gI[:,4:8] W12^T) * (M > 0) (gathered),
 * gH = [bwd(gI[:,0:4]; W01) | bwd(gM; W11)] * (H > 0) (gathered), gX = bwd(gH[:,0:4]; W00) + gI + gH[:,4:8] W10^T
 * (+ old gX: LINR_ACCUM) (* (x > 0): LINR_RELU_MASK, x = the ReLU output that fed the layer). */
typedef struct linr_inception_params {
    const float *w00, *b00;   /* conv0_0 [27][8][4], [4] */
    const float *w01, *b01;   /* conv0_1 [27][4][4], [4] */
    const float *w10, *b10;   /* conv1_0 [8][4], [4]     */
    const float *w11, *b11;   /* conv1_1 [27][4][4], [4] */
    const float *w12, *b12;   /* conv1_2 [4][4], [4]     */
} linr_inception_params;
LINR_API int linr_inception_fwd(const float* x, const int32_t* lo, const uint32_t* mask, int64_t ld, int64_t n,
                       const linr_inception_params* q, float* H, float* M, float* I, void* stream);
LINR_API int linr_inception_bwd_data(const float* gI, const float* x, const float* H, const float* M, const int32_t* lo,
                            const uint32_t* mask, int64_t ld, int64_t n, const linr_inception_params* q, float* gM,
                            float* gH, float* gX, uint32_t flags, void* stream);
/* weight gradients of the layer's two 4->4 convolutions in one pass (conv0_1 on H[:,0:4] with gradient g0, conv1_1 on
 * H[:,4:8] with g1): 512 per-block partials slab[b][872] = [gW01 432 | gb01 4 | gW11 432 | gb11 4], summed in ascending b. */
LINR_API int linr_spconv_wgrad_dual44(const float* H, const float* g0, int32_t g0_ld, const float* g1, int32_t g1_ld,
                             const int32_t* nbr, const int32_t* tile8t, int64_t ld, int64_t n, float* slab, void* stream);

/* The backward of an Inception layer's two convolution pairs in the same form (models/resnet.py:55-60; gM comes from the
 * caller: the tail convolution's epilogue or a pointwise op):
 *   gH = [bwd(gI[:, 0:4]; W01) | bwd(gM; W11)] * (H > 0)  with dW01, db01, dW11, db11  (one gather of [gI[:, 0:4] | gM]), then
 *   gX = (bwd(gH[:, 0:4]; W00) + gI (+ old gX: LINR_ACCUM) + gH[:, 4:8] @ W10^T) (* (x > 0): LINR_RELU_MASK)  with dW00, db00 and,
 *        on lanes the 11-tap last chunk leaves idle, dW10 = x^T gH[:, 4:8], db10 of the 1x1 conv1_0.
 * gH and gX are bit-identical to linr_inception_bwd_data's.  slab: [nblocks][1776] per-block partials
 * [W00 864 | b00 4 | W01 432 | b01 4 | W11 432 | b11 4 | W10 32 | b10 4], every row written; sum over the rows = the gradients.
 * conv1_2's gradient (M^T gI[:, 4:8]) is linr_linear_bwd_weight's job.  gI, gH, gX, x, H: [n][8], gM: [n][4], all
 * 16-byte aligned; gI, gM and gH need the zero row at index -1. */
LINR_API int linr_inception_bwd_fused(const float* gI, const float* gM, const float* x, const float* H, const int32_t* lo,
                             const uint32_t* mask, int64_t ld, int64_t n, const linr_inception_params* q, float* gH, float* gX,
                             uint32_t flags, float* slab, int32_t nblocks, void* stream);

/* Weight gradients of the FIRST convolutions of the 7 outter blocks (block b = 1..7: conv3(occ[:, :b] -> 8) on the same occupancy
 * rows, models/upsample.py:206-214; ME: seven MinkowskiConvolution backward-weight calls) from ONE gather of the occupancy rows:
 *   gW_b[k][ci][co] = sum_r occ[nbr(r, k)][ci] * gout7[b - 1][r][co]  (ci < b),   gb_b[co] = sum_r gout7[b - 1][r][co].
 * occ [n][8] with the zero row at index -1; gout7_h: HOST array of 7 device pointers [n][8] (the gradients behind the ReLU);
 * everything 16-byte aligned.  slab: [nblocks][6104] per-block partials, for b = 1..7: kernel [27][b][8] then bias [8]; only the
 * first *rows_written_h (<= nblocks) rows are written - sum over those rows = the gradients. */
LINR_API int linr_occ_wgrad7(const float* occ, const float* const* gout7_h, const int32_t* lo, const uint32_t* mask, int64_t ld,
                    int64_t n, float* slab, int32_t nblocks, int32_t* rows_written_h, void* stream);
/* First convolutions of the 7 outter blocks (models/upsample.py:206-214 -> make_block's first conv + ReLU): block g + 1
 * computes relu(conv3(occ[:, :g+1]; kernel [27][g+1][8]) + bias) on the SAME gathered occupancy rows, so one gather feeds
 * all seven.  occ [n][8] (gathered); kernel / bias of block g at params + w_off_h[g] / b_off_h[g]; result of block g at
 * out + out_off_h[g] ([n][8], element offsets, multiples of 4). */
LINR_API int linr_occ_conv7(const float* occ, const int32_t* lo, const uint32_t* mask, int64_t ld, int64_t n,
                   const float* params, const int64_t* w_off_h, const int64_t* b_off_h, float* out,
                   const int64_t* out_off_h, void* stream);

/* ---- arithmetic-coder feed (host side) -----------------------------------------------------------------------
 * Replaces torchac.encode_float_cdf / decode_float_cdf as used by BinaryArithmeticCoding
 * (models/module_utils.py:8-40; callers models/upsample.py:224-237,275; models/model_core.py:204-208) and by the
 * model stream (model_compression/model_size_est.py:470-482,545-563).  Follows torchac 0.9.3's published
 * coder (un-vendored, pinned in enviroment.yaml:32); the one known-answer vector the reference ships (the model stream of
 * loot/gop_32_62: 282,642 bits) is consistent with this coder in two ways that cannot be told apart offline - 35,319 bytes with
 * the CPU's Laplace pdf plus a 90-bit header of an older revision, or 35,320 bytes plus today's 82-bit header if the CUDA pdf
 * the reference builds its CDF from differs in the last bit (tests/test_oracle_golden.py::test_model_stream_known_answer).
 * Consequence for interop: a model.bin whose CDF was built on another device decodes only if that device's expf agrees to the
 * last bit on the 256 pdf values.  Real torchac is not installable here, so byte-compatibility beyond that vector is by
 * construction, not by test.
 * All pointers here are HOST pointers.  Return: bytes written (>= 0) or a negative LINR_E* code. */
LINR_API int64_t linr_ac_encode_binary(const float* prob_h, const uint8_t* sym_h, int64_t n, uint8_t* out_h, int64_t cap);
LINR_API int     linr_ac_decode_binary(const float* prob_h, int64_t n, const uint8_t* in_h, int64_t in_len, uint8_t* sym_h);
LINR_API int64_t linr_ac_encode_cdf16(const uint16_t* cdf_h, int32_t lp, int32_t cdf_shared, const int16_t* sym_h,
                             int64_t n, uint8_t* out_h, int64_t cap);
LINR_API int     linr_ac_decode_cdf16(const uint16_t* cdf_h, int32_t lp, int32_t cdf_shared, int64_t n,
                             const uint8_t* in_h, int64_t in_len, int16_t* sym_h);
/* n_streams independent binary streams coded on a thread pool (8 stages x scales are independent streams) */
LINR_API int linr_ac_encode_binary_batch(const float* const* prob_h, const uint8_t* const* sym_h, const int64_t* n,
                                int32_t n_streams, uint8_t* const* out_h, const int64_t* cap,
                                int64_t* out_len, int32_t n_threads);
/* The decode twin: n_streams independent binary streams decoded on a thread pool (the frames of a lock-step decode group are
 * independent streams).  Stream i: n[i] symbols from in_h[i] / in_len[i] against prob_h[i] into sym_h[i], as linr_ac_decode_binary.
 * Returns the first non-zero code a stream returned, else 0; no thread is left running on return. */
LINR_API int linr_ac_decode_binary_batch(const float* const* prob_h, const int64_t* n, const uint8_t* const* in_h,
                                const int64_t* in_len, int32_t n_streams, uint8_t* const* sym_h, int32_t n_threads);
/* The same coder fed with code values instead of probabilities (BinaryArithmeticCoding, models/module_utils.py:8-40; callers
 * models/upsample.py:224-239): c1_h[i] = (rint((1 - p[i]) * 65534) + 1) & 0xFFFF, the one cdf entry a binary symbol needs,
 * and the symbols as bits - symbol i is bit i & 31 of sym_h[i >> 5] (ceil(n / 32) words are read).  Interval update,
 * renormalisation and termination are those of linr_ac_encode_binary / _decode_binary (one loop body serves both forms), so
 * code values computed as above give the same bytes.  The decoder writes one byte per symbol, like linr_ac_decode_binary. */
LINR_API int64_t linr_ac_encode_binary_codes(const uint16_t* c1_h, const uint32_t* sym_h, int64_t n, uint8_t* out_h, int64_t cap);
LINR_API int     linr_ac_decode_binary_codes(const uint16_t* c1_h, int64_t n, const uint8_t* in_h, int64_t in_len, uint8_t* sym_h);
LINR_API int linr_ac_encode_binary_codes_batch(const uint16_t* const* c1_h, const uint32_t* const* sym_h, const int64_t* n,
                                      int32_t n_streams, uint8_t* const* out_h, const int64_t* cap,
                                      int64_t* out_len, int32_t n_threads);
/* linr_ac_decode_binary through the DEVICE decoder's body (csrc/rc_dec_body.h, what rc_decode_k below runs a wave per entry) on the
 * CPU: 64-symbol chunks of code values, the stream through aligned 64-word windows with the funnel shift and the masked last word,
 * exactly as the wave walks them.  Same arguments, same symbols on ANY bytes (both decoders read zeros at and behind in_h + in_len;
 * no byte there is read); it shares no text with linr_ac_decode_binary, which is its reference (tests/test_rc_decode_host.py). */
LINR_API int     linr_ac_decode_binary_twin(const float* prob_h, int64_t n, const uint8_t* in_h, int64_t in_len, uint8_t* sym_h);
/* Chunked stage streams (opt-in; side_info.json's stream_chunk = S, a multiple of 64 in 64..2^24): a stage stream of n symbols has
 * k = max(1, ceil(n / S)) chunks, chunk j being exactly the stream of symbols [j S, min((j + 1) S, n)) on their own.  k == 1: the
 * stream is that chunk, i.e. the unchunked stream.  k > 1: the byte lengths of chunks 0 .. k - 2 as unsigned LEB128 of at most 5
 * bytes each, then the chunks; the last chunk takes the bytes that remain (a decoder knows n and S, so there is no count field).
 * linr_stream_chunk_count: k (1 for S == 0, "not chunked"), LINR_EINVAL for n < 0 or a bad S.
 * linr_stream_split_chunks: chunk_h[j] / chunk_len[j], j < k, point into in_h; returns k.  LINR_EINVAL for a truncated length, a
 * length of more than 5 bytes, lengths that together exceed the bytes present, or bad arguments; LINR_ENOSPC for max_chunks < k.  No
 * byte at or behind in_h + in_len is read, and a refused stream writes nothing to chunk_h / chunk_len. */
LINR_API int64_t linr_stream_chunk_count(int64_t n, int64_t chunk_symbols);
LINR_API int64_t linr_stream_split_chunks(const uint8_t* in_h, int64_t in_len, int64_t n, int64_t chunk_symbols,
                                 const uint8_t** chunk_h, int64_t* chunk_len, int64_t max_chunks);
/* Those inputs computed on the DEVICE (csrc/ac_codes.hip), one launch on `stream`: what BinaryArithmeticCoding.encode
 * (models/module_utils.py:8-40) derives from the probabilities and occupancy of CNP.encode (models/upsample.py:224-239) on the
 * host.  probs [8][probs_ld] fp32 in [0, 1] (plane k = stage k, as linr_net_forward writes them), occ [n][occ_ld] fp32, 0 or
 * non-zero, column k = stage k (a frame's occupancy BEHIND its zero row).  c1 [8][c1_ld] uint16 receives the code values - fp32
 * 1 - p, then fp32 * 65534, two roundings as on the host, then round to nearest even, + 1, & 0xFFFF; sym [8][sym_ld] uint32 the
 * bit planes: bit i & 31 of word i >> 5 of plane k = (occ[i][k] != 0), the unused high bits of word linr_ac_codes_sym_words(n) - 1
 * zero.  Elements [n, c1_ld) of a code plane and words beyond linr_ac_codes_sym_words(n) = ceil(n / 32) are not written.  LINR_EINVAL
 * for a NULL pointer, n < 0, probs_ld < n, c1_ld < n, sym_ld < words, occ_ld < 8 or n >= 2^27 - 1; n == 0 launches nothing.
 * The kernel uses no LDS and belongs to no linr_prof_* / linr_debug_poison class (all 24 are taken). */
LINR_API size_t linr_ac_codes_sym_words(int64_t n);
LINR_API int linr_ac_codes(const float* probs, int64_t probs_ld, const float* occ, int32_t occ_ld, int64_t n, uint16_t* c1,
                  int64_t c1_ld, uint32_t* sym, int64_t sym_ld, void* stream);

/* ---- range coder on the DEVICE (csrc/ac_device.hip, body: csrc/rc_body.h) ------------------------------------------------
 * linr_ac_encode_binary_codes for many independent streams in one call, a wave per stream: only stream bytes and lengths have to
 * cross to the host.  The bytes are the host coder's bytes: both run the one body of csrc/rc_body.h.  Stream i codes n symbols whose code values start at element c1_off of
 * c1_dev (uint16) and whose symbol bits start at bit 0 of word sym_off of sym_dev (bit j & 31 of word sym_off + (j >> 5), ceil(n / 32)
 * words are read), into out_dev + out_off (a multiple of 4), at most cap bytes: no byte at or behind out_off + cap is written. */
typedef struct linr_rc_stream {
    int64_t c1_off, sym_off, n, out_off, cap;
} linr_rc_stream;
/* Workspace of linr_rc_encode_codes for n_streams streams whose caps sum to total_cap: the device copy of the table, the scan's
 * input and temporary storage.  0 for negative arguments. */
LINR_API size_t linr_rc_encode_ws_bytes(int32_t n_streams, int64_t total_cap);
/* Three launches on `stream`: rc_encode_k (len_dev[i] = length of stream i in bytes, or LINR_ENOSPC when it needs more than its
 * cap - the other streams of the call are unaffected), an exclusive scan of the lengths (a negative one counts as 0) into
 * offsets_dev [n_streams + 1] int64, and rc_pack_k, which gathers the streams into payload_dev: stream i is
 * payload[offsets[i] .. offsets[i + 1]).  A host then needs two small reads: the offsets, then payload[:offsets[n_streams]].
 * streams_host is a HOST array; it is checked completely before the first launch and may be freed when the call returns.
 * LINR_EINVAL, nothing launched: a NULL pointer (with n_streams > 0), n_streams < 0, a stream with n < 0, cap < 0, negative
 * offsets, n >= 2^27 - 1, out_off not a multiple of 4, an out region that ends behind out_bytes or overlaps another stream's,
 * payload_bytes below the sum of the caps, ws_bytes below linr_rc_encode_ws_bytes(n_streams, sum of caps).
 * LINR_EALIGN: out_dev or ws not 8-byte aligned.  n_streams == 0 returns 0 and launches nothing.
 * The kernels use no LDS and no atomics and belong to no linr_prof_* / linr_debug_poison class (all 24 are taken). */
LINR_API int linr_rc_encode_codes(const uint16_t* c1_dev, const uint32_t* sym_dev, const linr_rc_stream* streams_host, int32_t n_streams,
                         uint8_t* out_dev, int64_t out_bytes, int64_t* len_dev, uint8_t* payload_dev, int64_t payload_bytes,
                         int64_t* offsets_dev, void* ws, size_t ws_bytes, void* stream);
/* linr_rc_encode_codes for chunked stage streams, a wave per CHUNK: with chunk_symbols = S stream i has k_i =
 * linr_stream_chunk_count(n, S) chunks, and payload[offsets[i] .. offsets[i + 1]) receives its final bytes - the LEB128 lengths of
 * chunks 0 .. k_i - 2 and the chunks, or the lone chunk - byte for byte what the host coder's chunks joined give.  The table stays
 * per stream and is checked as above; the chunks' descriptors are derived on the device from it and from the host's prefix sum of
 * the k_i.  Chunk j of a stream with k > 1 owns the 2 n_j + 64 bytes at out_off + j (2 S + 64), so such a stream needs
 * cap >= 2 n + 64 k (LINR_EINVAL otherwise); a stream of one chunk keeps its own cap.  len_dev[i] is the final length, or LINR_ENOSPC
 * when one of its chunks needed more than its region (then it counts 0 in the offsets).  payload_bytes must reach the sum of the caps
 * + 5 (chunks - streams), ws_bytes linr_rc_encode_chunked_ws_bytes(n_streams, chunks) (0 for n_chunks < n_streams or >= 2^31 - 1);
 * ws 16-byte aligned.  Launches: the two uploads, the chunk table, rc_encode_k unchanged, a scan over the chunks, one over the
 * streams, the pack.  No LDS, no atomics, no floating point.  chunk_symbols == 0 IS linr_rc_encode_codes. */
LINR_API size_t linr_rc_encode_chunked_ws_bytes(int32_t n_streams, int64_t n_chunks);
LINR_API int linr_rc_encode_codes_chunked(const uint16_t* c1_dev, const uint32_t* sym_dev, const linr_rc_stream* streams_host,
                                 int32_t n_streams, int64_t chunk_symbols, uint8_t* out_dev, int64_t out_bytes, int64_t* len_dev,
                                 uint8_t* payload_dev, int64_t payload_bytes, int64_t* offsets_dev, void* ws, size_t ws_bytes,
                                 void* stream);

/* ---- range DECODER on the DEVICE (csrc/ac_device_dec.hip, body: csrc/rc_dec_body.h) ---------------------------------------
 * linr_ac_decode_binary for many independent entries in one launch, a wave per entry, from probabilities that never leave the device:
 * entry i decodes n symbols against probs_dev[p_off .. p_off + n) (fp32 in [0, 1]; the code value is computed as linr_ac_codes
 * computes it) from the bytes [in_off, in_off + in_len) of bytes_dev - in_off has NO alignment; whatever follows the entry's last
 * byte reads as zeros, as the host decoder reads past a stream's end - and writes symbol j as 0.0f / 1.0f to
 * occ_col_dev[(out_row + j) * occ_ld] (a column of an occupancy matrix: pass occ + k and occ_ld = 8) and, with sym_dev != NULL, as a
 * byte to sym_dev[out_row + j].  Nothing else is written.  An entry is a whole stream or one chunk of a chunked stream. */
typedef struct linr_rc_dec_entry {
    int64_t p_off, n, in_off, in_len, out_row;
} linr_rc_dec_entry;
/* Workspace of linr_rc_decode_probs: the device copy of the table.  0 for a negative count. */
LINR_API size_t linr_rc_decode_ws_bytes(int32_t n_entries);
/* The table's upload (kernel arguments: entries_host is a HOST array and free on return) and rc_decode_k, on `stream`; no
 * synchronisation.  The whole table is checked before the first launch - LINR_EINVAL, nothing written: a NULL pointer (sym_dev may be
 * NULL; bytes_dev too when bytes_len is 0), n_entries < 0, occ_ld < 1, a negative field, p_off + n > n_probs, in_off + in_len >
 * bytes_len, out_row + n > n_rows, two entries whose row ranges [out_row, out_row + n) overlap, ws_bytes below
 * linr_rc_decode_ws_bytes(n_entries).  LINR_EALIGN: probs_dev, occ_col_dev or bytes_dev not 4-byte aligned, ws not 8-byte aligned.
 * bytes_dev is read in aligned 32-bit words: it must be readable up to bytes_len rounded up to a multiple of 4, and no address at or
 * behind that is formed (a 256-byte aligned buffer makes every window one full-line load).  n_entries == 0 returns 0 and launches
 * nothing.  The kernel uses no LDS, no atomics and no scratch, and belongs to no linr_prof_* class; on its own it belongs to no
 * linr_debug_poison class either (inside the decoder scales below it sits behind class 15). */
LINR_API int linr_rc_decode_probs(const float* probs_dev, int64_t n_probs, const uint8_t* bytes_dev, int64_t bytes_len,
                         const linr_rc_dec_entry* entries_host, int32_t n_entries, float* occ_col_dev, int64_t occ_ld, int64_t n_rows,
                         uint8_t* sym_dev, void* ws, size_t ws_bytes, void* stream);

/* ---- geometry digests (opt-in; csrc/digest.hip, body: csrc/digest_body.h) -------------------------------------------------------
 * What an encoder records of every octree level of a frame and a decoder checks as soon as it has decoded the level
 * (linr_pcgc_amd/stream_digests.py: bins/digests.bin holds D >> 32).  The digest of a multiset of int32 rows (x, y, z), with an
 * optional origin added first; all arithmetic unsigned 64-bit and wrapping, u32(a) the 32-bit pattern of a:
 *   G        = 0x9E3779B97F4A7C15
 *   m(v):      v ^= v >> 30;  v *= 0xBF58476D1CE4E5B9;  v ^= v >> 27;  v *= 0x94D049BB133111EB;  v ^= v >> 31
 *   r(x,y,z) = m( m( u32(x) | u32(y) << 32 ) + u32(z) + G )       with (x, y, z) = row + origin, added in int32 (wrapping)
 *   S        = sum of r over the n rows (mod 2^64);   D = m( S ^ m(n + G) )
 * Integer adds and multiplies only, so any reduction order gives the same value: it is a digest of the SET of rows, not of their order
 * (the decoders' row order is fixed by construction).  It detects errors; it is not cryptographic.
 * linr_coords_digest_segments: coords_dev [N][3] int32, 4-byte aligned; segment j is rows [seg_off_h[j], seg_off_h[j + 1]) of it
 * (seg_off_h: n_seg + 1 HOST offsets, non-negative and non-decreasing; empty segments allowed), 1 <= n_seg <= LINR_DECODE_MAX_FRAMES;
 * origins_h: HOST int32 [n_seg][3] or NULL (all zero).  digest_dev[j] (8-byte aligned) holds D of segment j once `stream` reaches that
 * point; the entry does not synchronise and writes nothing but digest_dev[0 .. n_seg) and its workspace (ws:
 * linr_coords_digest_ws_bytes(n_seg) bytes - 0 for n_seg out of range -, 8-byte aligned, uninitialised).  The table travels as kernel
 * arguments: the host arrays are free on return.  Two launches - a grid of (at most 256 workgroups, segment) that leaves one partial sum
 * per workgroup in ws, one wave per segment that sums them and finalises -, no atomics.  Checked before the first launch, and a refused
 * call writes nothing: LINR_EINVAL for a NULL pointer (origins_h may be NULL; coords_dev too when every segment is empty), n_seg out of
 * range, a negative or decreasing seg_off_h; LINR_EALIGN for a misaligned coords_dev, digest_dev or ws; LINR_ENOSPC for a short
 * workspace.  The kernels sit behind linr_debug_poison class 15 (the decoder scales') and belong to no linr_prof_* class.
 * linr_coords_digest_host: the same D for n rows in HOST memory with one origin (HOST int32 [3] or NULL) as a plain loop; no GPU
 * involved, thread-safe.  n <= 0 (or coords_h NULL): the digest of no rows. */
LINR_API size_t   linr_coords_digest_ws_bytes(int32_t n_seg);
LINR_API int      linr_coords_digest_segments(const int32_t* coords_dev, const int64_t* seg_off_h, int32_t n_seg, const int32_t* origins_h,
                                     uint64_t* digest_dev, void* ws, size_t ws_bytes, void* stream);
LINR_API uint64_t linr_coords_digest_host(const int32_t* coords_h, int64_t n, const int32_t* origin_h);

/* ---- frame input (host) ----------------------------------------------------------------------------------------------
 * Body of an ASCII PLY (datautils/custom_dataset.py:9-14 read_ply_o3d - open3d's C++ reader - followed by :263-269, which keeps
 * the rounded x, y, z).  text_h / len: the bytes BEHIND "end_header\n"; n_rows vertices of n_cols whitespace-separated numbers,
 * one vertex per line (empty lines between vertices tolerated); cx, cy, cz: the columns of x, y, z.  xyz_h [n_rows][3] receives
 * the values rounded to the nearest integer (ties to even, like numpy.rint).  Returns 0, or LINR_EINVAL for a short / malformed
 * line, a non-finite coordinate or bad arguments; *rows_parsed_h (optional) = the vertices completed before the error.
 * Host pointers only; no GPU involved; thread-safe (linr_pcgc_amd/ply.py reads the frames of a GOP on a thread pool). */
LINR_API int linr_ply_parse_ascii(const char* text_h, size_t len, int64_t n_rows, int32_t n_cols, int32_t cx, int32_t cy,
                         int32_t cz, int64_t* xyz_h, int64_t* rows_parsed_h);

/* ---- frame input (device) --------------------------------------------------------------------------------------------
 * The same bodies parsed on the DEVICE (csrc/ply_parse.hip), for callers that want the coordinates there anyway.
 * linr_ply_parse_ascii_device: text_d / len are the bytes BEHIND "end_header\n" in device memory, text_d 16-byte aligned,
 * len <= 2^31 - 1 (offsets are 32-bit).  The contract is linr_ply_parse_ascii's: n_rows vertices of n_cols (3..64) whitespace-separated
 * numbers, one vertex per line, a line ended by '\n' only, blanks ' ' \t \r \f \v, whitespace-only lines between vertices tolerated,
 * everything behind the n_rows-th non-empty line ignored, a last line without a newline complete.  No byte at or past text_d + len is
 * read.  xyz_d [n_rows][3] int32 receives columns cx, cy, cz rounded to the nearest integer, ties to even.  status_d: 2 int64 in
 * device memory, 8-byte aligned, set to {0, n_rows} in stream order before anything else and left as {flags, first_row}: flags == 0
 * when every one of the first n_rows non-empty lines was handled on the device, else an OR of
 *   LINR_PLY_TOKEN    a token is not [+-] digits [. digits] with 1..15 digits in all (the host parser takes such tokens to strtod:
 *                     they may be valid);
 *   LINR_PLY_COLUMNS  a line ended before n_cols tokens, or has a non-blank byte behind them;
 *   LINR_PLY_SHORT    fewer than n_rows non-empty lines;
 *   LINR_PLY_RANGE    a rounded value is outside int32 (linr_ply_gather_binary: or not finite);
 * first_row is the smallest vertex index that raised a flag (LINR_PLY_SHORT: the number of non-empty lines found).  Rows without a flag
 * are written correctly in every case, rows with one are unspecified: a caller that sees flags != 0 hands the same bytes to
 * linr_ply_parse_ascii.  The device takes the host parser's fast path only and takes it exactly: mant / 10^f rounded in integers is what
 * the host's correctly rounded double division followed by nearbyint gives for at most 15 digits.
 * ws_d: linr_ply_parse_ws_bytes(len, n_rows) bytes (0 for len over the bound or n_rows < 0), 256-byte aligned, uninitialised.
 * linr_ply_gather_binary: rec_d holds n_rows records of `stride` bytes (no alignment); field j of a record lies at byte off[j] and
 * has type code type[j]: 0 i1, 1 u1, 2 i2, 3 u2, 4 i4, 5 u4, 6 f4, 7 f8 (off / type are HOST arrays), little endian or, with
 * big_endian != 0, big endian.  Every value is converted exactly to double and rounded with rint; xyz_d and status_d as above.
 * Both check their arguments before the first launch: LINR_EINVAL for n_rows < 0, a NULL pointer with n_rows > 0, n_cols outside
 * 3..64, a column outside [0, n_cols), len over the bound, stride <= 0, a type code outside 0..7 or a field that does not lie inside
 * the record; LINR_ENOSPC for a short workspace; LINR_EALIGN for a misaligned text_d, ws_d, xyz_d or status_d.  n_rows == 0 returns
 * 0, launches nothing and leaves *status_d untouched.  Stream-ordered, nothing allocated, no LDS, no float atomics; the kernels belong to
 * no linr_prof_* / linr_debug_poison class (all 24 are taken). */
#define LINR_PLY_TOKEN   1
#define LINR_PLY_COLUMNS 2
#define LINR_PLY_SHORT   4
#define LINR_PLY_RANGE   8
LINR_API size_t linr_ply_parse_ws_bytes(size_t len, int64_t n_rows);
LINR_API int    linr_ply_parse_ascii_device(const char* text_d, size_t len, int64_t n_rows, int32_t n_cols, int32_t cx, int32_t cy,
                                   int32_t cz, int32_t* xyz_d, void* ws_d, size_t ws_bytes, int64_t* status_d, void* stream);
LINR_API int    linr_ply_gather_binary(const uint8_t* rec_d, int64_t n_rows, int32_t stride, const int32_t off[3], const int32_t type[3],
                              int32_t big_endian, int32_t* xyz_d, int64_t* status_d, void* stream);

/* ---- frame output (device) -------------------------------------------------------------------------------------------
 * Body of an ASCII PLY formatted on the DEVICE (csrc/ply_format.hip): what write_ply_ascii (datautils/custom_dataset.py:37-58,
 * called from decoder.py:144-146) hands to np.savetxt(fmt='%d').  xyz [n][3] int32, 4-byte aligned; text receives n lines
 * "%d %d %d\n" back to back - decimal, '-' only for negatives, no leading zeros, one blank between columns - and *text_len (DEVICE
 * int64, 8-byte aligned) their byte count; bytes of text at and past *text_len are not written.  A line is 6 .. 36 bytes
 * (LINR_PLY_FORMAT_MAX_LINE: three times "-2147483648"), byte offsets are 32-bit: n <= LINR_PLY_FORMAT_MAX_ROWS.
 * text_cap >= linr_ply_format_text_bytes(n) = 36 n, the capacity no input can overflow; ws: linr_ply_format_ws_bytes(n) bytes,
 * 256-byte aligned, uninitialised (the n + 1 row offsets and the scan's own scratch).  Both sizes are 0 for n <= 0 and for n over
 * the bound.  Arguments are checked before the first launch: LINR_EINVAL for n < 0, n over the bound or a NULL pointer with n > 0,
 * LINR_ENOSPC for a short text_cap or workspace, LINR_EALIGN for a misaligned xyz, ws or text_len.  n == 0 returns 0, launches
 * nothing and leaves *text_len untouched.  Stream-ordered, nothing allocated; the kernels use no LDS and belong to no
 * linr_prof_* / linr_debug_poison class (all 24 are taken). */
#define LINR_PLY_FORMAT_MAX_LINE 36
#define LINR_PLY_FORMAT_MAX_ROWS (2147483647 / LINR_PLY_FORMAT_MAX_LINE)
LINR_API size_t linr_ply_format_text_bytes(int64_t n);
LINR_API size_t linr_ply_format_ws_bytes(int64_t n);
LINR_API int    linr_ply_format_ascii(const int32_t* xyz_d, int64_t n, char* text_d, size_t text_cap, void* ws_d, size_t ws_bytes,
                             int64_t* text_len_d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LINR_HIP_H */
