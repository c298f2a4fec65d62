"""ctypes binding of liblinr_hip.so (include/linr_hip.h).  Fails loudly when the library is missing."""
import ctypes
import os

import torch  # noqa: F401  - MUST precede loading liblinr_hip.so: both link libamdhip64.so.7 and the process has to
#                             end up with ONE HIP runtime, the one PyTorch bundles (streams and memory come from it).

_HERE = os.path.dirname(os.path.abspath(__file__))
# LINR_HIP_LIB: another build of the same library (kernel experiments, tools/wgrad_floor_lab.sh); the ABI check below still applies
LIB_PATH = os.environ.get('LINR_HIP_LIB') or os.path.join(_HERE, 'liblinr_hip.so')

LINR_RELU, LINR_ACCUM, LINR_RELU_MASK, LINR_NO_BIAS, LINR_PAD_ROW = 1, 2, 4, 8, 16
LINR_MUL_BF16 = 16          # the wide convolutions' entries only (they take no LINR_PAD_ROW): bf16 products, fp32 sums
LINR_FRAME_OCC_PADDED = 1
LINR_PLY_TOKEN, LINR_PLY_COLUMNS, LINR_PLY_SHORT, LINR_PLY_RANGE = 1, 2, 4, 8
ABI_VERSION = 27

c_i32, c_i64, c_u32, c_f32, c_f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_float, ctypes.c_double
c_ptr, c_size = ctypes.c_void_p, ctypes.c_size_t


class LinrWidePw(ctypes.Structure):
    """linr_wide_pw of include/linr_hip.h: a pointwise layer fused into a wide convolution's epilogue."""
    _fields_ = [('mode', ctypes.c_int32), ('W', ctypes.c_void_p), ('b', ctypes.c_void_p), ('aux_h', ctypes.c_void_p), ('out2_h', ctypes.c_void_p)]


class LinrWideReduce(ctypes.Structure):
    """linr_wide_reduce of include/linr_hip.h: one deferred weight-gradient reduction."""
    _fields_ = [('kind', ctypes.c_int32), ('nblocks', ctypes.c_int32), ('cin', ctypes.c_int32), ('cout', ctypes.c_int32),
                ('ws_ci', ctypes.c_int32), ('ws_co', ctypes.c_int32), ('slab', ctypes.c_void_p), ('gW', ctypes.c_void_p),
                ('gb', ctypes.c_void_p)]


class LinrFrame(ctypes.Structure):
    """struct linr_frame (include/linr_hip.h)."""
    _fields_ = [('rows', c_i64), ('n_scales', c_i32), ('model_scale_num', c_i32), ('block_layers', c_i32),
                ('flags', c_i32), ('row_off_h', c_ptr),
                ('scale_idx_h', c_ptr), ('nbr', c_ptr), ('nbr_ld', c_i64), ('nbr_lo', c_ptr), ('nbr_mask', c_ptr),
                ('offset_feat', c_ptr), ('occ', c_ptr), ('nbr8t', c_ptr)]


class LinrInceptionParams(ctypes.Structure):
    """struct linr_inception_params (include/linr_hip.h)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ('w00', 'b00', 'w01', 'b01', 'w10', 'b10', 'w11', 'b11', 'w12', 'b12')]


class LinrRcDecEntry(ctypes.Structure):
    """struct linr_rc_dec_entry (include/linr_hip.h): one entry of linr_rc_decode_probs; five int64, so an int64 [n, 5] array is a table."""
    _fields_ = [(n, c_i64) for n in ('p_off', 'n', 'in_off', 'in_len', 'out_row')]


class LinrRcStream(ctypes.Structure):
    """struct linr_rc_stream (include/linr_hip.h): one stream of linr_rc_encode_codes; five int64, so an int64 [n, 5] array is a table."""
    _fields_ = [(n, c_i64) for n in ('c1_off', 'sym_off', 'n', 'out_off', 'cap')]


class LinrDecodeOpts(ctypes.Structure):
    """struct linr_decode_opts (include/linr_hip.h): the options of a decoder scale; NULL in its place means (0, 1, 0)."""
    _fields_ = [('chunk_symbols', c_i64), ('n_threads', c_i32), ('device', c_i32)]


class LinrStepArgs(ctypes.Structure):
    """struct linr_step_args (include/linr_hip.h): what one overfit iteration takes beyond frame, parameters, arena and stream."""
    _fields_ = [('gscale', c_f32), ('exp_avg', c_ptr), ('exp_avg_sq', c_ptr), ('lr', c_f64), ('step', c_i64), ('scale_steps_h', c_ptr),
                ('beta1', c_f64), ('beta2', c_f64), ('eps', c_f64), ('weight_decay', c_f64), ('bits_acc', c_ptr), ('qparams', c_ptr),
                ('bitdepth', c_i32)]


class LinrOverfitFrame(ctypes.Structure):
    """struct linr_overfit_frame (include/linr_hip.h): one frame of linr_overfit_gop."""
    _fields_ = [('f', ctypes.POINTER(LinrFrame)), ('point_num', c_f64), ('occ_bf16', c_ptr)]


class LinrOverfitArgs(ctypes.Structure):
    """struct linr_overfit_args (include/linr_hip.h)."""
    _fields_ = [('executor', c_i32), ('hidden', c_i32), ('flags', c_u32), ('n_frames', c_i32), ('params', c_ptr), ('exp_avg', c_ptr),
                ('exp_avg_sq', c_ptr), ('beta1', c_f64), ('beta2', c_f64), ('eps', c_f64), ('weight_decay', c_f64), ('lr', c_f64),
                ('min_lr', c_f64), ('gamma', c_f64), ('step_size', c_i64), ('step', c_i64), ('sched_steps', c_i64), ('scale_steps_h', c_ptr),
                ('epochs', c_i32), ('keep_best', c_i32), ('qat_from', c_i32), ('bitdepth', c_i32), ('qparams', c_ptr), ('arena', c_ptr),
                ('arena_bytes', c_size), ('ws', c_ptr), ('ws_bytes', c_size)]


class LinrOverfitResult(ctypes.Structure):
    """struct linr_overfit_result (include/linr_hip.h)."""
    _fields_ = [('losses_h', c_ptr), ('best_epoch', c_i32), ('best_loss', c_f64), ('step', c_i64), ('sched_steps', c_i64), ('lr', c_f64),
                ('scale_steps_h', c_ptr)]


class LinrOverfitAvg(ctypes.Structure):
    """struct linr_overfit_avg (include/linr_hip.h): the averages linr_overfit_gop_avg keeps beside the training."""
    _fields_ = [('n_avg', c_i32), ('weight', c_f32 * 4), ('avg', c_ptr), ('stride', c_i64)]


LINR_OVERFIT_F32, LINR_OVERFIT_BF16, LINR_OVERFIT_WIDE = 0, 1, 2
LINR_AVG_MAX = 4            # rows of linr_params_average / linr_overfit_avg

_PROTOS = {
    'linr_abi_version': (ctypes.c_int, []),
    'linr_param_count': (c_i64, [c_i32, c_i32]),
    'linr_kmap_workspace_bytes': (c_size, [c_i64]),
    'linr_kmap_build': (ctypes.c_int, [c_ptr, c_i64, c_ptr, c_i64, c_i64, c_ptr, c_size, c_ptr]),
    'linr_kmap_validate': (ctypes.c_int, [c_ptr, c_i64, c_ptr, c_ptr]),
    'linr_spconv_wgrad_cmap_blocks': (ctypes.c_int64, []),
    'linr_spconv_wgrad_cmap': (ctypes.c_int, [c_ptr, c_i32, c_ptr, c_i32, c_ptr, c_ptr, c_i64, c_i64, c_i32, c_i32, c_ptr, c_ptr]),
    'linr_spconv_bwd_fused': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_i32, c_ptr]),
    'linr_inception_bwd_fused': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64,
                                                ctypes.POINTER(LinrInceptionParams), c_ptr, c_ptr, c_u32, c_ptr, c_i32, c_ptr]),
    'linr_slab_reduce': (ctypes.c_int, [c_ptr, c_i32, c_i32, c_i32, c_ptr, c_ptr, c_u32, c_ptr]),
    'linr_axpy': (ctypes.c_int, [c_ptr, c_i64, c_ptr, c_i32, c_ptr]),
    'linr_sum_many': (ctypes.c_int, [c_ptr, c_i32, c_i64, c_ptr, c_i32, c_ptr]),
    'linr_occ_wgrad7': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_i32, c_ptr, c_ptr]),
    'linr_kmap_tile8t_bytes': (c_size, [c_i64]),
    'linr_kmap_tile8t': (ctypes.c_int, [c_ptr, c_i64, c_i64, c_ptr, c_size, c_ptr]),
    'linr_prof_mask': (ctypes.c_int, [c_u32]),
    'linr_prof_enable': (ctypes.c_int, [c_i32]),
    'linr_debug_poison': (ctypes.c_int, [c_u32]),
    'linr_debug_poison_now': (ctypes.c_int, [c_ptr]),
    'linr_prof_read': (ctypes.c_int, [c_i32, c_ptr, c_ptr, c_ptr]),
    'linr_octree_occupancy': (ctypes.c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, ctypes.c_size_t, c_ptr]),
    'linr_sort_unique_workspace_bytes': (ctypes.c_size_t, [c_i64]),
    'linr_coords_sort_unique': (ctypes.c_int, [c_ptr, c_i64, c_ptr, c_i32, c_i32, c_ptr, c_ptr, c_ptr, ctypes.c_size_t, c_ptr]),
    'linr_coords_minmax': (ctypes.c_int, [c_ptr, c_i64, c_ptr, c_ptr]),
    'linr_octree_level': (ctypes.c_int, [c_ptr, c_i64, c_i32, c_ptr, c_ptr, c_ptr, c_ptr, ctypes.c_size_t, c_ptr]),
    'linr_octree_levels_count': (c_i32, [c_i32, c_i32]),
    'linr_octree_levels_rows': (c_i64, [c_i64, c_i32, c_i32]),
    'linr_octree_levels_workspace_bytes': (ctypes.c_size_t, [c_i64, c_i32, c_i32]),
    'linr_octree_levels': (ctypes.c_int, [c_ptr, c_i64, c_ptr, c_i32, c_i32, c_ptr, c_ptr, c_ptr, c_ptr, ctypes.c_size_t, c_ptr]),
    'linr_kmap_offset_feat': (ctypes.c_int, [c_ptr, c_i64, c_i64, c_i64, c_ptr, c_ptr]),
    'linr_kmap_compress': (ctypes.c_int, [c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_i64, c_ptr]),
    'linr_spconv_fwd': (ctypes.c_int, [c_ptr, c_i32, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_i32, c_i32, c_ptr, c_i32,
                                       c_ptr, c_i32, c_u32, c_ptr]),
    'linr_spconv_bwd_data': (ctypes.c_int, [c_ptr, c_i32, c_ptr, c_i64, c_i64, c_ptr, c_i32, c_i32, c_ptr, c_i32,
                                            c_ptr, c_i32, c_u32, c_ptr]),
    'linr_spconv_wide': (ctypes.c_int, [c_i32, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_i32, c_i32, c_ptr, c_ptr, c_ptr, c_u32,
                                        ctypes.POINTER(LinrWidePw), c_ptr]),
    'linr_spconv_wgrad_wide_slab_bytes': (ctypes.c_size_t, [c_i32, c_i32]),
    'linr_spconv_wgrad_wide': (ctypes.c_int, [c_ptr, c_i32, c_ptr, c_i32, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_u32, c_ptr]),
    'linr_linear_wide': (ctypes.c_int, [c_ptr, ctypes.c_int32, ctypes.c_int32, c_ptr, ctypes.c_int32, ctypes.c_int32, c_ptr, ctypes.c_int32,
                                        ctypes.c_int32, c_ptr, c_ptr, c_ptr, c_i64, ctypes.c_uint32, c_ptr]),
    'linr_spconv_wgrad_wide2': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i32, c_ptr, c_i64, c_ptr, c_u32, c_ptr]),
    'linr_spconv_wgrad_wide_blocks': (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32]),
    'linr_linear_wgrad_wide_blocks': (ctypes.c_int32, [c_i64]),
    'linr_wide_reduce_many': (ctypes.c_int, [ctypes.POINTER(LinrWideReduce), ctypes.c_int32, c_ptr]),
    'linr_head_wide_workspace_bytes': (ctypes.c_size_t, [c_i64]),
    'linr_bits_finish': (ctypes.c_int, [c_ptr, c_i64, c_ptr, c_ptr]),
    'linr_head_wide_fwd': (ctypes.c_int, [c_ptr, ctypes.c_int32, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, ctypes.c_int32, c_i64, c_ptr, c_ptr, c_ptr,
                                          ctypes.c_size_t, c_ptr]),
    'linr_head_wide_bwd_slab_bytes': (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32]),
    'linr_head_wide_bwd': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, ctypes.c_int32, c_ptr, c_ptr, c_ptr, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.c_float, c_ptr, c_i64, c_ptr, ctypes.c_size_t, c_ptr, c_ptr]),
    'linr_linear_wgrad_wide_workspace_bytes': (ctypes.c_size_t, [c_i64, ctypes.c_int32, ctypes.c_int32]),
    'linr_linear_wgrad_wide': (ctypes.c_int, [c_ptr, ctypes.c_int32, ctypes.c_int32, c_ptr, ctypes.c_int32, ctypes.c_int32, c_i64, c_ptr,
                                              ctypes.c_int32, ctypes.c_int32, c_ptr, ctypes.c_uint32, c_ptr, ctypes.c_size_t, c_ptr]),
    'linr_spconv_cmap': (ctypes.c_int, [c_i32, c_ptr, c_i32, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_i32, c_i32, c_ptr,
                                        c_i32, c_ptr, c_i32, c_ptr, c_i32, c_u32, c_ptr]),
    'linr_spconv_bwd_weight_workspace_bytes': (c_size, [c_i64, c_i32, c_i32]),
    'linr_spconv_bwd_weight': (ctypes.c_int, [c_ptr, c_i32, c_ptr, c_i32, c_ptr, c_i64, c_i64, c_i32, c_i32, c_ptr,
                                              c_ptr, c_u32, c_ptr, c_size, c_ptr]),
    'linr_linear_fwd': (ctypes.c_int, [c_ptr, c_i32, c_i64, c_ptr, c_i32, c_i32, c_ptr, c_i32, c_i32, c_ptr, c_i32,
                                       c_ptr, c_i32, c_u32, c_ptr]),
    'linr_linear_bwd_data': (ctypes.c_int, [c_ptr, c_i32, c_i64, c_ptr, c_i32, c_i32, c_i32, c_i32, c_ptr, c_i32,
                                            c_ptr, c_i32, c_u32, c_ptr]),
    'linr_linear_bwd_weight_workspace_bytes': (c_size, [c_i64, c_i32, c_i32]),
    'linr_linear_bwd_weight': (ctypes.c_int, [c_ptr, c_i32, c_ptr, c_i32, c_i64, c_i32, c_i32, c_ptr, c_i32, c_i32,
                                              c_ptr, c_u32, c_ptr, c_size, c_ptr]),
    'linr_bce_workspace_bytes': (c_size, [c_i64]),
    'linr_bce_bits_fwd': (ctypes.c_int, [c_ptr, c_ptr, c_i32, c_i64, c_ptr, c_ptr, c_ptr, c_size, c_ptr]),
    'linr_bce_bits_bwd': (ctypes.c_int, [c_ptr, c_ptr, c_i32, c_i64, c_f32, c_ptr, c_ptr]),
    'linr_adam_step': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_f64, c_f64, c_f64, c_f64, c_f64, c_f64,
                                      c_ptr]),
    'linr_net_arena_bytes': (c_size, [c_i64, c_i32]),
    'linr_net_forward': (ctypes.c_int, [ctypes.POINTER(LinrFrame), c_ptr, c_ptr, c_size, c_i32, c_i32, c_ptr, c_ptr,
                                        c_ptr]),
    'linr_net_backward': (ctypes.c_int, [ctypes.POINTER(LinrFrame), c_ptr, c_ptr, c_size, c_f32, c_ptr, c_ptr]),
    'linr_net_train_step': (ctypes.c_int, [ctypes.POINTER(LinrFrame), c_ptr, c_ptr, c_size, ctypes.POINTER(LinrStepArgs), c_ptr]),
    'linr_net_bf16_arena_bytes': (c_size, [c_i64, c_i32]),
    'linr_net_forward_bf16': (ctypes.c_int, [ctypes.POINTER(LinrFrame), c_ptr, c_f32, c_f32, c_ptr, c_size, c_i32, c_i32, c_ptr,
                                             c_ptr, c_ptr]),
    'linr_wide_bf16_image_elems': (ctypes.c_int64, [c_i32, c_i32]),
    'linr_wide_bf16_prep': (ctypes.c_int, [c_ptr, c_i64, c_f32, c_f32, c_ptr, c_i32, c_i64, c_ptr, c_ptr, c_ptr]),
    'linr_spconv_wide_bf16': (ctypes.c_int, [c_i32, c_ptr, c_i64, c_i32, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_i32, c_ptr, c_i64,
                                             c_ptr, c_i64, c_ptr, c_ptr, c_i32, c_ptr, c_i64, c_ptr]),
    'linr_head_wide_bf16_fwd': (ctypes.c_int, [c_ptr, c_i64, c_i32, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                               c_ptr, c_i32, c_ptr, c_ptr, c_ptr]),
    'linr_sce_fwd_bf16': (ctypes.c_int, [c_ptr, ctypes.POINTER(LinrFrame), c_ptr, c_ptr]),
    'linr_param_count_wide': (c_i64, [c_i32, c_i32, c_i32]),
    'linr_net_wide_arena_bytes': (c_size, [c_i64, c_i32, c_i32, c_i32]),
    'linr_net_forward_wide': (ctypes.c_int, [ctypes.POINTER(LinrFrame), c_ptr, c_i32, c_ptr, c_size, c_i32, c_i32, c_ptr, c_ptr, c_ptr]),
    'linr_net_forward_wide_bf16': (ctypes.c_int, [ctypes.POINTER(LinrFrame), c_ptr, c_f32, c_f32, c_i32, c_ptr, c_size, c_i32, c_i32, c_ptr,
                                                  c_ptr, c_ptr]),
    'linr_net_wide_train_arena_bytes': (c_size, [c_i64, c_i32, c_i32]),
    'linr_net_forward_train_wide': (ctypes.c_int, [ctypes.POINTER(LinrFrame), c_ptr, c_i32, c_ptr, c_size, c_u32, c_ptr, c_ptr]),
    'linr_net_backward_wide': (ctypes.c_int, [ctypes.POINTER(LinrFrame), c_ptr, c_i32, c_ptr, c_size, c_u32, c_f32, c_ptr, c_ptr]),
    'linr_net_train_step_wide': (ctypes.c_int, [ctypes.POINTER(LinrFrame), c_ptr, c_i32, c_ptr, c_size, c_u32, ctypes.POINTER(LinrStepArgs),
                                                c_ptr]),
    'linr_net_train_bf16_arena_bytes': (c_size, [c_i64, c_i32]),
    'linr_occ_to_bf16': (ctypes.c_int, [c_ptr, c_i64, c_ptr, c_ptr]),
    'linr_net_forward_train_bf16': (ctypes.c_int, [ctypes.POINTER(LinrFrame), c_ptr, c_ptr, c_size, c_ptr, c_ptr, c_ptr, c_ptr]),
    'linr_net_backward_bf16': (ctypes.c_int, [ctypes.POINTER(LinrFrame), c_ptr, c_ptr, c_size, c_ptr, c_f32, c_ptr, c_ptr]),
    'linr_net_train_step_bf16': (ctypes.c_int, [ctypes.POINTER(LinrFrame), c_ptr, c_ptr, c_size, c_ptr, ctypes.POINTER(LinrStepArgs),
                                                c_ptr]),
    'linr_spconv_bwd_fused_bf16': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_i32, c_ptr, c_ptr]),
    'linr_sce_fwd': (ctypes.c_int, [c_ptr, ctypes.POINTER(LinrFrame), c_ptr, c_ptr, c_ptr, c_ptr]),
    'linr_sce_bwd': (ctypes.c_int, [c_ptr, ctypes.POINTER(LinrFrame), c_ptr, c_ptr, c_ptr, c_ptr]),
    'linr_sce_param_count': (ctypes.c_int64, [ctypes.c_int32]),
    'linr_sce_bwd_params_slab_bytes': (ctypes.c_size_t, [ctypes.c_int32]),
    'linr_sce_bwd_params': (ctypes.c_int, [c_ptr, ctypes.POINTER(LinrFrame), c_ptr, c_ptr, c_ptr, ctypes.c_size_t, c_ptr, c_ptr]),
    'linr_head_workspace_bytes': (c_size, [c_i64]),
    'linr_head_fwd': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i32,
                                     c_ptr, c_ptr, c_ptr, c_ptr, c_size, c_ptr]),
    'linr_head_bwd': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_i32, c_ptr, c_ptr, c_ptr, c_f32, c_ptr, c_i64, c_ptr, c_ptr, c_size,
                                     c_ptr]),
    'linr_inception_fwd': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_i64, ctypes.POINTER(LinrInceptionParams), c_ptr, c_ptr,
                                          c_ptr, c_ptr]),
    'linr_inception_bwd_data': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64,
                                               ctypes.POINTER(LinrInceptionParams), c_ptr, c_ptr, c_ptr, c_u32, c_ptr]),
    'linr_spconv_wgrad_dual44': (ctypes.c_int, [c_ptr, c_ptr, c_i32, c_ptr, c_i32, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr]),
    'linr_occ_conv7': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    'linr_ac_encode_binary': (c_i64, [c_ptr, c_ptr, c_i64, c_ptr, c_i64]),
    'linr_ac_decode_binary': (ctypes.c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr]),
    'linr_net_decode_stages': (ctypes.c_int, [ctypes.POINTER(LinrFrame), c_ptr, c_ptr, c_f32, c_f32, c_ptr, c_size, c_ptr, c_ptr, c_ptr,
                                              c_ptr, c_ptr, c_ptr, c_ptr]),
    'linr_decode_scale_ws_bytes': (c_size, [c_i64, c_i32, c_i32, c_i64, c_i64]),
    'linr_decode_scale': (ctypes.c_int, [c_ptr, c_i64, c_i32, c_i32, c_i32, c_i32, c_ptr, c_ptr, c_f32, c_f32, c_ptr, c_ptr, c_ptr, c_size,
                                         c_ptr, c_ptr, c_ptr, c_i64, c_ptr, ctypes.POINTER(LinrDecodeOpts), c_ptr]),
    'linr_kmap_build_segments': (ctypes.c_int, [c_ptr, c_ptr, c_i32, c_ptr, c_i64, c_ptr, c_size, c_ptr]),
    'linr_children_segments_ws_bytes': (c_size, [c_i64]),
    'linr_children_segments': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_i32, c_ptr, c_i64, c_ptr, c_ptr, c_size, c_ptr]),
    'linr_decode_scale_batch_ws_bytes': (c_size, [c_i64, c_i32, c_i32, c_i32, c_i64, c_i64]),
    'linr_decode_scale_batch': (ctypes.c_int, [c_ptr, c_ptr, c_i32, c_i32, c_i32, c_i32, c_ptr, c_ptr, c_f32, c_f32, c_ptr, c_ptr, c_ptr,
                                               c_size, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, ctypes.POINTER(LinrDecodeOpts), c_ptr]),
    'linr_decode_scale_wide_ws_bytes': (c_size, [c_i64, c_i32, c_i32, c_i64, c_i64, c_i32]),
    'linr_decode_scale_wide': (ctypes.c_int, [c_ptr, c_i64, c_i32, c_i32, c_i32, c_i32, c_ptr, c_ptr, c_f32, c_f32, c_ptr, c_ptr, c_ptr, c_size,
                                              c_ptr, c_ptr, c_ptr, c_i64, c_ptr, ctypes.POINTER(LinrDecodeOpts), c_i32, c_ptr]),
    'linr_decode_scale_batch_wide_ws_bytes': (c_size, [c_i64, c_i32, c_i32, c_i32, c_i64, c_i64, c_i32]),
    'linr_decode_scale_batch_wide': (ctypes.c_int, [c_ptr, c_ptr, c_i32, c_i32, c_i32, c_i32, c_ptr, c_ptr, c_f32, c_f32, c_ptr, c_ptr, c_ptr,
                                                    c_size, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, ctypes.POINTER(LinrDecodeOpts), c_i32, c_ptr]),
    'linr_ac_decode_binary_twin':(ctypes.c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr]),
    'linr_rc_decode_ws_bytes': (c_size, [c_i32]),
    'linr_rc_decode_probs': (ctypes.c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i32, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_size, c_ptr]),
    'linr_ac_decode_binary_batch': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i32, c_ptr, c_i32]),
    'linr_stream_chunk_count': (c_i64, [c_i64, c_i64]),
    'linr_stream_split_chunks': (c_i64, [c_ptr, c_i64, c_i64, c_i64, c_ptr, c_ptr, c_i64]),
    'linr_ac_encode_cdf16': (c_i64, [c_ptr, c_i32, c_i32, c_ptr, c_i64, c_ptr, c_i64]),
    'linr_ac_decode_cdf16': (ctypes.c_int, [c_ptr, c_i32, c_i32, c_i64, c_ptr, c_i64, c_ptr]),
    'linr_ply_parse_ascii': (ctypes.c_int, [c_ptr, c_size, c_i64, c_i32, c_i32, c_i32, c_i32, c_ptr, c_ptr]),
    'linr_ac_encode_binary_batch': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_i32, c_ptr, c_ptr, c_ptr, c_i32]),
    'linr_ac_encode_binary_codes': (c_i64, [c_ptr, c_ptr, c_i64, c_ptr, c_i64]),
    'linr_ac_decode_binary_codes': (ctypes.c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr]),
    'linr_ac_encode_binary_codes_batch': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_i32, c_ptr, c_ptr, c_ptr, c_i32]),
    'linr_ac_codes_sym_words': (c_size, [c_i64]),
    'linr_ac_codes': (ctypes.c_int, [c_ptr, c_i64, c_ptr, c_i32, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_ptr]),
    'linr_rc_encode_ws_bytes': (c_size, [c_i32, c_i64]),
    'linr_rc_encode_codes': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_i32, c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_size, c_ptr]),
    'linr_rc_encode_chunked_ws_bytes': (c_size, [c_i32, c_i64]),
    'linr_rc_encode_codes_chunked': (ctypes.c_int, [c_ptr, c_ptr, c_ptr, c_i32, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_size,
                                                    c_ptr]),
    'linr_ply_format_text_bytes': (c_size, [c_i64]),
    'linr_ply_format_ws_bytes': (c_size, [c_i64]),
    'linr_ply_format_ascii': (ctypes.c_int, [c_ptr, c_i64, c_ptr, c_size, c_ptr, c_size, c_ptr, c_ptr]),
    'linr_ply_parse_ws_bytes': (c_size, [c_size, c_i64]),
    'linr_ply_parse_ascii_device': (ctypes.c_int, [c_ptr, c_size, c_i64, c_i32, c_i32, c_i32, c_i32, c_ptr, c_ptr, c_size, c_ptr, c_ptr]),
    'linr_ply_gather_binary': (ctypes.c_int, [c_ptr, c_i64, c_i32, c_ptr, c_ptr, c_i32, c_ptr, c_ptr, c_ptr]),
    'linr_params_fake_quant': (ctypes.c_int, [c_ptr, c_i64, c_i32, c_ptr, c_ptr, c_ptr, c_ptr]),
    'linr_params_fake_quant_host': (ctypes.c_int, [c_ptr, c_i64, c_i32, c_ptr, c_ptr, c_ptr]),
    'linr_params_fake_quant_ranges': (ctypes.c_int, [c_ptr, c_i64, c_i32, c_ptr, c_i32, c_i64, c_ptr, c_ptr, c_ptr, c_ptr]),
    'linr_params_fake_quant_ranges_host': (ctypes.c_int, [c_ptr, c_i64, c_i32, c_ptr, c_i32, c_i64, c_ptr, c_ptr, c_ptr]),
    'linr_overfit_plan': (ctypes.c_int, [c_ptr, c_i32, c_i32, c_i32, c_i64, c_i64, c_f64, c_ptr, c_i64, c_f64, c_f64, c_ptr, c_ptr, c_ptr,
                                         c_ptr, c_ptr, c_ptr, c_ptr]),
    'linr_overfit_ws_bytes': (c_size, [c_i64, c_i32, c_i32]),
    'linr_overfit_gop': (ctypes.c_int, [ctypes.POINTER(LinrOverfitFrame), ctypes.POINTER(LinrOverfitArgs), ctypes.POINTER(LinrOverfitResult),
                                        c_ptr]),
    'linr_params_average': (ctypes.c_int, [c_ptr, c_i64, c_ptr, c_i32, c_i64, c_ptr, c_ptr]),
    'linr_params_average_host': (ctypes.c_int, [c_ptr, c_i64, c_ptr, c_i32, c_i64, c_ptr]),
    'linr_overfit_gop_avg': (ctypes.c_int, [ctypes.POINTER(LinrOverfitFrame), ctypes.POINTER(LinrOverfitArgs), ctypes.POINTER(LinrOverfitAvg),
                                            ctypes.POINTER(LinrOverfitResult), c_ptr]),
    'linr_coords_digest_ws_bytes': (c_size, [c_i32]),
    'linr_coords_digest_segments': (ctypes.c_int, [c_ptr, c_ptr, c_i32, c_ptr, c_ptr, c_ptr, c_size, c_ptr]),
    'linr_coords_digest_host': (ctypes.c_uint64, [c_ptr, c_i64, c_ptr]),
}

EXPORTS = tuple(_PROTOS)
_lib = None


class LinrError(RuntimeError):
    pass


class LinrDigestError(LinrError):
    """A decoded octree level does not have the digest its GOP carries (bins/digests.bin; codec.decode_gop verify=True).
    frame: the frame's index in the GOP; scale: the scale whose children differ; want: the stream's value; got: the value of what was
    decoded (both D >> 32 of stream_digests.py)."""

    def __init__(self, frame, scale, want, got):
        self.frame, self.scale, self.want, self.got = int(frame), int(scale), int(want), int(got)
        super().__init__('frame %d, scale %d: the decoded level has digest %08x, the stream records %08x.  This usually means that '
                         'the stream was encoded by another build of the library or on another GPU than this decoder runs on (the '
                         'probabilities must be reproduced bit for bit), or that one of the GOP\'s files is damaged'
                         % (self.frame, self.scale, self.got, self.want))


def lib():
    """The loaded library.  Raises (never falls back) when liblinr_hip.so has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LinrError('%s not found: build it with linr_pcgc_amd/csrc/build.sh (or __graft_entry__.build()); '
                            'there is no CPU / PyTorch fallback for the coding network' % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(handle, name)          # AttributeError if an export is missing
            fn.restype, fn.argtypes = res, args
        if handle.linr_abi_version() != ABI_VERSION:
            raise LinrError('liblinr_hip.so ABI %d != binding ABI %d' % (handle.linr_abi_version(), ABI_VERSION))
        if os.environ.get('LINR_DEBUG_POISON'):
            handle = _Poisoned(handle)
        _lib = handle
    return _lib


class _Poisoned:
    """LINR_DEBUG_POISON=1 (test aid, tools/README.md): every GPU entry point is called with the LDS and vector registers of all
    CUs freshly filled with a NaN pattern (linr_debug_poison_now in front of it, linr_debug_poison(all classes) for the launches
    inside the executors).  The test suite must pass unchanged under it: no kernel may read on-chip state it did not write."""
    _HOST = ('linr_ac_', 'linr_stream_', 'linr_prof_', 'linr_debug_', 'linr_abi_version', 'linr_params_fake_quant_host',
             'linr_params_fake_quant_ranges_host', 'linr_overfit_plan', 'linr_coords_digest_host', 'linr_params_average_host')

    def __init__(self, handle):
        self._h = handle
        handle.linr_debug_poison(0xFFFFFF)

    def __getattr__(self, name):
        fn = getattr(self._h, name)
        if name.startswith(self._HOST) or name.endswith('_bytes'):
            return fn
        h = self._h

        def call(*a):
            import torch
            if torch.cuda.is_available():
                h.linr_debug_poison_now(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            return fn(*a)
        return call


_ERR = {-1: 'LINR_EINVAL (bad argument)', -2: 'LINR_ENOSPC (buffer too small)', -3: 'LINR_EALIGN (misaligned pointer)'}


def check(rc, what):
    """The reference's only error convention is Python assert/ValueError (encoder.py:86-87); we raise RuntimeError."""
    if rc != 0:
        raise LinrError('%s failed: %s' % (what, _ERR.get(rc, 'hipError_t %d' % rc)))


def scratch(nbytes, device):
    """Uninitialised device scratch (arenas, workspaces, slabs) that the library must initialise itself wherever it reads it.
    Under LINR_DEBUG_POISON it comes filled with 0xFF bytes (NaN as float, -1 as int) instead of whatever the allocator returns -
    mostly zeros from a fresh process, which is exactly what hides a missing initialisation."""
    import torch
    t = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    if os.environ.get('LINR_DEBUG_POISON'):
        t.fill_(0xFF)
    return t


def current_stream_handle():
    """The raw handle of PyTorch's current HIP stream on the current device.  torch.cuda.current_stream() builds a Stream object through
    several Python layers (~9 us per call; a frame's staging makes twenty such calls): the two C entry points below are what it ends in."""
    try:
        return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
    except AttributeError:                                         # (a torch build without them)
        return torch.cuda.current_stream().cuda_stream
