"""GPU tests of the wide C forward (csrc/wide_fwd.hip: linr_net_forward_wide / _bf16) and of the decoder scale entries for
hidden_channel_conv 16 / 32 (linr_decode_scale_wide / _batch_wide).  The C schedule makes the Python executor's launches with the
Python executor's arguments, so EVERY comparison here is torch.equal: probabilities and the float64 bits against WideNet.forward /
forward_bf16, decoded coordinates against the stage-wise decoder's and against the truth.  Nothing has a tolerance."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [(16, 1), (16, 2), (16, 4), (32, 1), (32, 2)]
_CACHE = {}


def _shell_info():
    """synthetic.sphere_shell(6, 20) through the dataset's octree: the per-scale inputs (finest first) with the 7-neighbour features."""
    if 'gop' not in _CACHE:
        from linr_pcgc_amd import overfit, synthetic
        _CACHE['gop'] = overfit.Gop(None, [synthetic.sphere_shell(6, 20)], None, 64, 'cuda')
    return _CACHE['gop']


def _scale(s, idx=None):
    return {'coord': s['coord'], 'occ': s['occ'], 'offset_tensor': s['offset_tensor'], 'scale_idx': s['scale_idx'] if idx is None else idx}


def _empty(idx):
    return {'coord': np.zeros((0, 3), np.int32), 'occ': np.zeros((0, 8), np.float32), 'offset_tensor': np.zeros((0, 7), np.float32),
            'scale_idx': idx}


def _level(n):
    """A random sparse cloud of n voxels in a 24^3 box with a random occupancy, as one scale."""
    rng = np.random.default_rng(1000 + n)
    lin = np.sort(rng.choice(24 ** 3, size=n, replace=False))
    c = np.stack([lin // 576, (lin // 24) % 24, lin % 24], axis=1).astype(np.int32)
    return {'coord': torch.from_numpy(c).cuda(), 'occ': torch.from_numpy((rng.random((n, 8)) < 0.4).astype(np.float32)).cuda(),
            'offset_tensor': None, 'scale_idx': n % 3}


def _coded(hidden, block_layers):
    """A wide model off its initialisation, through the model codec at 8 bits: de-quantised fp32 parameters AND their codes."""
    key = ('model', hidden, block_layers)
    if key not in _CACHE:
        from linr_pcgc_amd import overfit
        from linr_pcgc_amd.model_codec import Model_Estimate
        sn = _shell_info().scale_num
        model = overfit.gen_model(sn, 'cuda', seed=8807, block_layers=block_layers, hidden=hidden)
        _CACHE[key] = Model_Estimate().compress_model(model, 8, True, overfit.gen_model(sn, 'cuda', block_layers=block_layers,
                                                                                         hidden=hidden))['new_model']
    return _CACHE[key]


def _python_forward(model, frame, precision):
    """frame_probs on the Python schedule (c_forward off on this executor)."""
    model._wide.c_forward = False
    try:
        return model.frame_probs(frame, precision=precision)
    finally:
        del model._wide.c_forward


def _c_forward(model, frame, precision):
    probs = torch.full((8, frame.rows), float('nan'), device='cuda')
    bits = torch.zeros(1, dtype=torch.float64, device='cuda')
    model._wide.forward_c(frame, probs, bits, precision == 'bf16')
    return probs, bits


def _frames(model):
    info = _shell_info().infos[0]['all_input_info']
    assert len(info) >= 3
    out = [('shell, all scales', model.make_frame([_scale(s) for s in info])),
           ('shell, scales 0 and 2 around an empty one', model.make_frame([_scale(info[0], 0), _empty(1), _scale(info[2], 2)]))]
    for n in (1, 63, 64, 65, 255, 256, 257):          # nbr_ld's multiple of 64, the heads' 256-row partial blocks
        out.append(('%d rows' % n, model.make_frame([_level(n)])))
    return out


# ---- 1. the C forward is the Python executor's, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
@pytest.mark.parametrize('hidden,block_layers', CASES)
def test_c_forward_equals_the_python_executor(pkg, hidden, block_layers, precision):
    model = _coded(hidden, block_layers)
    assert model._wide.c_forward          # the default
    for what, frame in _frames(model):
        want_p, want_b = _python_forward(model, frame, precision)
        got_p, got_b = _c_forward(model, frame, precision)
        assert bool(torch.isfinite(got_p).all()), what
        assert torch.equal(got_p, want_p), what
        assert torch.equal(got_b, want_b), what
        # ... and it is what frame_probs runs by default
        dflt_p, dflt_b = model.frame_probs(frame, precision=precision)
        assert torch.equal(dflt_p, want_p) and torch.equal(dflt_b, want_b), what


# ---- 2. stage ranges on one arena ----------------------------------------------------------------------------------------------------
def _entry(model, frame, precision, arena, nbytes, k0, k1, probs, bits):
    from linr_pcgc_amd import _lib
    L, st = _lib.lib(), _lib.current_stream_handle()
    b = None if bits is None else bits.data_ptr()
    if precision == 'bf16':
        rc = L.linr_net_forward_wide_bf16(frame.cref(), model._qcodes.data_ptr(), float(model._qrange[0]), float(model._qrange[1]),
                                          model.hidden, arena, nbytes, k0, k1, probs.data_ptr(), b, st)
    else:
        rc = L.linr_net_forward_wide(frame.cref(), model.flat_parameters().data_ptr(), model.hidden, arena, nbytes, k0, k1,
                                     probs.data_ptr(), b, st)
    assert rc == 0, rc


def _arena(frame, model, precision):
    from linr_pcgc_amd import _lib
    need = int(_lib.lib().linr_net_wide_arena_bytes(frame.rows, model.hidden, model.block_layers, 1 if precision == 'bf16' else 0))
    t = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device='cuda')
    return t, (t.data_ptr() + 63) & ~63, need


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
@pytest.mark.parametrize('hidden,block_layers', [(16, 2), (32, 1)])
def test_stage_calls_on_one_arena_equal_the_one_shot(pkg, hidden, block_layers, precision):
    model = _coded(hidden, block_layers)
    frame = model.make_frame([_scale(s) for s in _shell_info().infos[0]['all_input_info']])
    one, one_b = _c_forward(model, frame, precision)
    keep, arena, nbytes = _arena(frame, model, precision)
    staged = torch.full_like(one, float('nan'))
    bits = torch.zeros(1, dtype=torch.float64, device='cuda')
    for k in range(8):
        _entry(model, frame, precision, arena, nbytes, k, k + 1, staged, bits)
    assert torch.equal(staged, one)
    # bits added range by range are other roundings than the one-shot's one sum: they are the Python executor's over the same ranges
    py = model._wide.forward_bf16 if precision == 'bf16' else model._wide.forward
    want_p, want_b = torch.empty_like(one), torch.zeros(1, dtype=torch.float64, device='cuda')
    for k in range(8):
        py(frame, k, k + 1, want_p, want_b)
    assert torch.equal(want_p, one) and torch.equal(bits, want_b)
    keep2, arena2, _ = _arena(frame, model, precision)
    staged.fill_(float('nan'))
    bits.zero_()
    want_b.zero_()
    for k0, k1 in ((0, 3), (3, 8)):          # a range split elsewhere
        _entry(model, frame, precision, arena2, nbytes, k0, k1, staged, bits)
        py(frame, k0, k1, want_p, want_b)
    assert torch.equal(staged, one) and torch.equal(bits, want_b)
    one_again = torch.zeros(1, dtype=torch.float64, device='cuda')
    _entry(model, frame, precision, arena2, nbytes, 0, 8, staged, one_again)          # ... and the arena serves the next frame call
    assert torch.equal(staged, one) and torch.equal(one_again, one_b)
    # the arena contract: stage_begin > 0 READS what the (0, ...) call left.  On a fresh arena (0xFF bytes: NaN as fp32 and as bf16)
    # stage 1 is NOT required to match - and an entry that did recompute x_glob there would make it match
    keep3, arena3, _ = _arena(frame, model, precision)
    fresh = torch.zeros_like(one)
    _entry(model, frame, precision, arena3, nbytes, 1, 2, fresh, None)
    torch.cuda.synchronize()
    assert not torch.equal(fresh[1], one[1])
    del keep, keep2, keep3


# ---- 3. one decoder scale ------------------------------------------------------------------------------------------------------------
def _gop_and_streams(clouds, precision, hidden=16, scale_num=None):
    from linr_pcgc_amd import codec, overfit
    gop = overfit.Gop(None, clouds, scale_num, 64, 'cuda')
    gen = lambda seed=None: overfit.gen_model(gop.scale_num, 'cuda', seed=seed, hidden=hidden)
    enc = codec.encode_gop(gen(8807), gen(), gop, 8, precision=precision)
    return gop, gen, enc


def _decoder_model(gen, enc):
    """What decode_gop builds from model.bin and side_info.json."""
    from linr_pcgc_amd.model_codec import Model_Estimate
    side = dict(enc['side_info'])
    side.pop('arith_version', None)
    side['final_bytes'] = enc['model_bin']
    model, _ = Model_Estimate().decompress_model(gen(), side)
    model.inference_precision = side.get('precision', 'f32')
    return model


def _truth(gop, i):
    return torch.as_tensor(gop.infos[i]['ori']).cuda() + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32)


def _stagewise_step(model, lowx, s_idx, enc_bytes):
    from linr_pcgc_amd.module_utils import octree_level_obj
    occ = model.decode({'enc_bytes': enc_bytes, 'coord': lowx, 'offset_tensor': None, 'scale_idx': s_idx})
    return octree_level_obj.upper_layer(lowx, torch.cat(occ, dim=-1))


def _coarsest(enc, i):
    from linr_pcgc_amd import codec
    lows, _ = codec.dec_all_frame_low_xyz(enc['low_enc_bytes'])
    xyz = torch.tensor(lows[i].astype(np.int32), device='cuda')
    return codec.unique_sorted(xyz), max(1, int(xyz.max()).bit_length())


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_decode_scale_on_a_wide_model(pkg, precision):
    from linr_pcgc_amd import _lib, synthetic
    gop, gen, enc = _gop_and_streams([synthetic.sphere_shell(6, 20)], precision)
    model = _decoder_model(gen, enc)
    info = gop.infos[0]['all_input_info']
    streams = list(enc['frames'][0])
    lowx, bits = _coarsest(enc, 0)
    for s_idx in range(len(streams) - 1, -1, -1):
        bits = min(bits + 1, 21)
        got = model.decode_scale(lowx, s_idx, streams[s_idx], bits)
        want = _stagewise_step(model, lowx, s_idx, streams[s_idx])
        assert got.dtype == torch.int32 and torch.equal(got, want.to(torch.int32)), s_idx
        assert torch.equal(got, info[s_idx]['ground_truth'].to(device='cuda', dtype=torch.int32)), s_idx
        last, lowx = lowx, got
    assert torch.equal(lowx + torch.tensor(gop.coord_mins[0], device='cuda', dtype=torch.int32), _truth(gop, 0))
    # no rows: an empty level
    none = model.decode_scale(lowx[:0], 0, streams[0], bits)
    assert tuple(none.shape) == (0, 3)
    # a workspace that is too small: LINR_ENOSPC, and neither the child buffer nor the count is written
    L = _lib.lib()
    n = int(last.shape[0])
    from linr_pcgc_amd.function_utils import unpack_bitstream
    shared, opts, need, keep = model._decode_scale_args(L.linr_decode_scale_wide_ws_bytes, (n,), last, unpack_bitstream(streams[0]), 0, 1)
    keep[0].fill_(-7)
    torch.cuda.synchronize()
    m = ctypes.c_int64(99)
    shared = list(shared)
    shared[7] = need - 256 - 1          # (the size function's answer holds 256 bytes of slack for the caller's alignment)
    rc = L.linr_decode_scale_wide(last.data_ptr(), n, 0, model.scale_num, model.block_layers, bits, *shared, ctypes.byref(m),
                                  ctypes.byref(opts), model.hidden, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -2 and m.value == 0 and bool((keep[0] == -7).all())


# ---- 4. lock step ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_decode_scale_batch_equals_the_per_frame_entry(pkg, precision):
    from linr_pcgc_amd import synthetic
    clouds = [synthetic.sphere_shell(6, 20), synthetic.sphere_shell(6, 9), synthetic.sphere_shell(6, 24)]
    gop, gen, enc = _gop_and_streams(clouds, precision, scale_num=2)
    assert [len(f) for f in enc['frames']] == [2, 2, 2]
    model = _decoder_model(gen, enc)
    lows = [_coarsest(enc, i) for i in range(3)]
    bits = max(b for _, b in lows) + 1
    lows = [c for c, _ in lows]
    assert len({int(c.shape[0]) for c in lows}) == 3
    per_frame = [model.decode_scale(lows[i], 1, enc['frames'][i][1], bits) for i in range(3)]
    got = model.decode_scale_batch(lows, 1, [enc['frames'][i][1] for i in range(3)], n_threads=2)
    for i in range(3):
        assert torch.equal(got[i], per_frame[i]), i
        assert torch.equal(got[i], gop.infos[i]['all_input_info'][1]['ground_truth'].to(device='cuda', dtype=torch.int32)), i
    # the finest scale with frame 1's level EMPTY: its segment has no rows, its streams stay unread
    nxt = [per_frame[0], per_frame[1][:0], per_frame[2]]
    got = model.decode_scale_batch(nxt, 0, [enc['frames'][i][0] for i in range(3)], n_threads=2)
    assert tuple(got[1].shape) == (0, 3)
    for i in (0, 2):
        assert torch.equal(got[i], model.decode_scale(nxt[i], 0, enc['frames'][i][0], bits + 1)), i
        assert torch.equal(got[i] + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32), _truth(gop, i)), i


# ---- 5. the GOP decoder ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_decode_gop_of_a_wide_model_with_workers_and_lockstep(pkg, precision):
    from linr_pcgc_amd import codec, synthetic
    gop, gen, enc = _gop_and_streams([synthetic.sphere_shell(6, 20), synthetic.sphere_shell(6, 22)], precision)
    default = codec.decode_gop(gen(), enc, 'cuda')
    # the old path beside them: model.decode per scale, upper_layer in torch, the stage loop in Python
    model = _decoder_model(gen, enc)
    lows, mins = codec.dec_all_frame_low_xyz(enc['low_enc_bytes'])
    stagewise = [codec.decode_one_frame_stagewise(model, list(enc['frames'][i]), torch.tensor(lows[i].astype(np.int32), device='cuda'))
                 ['dec_coord'] + torch.tensor(mins[i], device='cuda', dtype=torch.int32) for i in range(2)]
    timing = {}
    in_flight = codec.decode_gop(gen(), enc, 'cuda', workers=2)
    lockstep = codec.decode_gop(gen(), enc, 'cuda', lockstep=2, timing=timing)
    assert len(in_flight) == 2 and len(lockstep) == 2
    for i in range(2):
        want = _truth(gop, i)
        for what, got in (('default', default), ('stage-wise', stagewise), ('workers=2', in_flight), ('lockstep=2', lockstep)):
            assert torch.equal(got[i].to(torch.int32), want), (what, i)
    assert timing['lockstep_ws_bytes'] > 0          # the group went through linr_decode_scale_batch_wide


# ---- 6. the options of a scale, at the model level ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_chunked_streams_and_the_device_decoder_through_decode_scale(pkg, precision):
    from linr_pcgc_amd.function_utils import pack_bitstream
    from linr_pcgc_amd.model_core import encode_streams
    model = _coded(16, 1)
    s = _shell_info().infos[0]['all_input_info'][0]          # the finest scale: thousands of rows, many chunks of 64
    frame = model.make_frame([_scale(s)])
    assert frame.rows > 4 * 64
    probs, _ = _c_forward(model, frame, precision)
    p_host = probs.cpu().numpy()
    occ_host = frame.occ.t().contiguous().cpu().numpy().astype(np.uint8)
    coord = s['coord'].to(device='cuda', dtype=torch.int32)
    bits = max(1, int(coord.max()).bit_length()) + 1
    truth = s['ground_truth'].to(device='cuda', dtype=torch.int32)
    model.inference_precision = precision
    try:
        chunked = pack_bitstream(encode_streams([p_host[k] for k in range(8)], [occ_host[k] for k in range(8)], chunk=64))
        assert torch.equal(model.decode_scale(coord, s['scale_idx'], chunked, bits, chunk=64, n_threads=2), truth)
        plain = pack_bitstream(encode_streams([p_host[k] for k in range(8)], [occ_host[k] for k in range(8)]))
        assert torch.equal(model.decode_scale(coord, s['scale_idx'], plain, bits, device_decoder=True), truth)
        assert torch.equal(model.decode_scale(coord, s['scale_idx'], chunked, bits, chunk=64, device_decoder=True), truth)
    finally:
        model.inference_precision = 'f32'


# ---- 7. one multi-tile level -----------------------------------------------------------------------------------------------------------
def test_decode_scale_on_a_multi_tile_level(pkg):
    """The finest level of the 9-bit shell of tests/test_gpu_wide.py (156,985 rows): the convolutions' workgroups walk several tiles."""
    from linr_pcgc_amd import overfit, synthetic
    from linr_pcgc_amd.module_utils import prepare_frame
    fr = prepare_frame(synthetic.sequence_frame({'bitdepth': 9, 'radius': 200, 'thickness': 0.5}, 0), None, 64, device='cuda')
    s = fr['all_input_info'][0]
    n = int(s['coord'].shape[0])
    assert n > 2 * torch.cuda.get_device_properties(0).multi_processor_count * 256
    model = overfit.gen_model(fr['scale_num'], 'cuda', seed=8807, hidden=16)
    enc = model.encode({'coord': s['coord'], 'occ': s['occ'], 'offset_tensor': None, 'scale_idx': 0})['enc_bytes']
    coord = s['coord'].to(torch.int32)
    got = model.decode_scale(coord, 0, enc, 9)
    assert torch.equal(got, _stagewise_step(model, coord, 0, enc).to(torch.int32))
    assert torch.equal(got, fr['ori'].to(torch.int32))


# ---- 8. nothing depends on leftover on-chip state ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
@pytest.mark.parametrize('block_layers', [1, 2, 4])
def test_c_forward_does_not_depend_on_leftover_onchip_state(pkg, block_layers, precision):
    """Width 16 with every launch of the wide and bf16 classes (linr_debug_poison bits 16 and 14; the scale context: 11, 12) behind a
    kernel that fills the LDS and vector registers of all CUs with 0xFFFFFFFF, on an arena of 0xFF bytes: the same bits."""
    from linr_pcgc_amd import _lib
    model = _coded(16, block_layers)
    frame = model.make_frame([_scale(s) for s in _shell_info().infos[0]['all_input_info']])
    clean_p, clean_b = _c_forward(model, frame, precision)
    keep, arena, nbytes = _arena(frame, model, precision)
    dirty_p = torch.full_like(clean_p, float('nan'))
    dirty_b = torch.zeros(1, dtype=torch.float64, device='cuda')
    L = _lib.lib()
    L.linr_debug_poison(0x1FFFF)
    try:
        L.linr_debug_poison_now(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        _entry(model, frame, precision, arena, nbytes, 0, 8, dirty_p, dirty_b)
        torch.cuda.synchronize()
    finally:
        L.linr_debug_poison(0xFFFFFF if os.environ.get('LINR_DEBUG_POISON') else 0)
    assert bool(torch.isfinite(dirty_p).all())
    assert torch.equal(dirty_p, clean_p) and torch.equal(dirty_b, clean_b)
    del keep
