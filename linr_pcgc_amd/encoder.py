"""encoder.py of the reference (encode / encode_one_gop / encode_one_frame, encoder.py:13-176) with its argument dicts, on the
HIP-backed model: a checkpoint per GOP in, ``<encode_dir>/<gop>/bins/{frameXXXX_scaleY.bin, model.bin, low_enc_bytes.bin}`` +
``side_info.json`` out.  This is the reference-shaped road (one model.encode call per scale and frame); ``codec.encode_gop`` is
the batched, pipelined one the sequence driver uses - both write the same files.

One deliberate difference: the reference builds a GOP's frame window as ``range(first, last)`` (encoder.py:47), which drops the
last frame and fails on a one-frame GOP; the window here is inclusive, like the GOP names.
"""
import json
import os

import torch

from .custom_dataset import Read_Data_with_cache
from .model_codec import Model_Estimate
from .test_utils import enc_all_frame_low_xyz, write_bin_file
from . import codec, stream_digests
from .stream_chunks import SIDE_BITS, check_chunk


def gop_bounds(gop_name):
    first, last = (int(d) for d in gop_name.replace('gop_', '').split('_'))
    return first, last


def encode(enc_args):
    """encoder.py:20-54.  enc_args: 'outputdir' (holds <gop>/model.pth), 'gop_names', 'Gen_Model', 'dataset', 'encode_dir'; optional
    'qrange_search' (default off), 'qrange_trims', 'qrange_frames': the rate-checked quantiser range of codec.encode_gop; optional
    'stream_chunk' (default 0 = off): its chunked stage streams; optional 'digests' (default off): its per-scale geometry digests
    (bins/digests.bin, stream_digests.py).  The averaged weights of codec.encode_gop(avg=) are not offered here: a checkpoint carries
    the kept epoch's parameters and no averages of the iterates, so this road always codes the model's own parameters."""
    os.makedirs(enc_args['encode_dir'], exist_ok=True)
    for gop_name in enc_args['gop_names']:
        first, last = gop_bounds(gop_name)
        reading = Read_Data_with_cache(enc_args['dataset'], list(range(first, last + 1)))
        encode_one_gop({'Gen_Model': enc_args['Gen_Model'], 'frame_num': last - first + 1,
                        'model_path': os.path.join(enc_args['outputdir'], gop_name, 'model.pth'),
                        'result_dir': os.path.join(enc_args['encode_dir'], gop_name), 'reading_data': reading,
                        'low_enc_bytes': enc_all_frame_low_xyz(reading, last - first + 1),
                        **{k: enc_args[k] for k in ('qrange_search', 'qrange_trims', 'qrange_frames', 'stream_chunk', 'digests') if k in enc_args}})


def encode_one_frame(model, all_inargs, ori=None, stream_chunk=0):
    """encoder.py:158-176: model.encode on every scale of a frame (stream_chunk: codec.encode_gop's, handed to model.encode)."""
    all_bit, all_bytes = 0, []
    for inargs in all_inargs:
        putin = dict(inargs)
        qsc = inargs['xyzqsc_t']
        putin['coord'], putin['offset_tensor'] = qsc.get_coord(), qsc.get_offset_tensor()
        if stream_chunk:
            putin['stream_chunk'] = stream_chunk
        ret = model.encode(putin)
        all_bit += ret['bits']
        all_bytes.append(ret['enc_bytes'])
    return {'all_bit': all_bit, 'all_bytes': all_bytes}


def encode_one_gop(inargs):
    """encoder.py:57-156.  Returns {'bpp_all', 'point_bpp', 'model_bpp', 'xyzlow_bpp'} (test_utils.py:146-157's accounting; the
    two extra side-info fields of this codec counted with the model).  inargs['stream_chunk'] = S > 0: the chunked stage streams of
    codec.encode_gop (side_info's 'stream_chunk', 32 bits more with the model; hidden_channel_conv 8 only).  inargs['digests'] true:
    its per-scale geometry digests (codec.gop_digests_launch on the reading data: bins/digests.bin and side_info's 'digests',
    8 * len(digests.bin) + 8 bits more with the model, returned as 'digest_bits' too)."""
    low = inargs.get('low_enc_bytes')
    if low is None:
        raise ValueError('low_enc_bytes is None')
    stream_chunk = check_chunk(inargs.get('stream_chunk', 0))
    gen = inargs['Gen_Model']
    ckpt = torch.load(inargs['model_path'], map_location='cpu', weights_only=False)
    trained = gen()
    trained.load_state_dict(ckpt['model'])
    if stream_chunk and getattr(trained, '_wide', None) is not None:
        raise ValueError('stream_chunk needs hidden_channel_conv 8: the widths 16 and 32 decode stage-wise in Python, without chunks')
    bitdepth = ckpt.get('bitdepth') or 8
    result_dir = inargs['result_dir']
    bins_dir = os.path.join(result_dir, 'bins')
    os.makedirs(bins_dir, exist_ok=True)
    with open(os.path.join(bins_dir, 'low_enc_bytes.bin'), 'wb') as f:
        f.write(low)
    qrange, found = None, None
    if inargs.get('qrange_search', False):
        # the rate-checked quantiser range of codec.encode_gop (codec.search_qrange), on this road's per-scale inputs
        reading = [inargs['reading_data'][i] for i in range(inargs['frame_num'])]

        def frame_bits(cand, i):
            per_scale = []
            for sc in reading[i]['all_input_info']:
                putin = dict(sc)
                putin['coord'], putin['offset_tensor'] = sc['xyzqsc_t'].get_coord(), sc['xyzqsc_t'].get_offset_tensor()
                per_scale.append(cand.frame_probs(cand._scale_frame(putin))[1])
            return torch.stack(per_scale).sum(0)

        found = codec.search_qrange(trained, gen(), reading, bitdepth, 'f32', inargs.get('qrange_trims'), inargs.get('qrange_frames', 4),
                                    frame_bits=frame_bits)
        qrange = found['ranges'][found['chosen']] if found['chosen'] else None
    packed = Model_Estimate().compress_model(trained, bitdepth, True, gen(), **({} if qrange is None else {'qrange': qrange}))
    with open(os.path.join(bins_dir, 'model.bin'), 'wb') as f:
        f.write(packed['final_bytes'])
    side_info = {'mu': packed['mu'], 'b': packed['b'], 'min_param': packed['min_param'], 'max_param': packed['max_param'],
                 'enc_mode': packed['enc_mode'], 'bitdepth': bitdepth, 'arith_version': codec.ARITH_VERSION}
    side_info.update(codec.model_shape(trained))
    if stream_chunk:
        side_info['stream_chunk'] = stream_chunk
    digests_bin = None
    if inargs.get('digests', False):
        side_info['digests'] = stream_digests.VERSION
        digests_bin = codec.gop_digests_bin(codec.gop_digests_launch([inargs['reading_data'][i] for i in range(inargs['frame_num'])]))
        with open(os.path.join(bins_dir, 'digests.bin'), 'wb') as f:
            f.write(digests_bin)
    if found is not None and len(found['trims']) > 1:
        side_info['qrange_trim'] = int(found['trims'][found['chosen']])
        side_info['qrange_candidates'] = len(found['trims'])
    with open(os.path.join(result_dir, 'side_info.json'), 'w') as f:
        json.dump(side_info, f, indent=4)
    model = packed['new_model']
    bits, points = 0, 0
    for frame_idx in range(inargs['frame_num']):
        frame = inargs['reading_data'][frame_idx]
        out = encode_one_frame(model, frame['all_input_info'], frame.get('ori'), stream_chunk)
        write_bin_file(frame_idx, out['all_bytes'], bins_dir)
        bits += out['all_bit']
        points += frame['point_num']
    model_bits = packed['bit_real'] + codec.EXTRA_SIDE_BITS + (SIDE_BITS if stream_chunk else 0) + stream_digests.bits(digests_bin)
    return {**({} if digests_bin is None else {'digest_bits': stream_digests.bits(digests_bin)}),
            'point_bpp': bits / points, 'model_bpp': model_bits / points, 'xyzlow_bpp': len(low) * 8 / points,
            'bpp_all': (bits + model_bits + len(low) * 8) / points}
