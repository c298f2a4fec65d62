"""decoder.py of the reference (decode / decode_one_gop / decode_one_frame, decoder.py:16-176) with its argument dicts: the
files of ``encoder.encode`` (or ``codec.write_gop``) in, every frame rebuilt from them alone, compared with the test data set
and - with ``write_flag`` - written as ``<result_dec_dir>/frameXXXX.ply``.  The frame window of a GOP is inclusive (see
encoder.py here for the reference's off-by-one)."""
import os

import torch

from . import codec
from .codec import decode_one_frame          # noqa: F401  (decoder.py:153-176: the drivers import it from here)
from .custom_dataset import Read_Data_with_cache
from .ply import PlyWriter
from .encoder import gop_bounds


def decode(inargs):
    """decoder.py:16-48.  inargs: 'gop_names', 'result_enc_dir', 'result_dec_dir', 'Gen_Model', 'dataset' (a MytestDataset: the
    sorted voxel list of every frame), 'write_flag'; optional 'device_decoder' (True: the range decoders run on the GPU,
    codec.decode_gop device_decoder=), 'verify' (default True: a GOP that carries digests is checked scale by scale,
    codec.decode_gop verify=; _lib.LinrDigestError names the frame and scale that differ)."""
    os.makedirs(inargs['result_dec_dir'], exist_ok=True)
    for gop_name in inargs['gop_names']:
        first, last = gop_bounds(gop_name)
        decode_one_gop({'gop_bound': [first, last], 'frame_num': last - first + 1, 'result_enc_dir': inargs['result_enc_dir'],
                        'result_dec_dir': inargs['result_dec_dir'], 'Gen_Model': inargs['Gen_Model'], 'gop_name': gop_name,
                        'reading_data': Read_Data_with_cache(inargs['dataset'], list(range(first, last + 1))),
                        'write_flag': inargs['write_flag'], 'device_decoder': bool(inargs.get('device_decoder', False)),
                        'verify': bool(inargs.get('verify', True))})


def decode_one_gop(inargs):
    """decoder.py:51-146: model.bin -> parameters, then every frame from its streams and the coarsest coordinates; raises
    AssertionError on the first frame that differs from the data set's."""
    enc = codec.read_gop(os.path.join(inargs['result_enc_dir'], inargs['gop_name']))
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    extra = {'device_decoder': True} if inargs.get('device_decoder', False) else {}
    if not inargs.get('verify', True):
        extra['verify'] = False
    decoded = codec.decode_gop(inargs['Gen_Model'](), enc, dev, frames=list(range(inargs['frame_num'])), workers=1, **extra)
    with PlyWriter() as writer:          # formatted on the GPU, written by the writer's thread; closed before this returns or raises
        for frame_idx, dec in enumerate(decoded):
            truth = inargs['reading_data'][frame_idx]
            if dec.shape != truth.shape or bool((dec.to(truth.dtype) != truth).any()):
                raise AssertionError('frame %d of %s does not decode to the input' % (frame_idx, inargs['gop_name']))
            if inargs['write_flag']:
                name = 'frame%s.ply' % str(inargs['gop_bound'][0] + frame_idx).zfill(4)
                writer.submit(os.path.join(inargs['result_dec_dir'], name), dec)
    return decoded


def parser():
    """The command line of main()."""
    import argparse
    ap = argparse.ArgumentParser('linr_pcgc_amd.decoder')
    ap.add_argument('--enc-dir', required=True)
    ap.add_argument('--dec-dir', required=True)
    ap.add_argument('--ori-dir', default=None)
    ap.add_argument('--ori-type', default='ply', choices=['ply', 'npy'])
    ap.add_argument('--hidden-channel-conv', type=int, default=8)
    ap.add_argument('--block-layers', type=int, default=1)
    ap.add_argument('--lockstep', type=int, default=0,
                    help='decode the frames of a GOP in groups of up to this many, all scales in lock step (codec.decode_gop lockstep=; 0: frame by frame)')
    ap.add_argument('--device-decoder', '--device_decoder', dest='device_decoder', action='store_true',
                    help='range-decode on the GPU, a wave per stream or chunk, without host coder threads (codec.decode_gop device_decoder=; '
                         'hidden_channel_conv 8 only); the files read are the same')
    ap.add_argument('--ply-parse', '--ply_parse', dest='ply_parse', default='host', choices=['host', 'device'],
                    help='with --ori-dir: the original PLY frames are parsed by the host parser (default) or on the GPU (ply.read_points_device)')
    ap.add_argument('--no-verify', '--no_verify', dest='verify', action='store_false',
                    help='do not check the decoded octree levels against the digests a GOP carries (codec.decode_gop verify=False); without '
                         'this flag a GOP encoded with --digests is checked scale by scale and the first level that differs ends the run')
    return ap


def main(argv=None):
    """python -m linr_pcgc_amd.decoder --enc-dir OUT/result_enc --dec-dir OUT/dec [--ori-dir frames --ori-type ply --ply-parse device] [--lockstep B]
    [--device-decoder] [--no-verify]
    The decoder as its own program (decoder.py:179-200): every GOP under --enc-dir from its files alone, frames written as
    frameXXXX.ply; with --ori-dir each one is also compared with the input.  The model's shape travels in side_info.json (the
    reference hard-codes it, decoder.py:189); for streams without it the scale count is read off the stream files and width /
    block_layers are flags.  A GOP that carries digests (run.py --digests; stream_digests.py) is verified against them while it is
    decoded - no originals needed -; the first level that differs ends the program with a non-zero status and a message that names
    the GOP, frame and scale.  The closing line says so when every GOP had them."""
    from ._lib import LinrDigestError
    from .model_core import LINR_PCGC_Model
    args = parser().parse_args(argv)
    names = sorted((n for n in os.listdir(args.enc_dir) if n.startswith('gop_')), key=lambda n: gop_bounds(n)[0])
    if not names:
        raise ValueError('no gop_* directory under %s' % args.enc_dir)
    os.makedirs(args.dec_dir, exist_ok=True)
    truth = None
    if args.ori_dir is not None:
        from .custom_dataset import MytestDataset
        truth = MytestDataset(args.ori_dir, ori_type=args.ori_type, device_parse=args.ply_parse == 'device')
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    extra = {'device_decoder': True} if args.device_decoder else {}
    if not args.verify:
        extra['verify'] = False
    frames, verified = 0, 0
    with PlyWriter() as writer:          # closed - every file complete - before main returns or raises
        for name in names:
            first, last = gop_bounds(name)
            enc = codec.read_gop(os.path.join(args.enc_dir, name))
            side = enc['side_info']          # streams of this package carry the model's shape; others: the flags, and the most scales a frame has
            shape = {'scale_num': int(side.get('scale_num', max(len(f) for f in enc['frames']))), 'in_channel': 7,
                     'hidden_channel_conv': int(side.get('hidden_channel_conv', args.hidden_channel_conv)),
                     'block_layers': int(side.get('block_layers', args.block_layers)), 'outstage': 8, 'instage': 1}
            gen = lambda: LINR_PCGC_Model(shape).to(dev)
            try:
                if args.lockstep > 0:
                    decoded = codec.decode_gop(gen(), enc, dev, lockstep=args.lockstep, **extra)
                else:
                    decoded = codec.decode_gop(gen(), enc, dev, workers=1 if shape['hidden_channel_conv'] != 8 else 4, **extra)
            except LinrDigestError as e:
                raise SystemExit('%s: %s' % (name, e))
            verified += bool(args.verify and side.get('digests') and enc.get('digests_bin') is not None)
            if len(decoded) != last - first + 1:
                raise ValueError('%s holds %d frames, its name says %d' % (name, len(decoded), last - first + 1))
            for i, dec in enumerate(decoded):
                if truth is not None:
                    want = torch.unique(truth[first + i], dim=0)
                    if dec.shape != want.shape or bool((dec.to(want.dtype) != want).any()):
                        raise AssertionError('frame %d does not decode to the input' % (first + i))
                writer.submit(os.path.join(args.dec_dir, 'frame%s.ply' % str(first + i).zfill(4)), dec)
                frames += 1
    notes = ([] if truth is None else ['all equal to the input']) + (["verified against the stream's digests"] if verified == len(names) else [])
    print('decoded %d frames of %d GOPs into %s%s' % (frames, len(names), args.dec_dir, ' (%s)' % ', '.join(notes) if notes else ''))


if __name__ == '__main__':
    main()
