"""A/B of the decoder and the codec forward of hidden_channel_conv 16 / 32 on their C schedule (csrc/wide_fwd.hip, the wide scale entries
of csrc/decode.hip) against the Python schedule, one process, one GPU: loot10 at GOP 4 (argv[1]), widths 16 and 32, fp32 and bf16
precision, the model of seed 8807 as initialised (the arms decode the same streams; their entropy does not enter the comparison).

  decode, ms per frame:  codec.decode_one_frame_stagewise per frame (model.decode per scale, the stage loop in Python)
                         against decode_gop() = the scale entries at workers = 1, then decode_gop(workers=4) and decode_gop(lockstep=4)
  codec forward, ms:     model.frame_probs with WideNet.c_forward off and on, on frame 0 of loot10 and on a 6-bit shell frame (launch-bound)

Medians of 5 after one warm-up per arm, the arms alternating inside every round, a device synchronisation around every timed call;
min - max beside every median.  An arm is called faster only where its median lies outside the other arm's min - max AND the other's
median outside its own.  Every decode is checked lossless."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from linr_pcgc_amd import codec, overfit, synthetic                     # noqa: E402
from linr_pcgc_amd.model_codec import Model_Estimate                    # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4
RUNS = 5
torch.set_num_threads(4)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.time()
    out = fn()
    torch.cuda.synchronize()
    return (time.time() - t0) * 1e3, out


def alternate(arms):
    """arms: [(name, fn)] -> {name: sorted times}: one warm-up each, then RUNS rounds with the arms one after the other."""
    for _, fn in arms:
        fn()
    t = {name: [] for name, _ in arms}
    for _ in range(RUNS):
        for name, fn in arms:
            t[name].append(timed(fn)[0])
    return {k: sorted(v) for k, v in t.items()}


def verdict(a, b):
    ma, mb = statistics.median(a), statistics.median(b)
    apart = (ma < b[0] or ma > b[-1]) and (mb < a[0] or mb > a[-1])
    return '%.2fx, %s' % (ma / mb, ('faster' if mb < ma else 'slower') if apart else 'not separated (a median lies inside the other min-max)')


def show(title, t, per=1.0, base=None):
    print(title)
    for name, v in t.items():
        v = [x / per for x in v]
        line = '  %-44s median %9.3f  min %9.3f  max %9.3f' % (name, statistics.median(v), v[0], v[-1])
        if base is not None and name != base:
            line += '   vs %s: %s' % (base, verdict(t[base], t[name]))
        print(line)


clouds = [synthetic.sequence_frame_device('loot10', t, 'cuda') for t in range(n)]
gop = overfit.Gop(None, clouds, None, 64, 'cuda')
small = overfit.Gop(None, [synthetic.sphere_shell(6, 20)], None, 64, 'cuda')
truth = [torch.as_tensor(gop.infos[i]['ori']).cuda() + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32) for i in range(n)]
print('loot10, %d frames, %d points, %d rows in frame 0; the shell frame has %d rows; %d host threads available'
      % (n, sum(gop.point_nums), gop.frames[0].rows, small.frames[0].rows, len(os.sched_getaffinity(0))))

for hidden in (16, 32):
    for precision in ('f32', 'bf16'):
        print('==== hidden_channel_conv %d, precision %s' % (hidden, precision))
        gen = lambda seed=None, g=gop: overfit.gen_model(g.scale_num, 'cuda', seed=seed, hidden=hidden)          # noqa: E731
        enc = codec.encode_gop(gen(8807), gen(), gop, 8, precision=precision)
        side = dict(enc['side_info'])
        side.pop('arith_version', None)
        side['final_bytes'] = enc['model_bin']
        model, _ = Model_Estimate().decompress_model(gen(), side)
        model.inference_precision = side.get('precision', 'f32')
        lows, mins = codec.dec_all_frame_low_xyz(enc['low_enc_bytes'])

        def stagewise():
            return [codec.decode_one_frame_stagewise(model, list(enc['frames'][i]), torch.tensor(lows[i].astype(np.int32), device='cuda'))
                    ['dec_coord'] + torch.tensor(mins[i], device='cuda', dtype=torch.int32) for i in range(n)]

        arms = [('decode_one_frame_stagewise (Python stage loop)', stagewise),
                ('decode_gop() (scale entries, workers=1)', lambda: codec.decode_gop(gen(), enc, 'cuda')),
                ('decode_gop(workers=4)', lambda: codec.decode_gop(gen(), enc, 'cuda', workers=4)),
                ('decode_gop(lockstep=4)', lambda: codec.decode_gop(gen(), enc, 'cuda', lockstep=4))]
        for name, fn in arms:
            assert all(torch.equal(a.to(torch.int32), b) for a, b in zip(fn(), truth)), name
        show('decode, ms per frame (all arms lossless)', alternate(arms), per=n, base=arms[0][0])

        for what, g in (('loot10 frame 0', gop), ('6-bit shell frame', small)):
            coded = Model_Estimate().compress_model(overfit.gen_model(g.scale_num, 'cuda', seed=8807, hidden=hidden), 8, True,
                                                    overfit.gen_model(g.scale_num, 'cuda', hidden=hidden))['new_model']
            frame = g.frames[0]

            def forward(on):
                coded._wide.c_forward = on
                return coded.frame_probs(frame, precision=precision)
            p0, b0 = forward(False)
            p1, b1 = forward(True)
            assert torch.equal(p0, p1) and torch.equal(b0, b1)
            show('codec forward (frame_probs) on the %s, %d rows, ms' % (what, frame.rows),
                 alternate([('c_forward off (Python schedule)', lambda: forward(False)), ('c_forward on (one C call)', lambda: forward(True))]),
                 base='c_forward off (Python schedule)')
