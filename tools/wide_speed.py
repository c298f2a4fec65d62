"""ms per training step of the channel-blocked executor (hidden_channel_conv 16 / 32) on frame 0 of a config, beside width 8.

--train-precision takes one name or several separated by commas (f32,bf16-mul): the arms of a width run in ONE session, alternating,
--rounds timed rounds of --steps steps each after a warm-up; a line gives an arm's median round and its spread (min .. max).  Width 8
runs in f32 only ('bf16-mul' is an option of the wide models)."""
import argparse, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from linr_pcgc_amd import overfit, synthetic
from linr_pcgc_amd.model_core import FlatAdam, train_step

ap = argparse.ArgumentParser()
ap.add_argument('cfg', nargs='?', default='loot10')
ap.add_argument('--train-precision', '--train_precision', dest='train_precision', default='f32')
ap.add_argument('--hidden', default='8,16,32')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--steps', type=int, default=10)
args = ap.parse_args()
cfg = args.cfg
gop = overfit.Gop(None, [synthetic.sequence_frame_device(cfg, 0, 'cuda')], None, 64, 'cuda')
for hidden in [int(h) for h in args.hidden.split(',')]:
    arms = []
    for tp in (args.train_precision.split(',') if hidden != 8 else ['f32']):
        m = overfit.gen_model(gop.scale_num, 'cuda', seed=8807, hidden=hidden)
        m.train_precision = tp
        arms.append({'tp': tp, 'm': m, 'o': FlatAdam(m), 'bits': torch.zeros(1, dtype=torch.float64, device='cuda'), 'ms': [], 'first': None})
    for a in arms:
        for _ in range(3):
            train_step(a['m'], a['o'], gop.frames[0], gop.point_nums[0], out=a['bits'])
    for _ in range(args.rounds):
        for a in arms:
            torch.cuda.synchronize(); t0 = time.time()
            for i in range(args.steps):
                a['bits'].zero_(); train_step(a['m'], a['o'], gop.frames[0], gop.point_nums[0], out=a['bits'])
                if a['first'] is None: a['first'] = float(a['bits'])
            torch.cuda.synchronize()
            a['ms'].append((time.time() - t0) * 1e3 / args.steps)
    for a in arms:
        print('%s hidden %2d %-8s: %.2f ms/step (median of %d rounds, %.2f .. %.2f), %d parameters, bits %.0f -> %.0f' % (
            cfg, hidden, a['tp'], statistics.median(a['ms']), args.rounds, min(a['ms']), max(a['ms']), a['m'].flat_parameters().numel(),
            a['first'], float(a['bits'])))
