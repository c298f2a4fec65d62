"""Does coding a rate-checked average of the overfit's iterates (overfit_gop avg_decays=, codec.encode_gop avg=) lower the coded rate,
and what do the search and the extra launch per step cost?  Complete overfits with the reference's recipe (as tools/qrange_ab.py runs
them) on one resident GOP, in both training precisions, over the seeds of profiles/qat_ab.txt; every cell trains ONE model - the
averages ride along, training is bit for bit what it is without them - and codes it three times with the real codec: plain, with the
choice on 4 evaluated frames (the default), with the choice on all frames.  The comparison is paired: the arms of a seed differ in the
coded vector alone.

Per run: total bits/point with the model (test_utils.py:146-157's accounting), the chosen decay, the gap between the coded point_bpp
and the loss of the coded epoch, the wall time of the search per GOP.  The report gives medians and spread over the seeds, never one
seed, and per seed how the two rates compare.  A last child measures the averaging launch's cost per step: HIP events around whole
epochs of one session in which epochs without and with the launch alternate, median of 5 epochs per arm with min .. max.

  python tools/avg_ab.py [--config loot10] [--gop 32] [--epochs 10] [--seeds 8807 1 2 3 4 5 6 7] [--precisions f32 bf16]
                         [--decays 0.9 0.97 0.99] [--out profiles/avg_ab.txt] [--step-timeout 240]

The driver starts one child process per (precision, seed) - a GPU step of its own under `timeout`; the first one that fails ends the
run (nothing more is started on the GPU) and what was measured so far is reported.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = (('plain', None), ('avg 4', 4), ('avg all', 0))


def stage(args):
    from linr_pcgc_amd import overfit, synthetic
    clouds = [synthetic.sequence_frame_device(args.config, t, 'cuda') for t in range(args.gop)]
    return overfit.Gop(None, clouds, None, 64, 'cuda')


def worker(args):
    """The three arms of one (precision, seed): one JSON line each on stdout."""
    import torch
    from linr_pcgc_amd import codec, overfit
    from linr_pcgc_amd.model_core import FlatAdam
    prec, seed = args.precisions[0], args.seeds[0]
    gop = stage(args)
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=seed)
    model.train_precision = prec
    info = {}
    overfit.overfit_gop(model, FlatAdam(model), gop, args.epochs, info=info, avg_decays=tuple(args.decays))
    for arm, frames in ARMS:
        kw = {} if frames is None else {'avg': info['averages'], 'avg_frames': frames}
        enc = codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda'), gop, 8, precision=prec, **kw)
        ok = None
        if args.decode:
            todo = list(range(min(args.decode, len(gop))))
            dec = codec.decode_gop(overfit.gen_model(gop.scale_num, 'cuda'), enc, frames=todo)
            ok = all(torch.equal(d, torch.as_tensor(gop.infos[i]['ori']).cuda() + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32))
                     for d, i in zip(dec, todo))
        bpp, found = enc['bpp'], enc.get('average')
        print(json.dumps({'train': prec, 'seed': seed, 'arm': arm, 'coded_loss': round(info['coded_loss'], 5), 'coded_epoch': info['coded_epoch'],
                          'point_bpp': round(bpp['point_bpp'], 5), 'model_bpp': round(bpp['model_bpp'], 5), 'bpp_all': round(bpp['bpp_all'], 5),
                          'gap': round(bpp['point_bpp'] - info['coded_loss'], 5),
                          'decay': enc['side_info'].get('avg_decay'), 'chosen': found['chosen'] if found else None,
                          'objective_bits': [None if x is None else round(x, 1) for x in found['objective_bits']] if found else None,
                          'search_s': round(found['search_s'], 5) if found else None, 'lossless': ok}), flush=True)


def cost_worker(args):
    """The averaging launch's cost per step: epochs without and with it alternate in one session, each between two HIP events."""
    import torch
    from linr_pcgc_amd import engine, overfit
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    prec = args.precisions[0]
    gop = stage(args)
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=args.seeds[0])
    model.train_precision = prec
    if prec == 'bf16':
        gop.share_train_bf16_arena()
    opt = FlatAdam(model)
    w = overfit.avg_weights(tuple(args.decays))
    n = model.flat_parameters().numel()
    rows = torch.zeros((len(w), (n + 3) & ~3), dtype=torch.float32, device='cuda')
    bits = torch.zeros(len(gop), dtype=torch.float64, device='cuda')
    ms = {'off': [], 'on': []}
    for epoch in range(2 + 10):                          # two warm-up epochs, then 5 per arm, alternating
        arm = 'on' if epoch % 2 else 'off'
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        bits.zero_()
        ev0.record()
        for j, (f, pn) in enumerate(zip(gop.frames, gop.point_nums)):
            train_step(model, opt, f, pn, out=bits[j:j + 1])
            if arm == 'on':
                engine.params_average(model.flat_parameters(), w, rows)
        ev1.record()
        torch.cuda.synchronize()
        if epoch >= 2:
            ms[arm].append(ev0.elapsed_time(ev1) / len(gop))
    print(json.dumps({'cost': prec, 'rows': len(w), 'off_ms_per_step': ms['off'], 'on_ms_per_step': ms['on']}), flush=True)


def spread(xs, fmt='%.4f'):
    xs = sorted(xs)
    return (fmt + '  [' + fmt + ' .. ' + fmt + ']') % (statistics.median(xs), xs[0], xs[-1])


def report(args, runs, costs, failed):
    lines = ['# Averaged weights A/B (tools/avg_ab.py): %s, GOP of %d frames, %d epochs, seeds %s; decays %s; the codec runs in the' %
             (args.config, args.gop, args.epochs, ' '.join(str(s) for s in args.seeds), ' '.join('%g' % d for d in args.decays)),
             '# training precision.  ONE trained model per (precision, seed), coded three times: plain (the default), the rate-checked choice',
             '# between the model and its averages on 4 evaluated frames, the choice on all frames.  Every cell: median over the seeds',
             '# [min .. max].  gap = coded point_bpp - loss of the coded epoch; rel gap = gap / that loss; search ms = wall time of the search per GOP.']
    if failed:
        lines.append('# INCOMPLETE: %s' % failed)
    arms = [a for a, _ in ARMS]
    for prec in args.precisions:
        lines.append('')
        lines.append('## training precision %s' % prec)
        lines.append('  arm         seeds  bpp_all                      point_bpp                    gap                           rel gap %                   model_bpp                    search ms')
        for arm in arms:
            rs = [r for r in runs if r['train'] == prec and r['arm'] == arm]
            if not rs:
                continue
            ms = [1e3 * r['search_s'] for r in rs if r['search_s'] is not None]
            lines.append('  %-10s  %5d  %s  %s  %s  %s  %s  %s' % (
                arm, len(rs), spread([r['bpp_all'] for r in rs]), spread([r['point_bpp'] for r in rs]), spread([r['gap'] for r in rs]),
                spread([100.0 * r['gap'] / r['coded_loss'] for r in rs]), spread([r['model_bpp'] for r in rs]), spread(ms, '%.1f') if ms else '-'))
        lines.append('  per seed: bpp_all at %s   point_bpp at the same   chosen decay   coded epoch and its loss' % ' / '.join(arms))
        for seed in args.seeds:
            row = [next((r for r in runs if r['train'] == prec and r['seed'] == seed and r['arm'] == a), None) for a in arms]
            if any(row):
                lines.append('    %5d  %s   %s   decay %s   epoch %s loss %s' % (
                    seed, ' / '.join('%.4f' % r['bpp_all'] if r else '  -   ' for r in row),
                    ' / '.join('%.4f' % r['point_bpp'] if r else '  -   ' for r in row),
                    ' / '.join('-' if not r or r['chosen'] is None else ('plain' if r['decay'] is None else '%g' % r['decay']) for r in row),
                    next((str(r['coded_epoch']) for r in row if r), '-'), next(('%.4f' % r['coded_loss'] for r in row if r), '-')))
        both = [(a, b, c) for a, b, c in ([next((r for r in runs if r['train'] == prec and r['seed'] == s and r['arm'] == arm), None) for arm in arms]
                                          for s in args.seeds) if a and b and c]
        if both:
            for i, arm in ((1, arms[1]), (2, arms[2])):
                d = [100.0 * (t[i]['bpp_all'] - t[0]['bpp_all']) / t[0]['bpp_all'] for t in both]
                lines.append('  %s against plain, bpp_all per seed: %s %%   (%d of %d seeds lower, %d equal, %d higher)' % (
                    arm, spread(d), sum(x < 0 for x in d), len(d), sum(x == 0 for x in d), sum(x > 0 for x in d)))
    if costs:
        lines.append('')
        lines.append('## the averaging launch per step (%d rows): HIP events around whole epochs, epochs without / with it alternating in one session,' % costs[0]['rows'])
        lines.append('## median of 5 epochs per arm [min .. max], ms per step')
        for c in costs:
            off, on = c['off_ms_per_step'], c['on_ms_per_step']
            lines.append('  %-5s  without %s   with %s   difference of the medians %+.1f us' % (
                c['cost'], spread(off), spread(on), 1e3 * (statistics.median(on) - statistics.median(off))))
    bad = [r for r in runs if r['lossless'] is False]
    lines.append('')
    lines.append('decoded frames lossless: %s' % ('all' if not bad else 'NO: %s' % [(r['train'], r['seed'], r['arm']) for r in bad]))
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='loot10')
    ap.add_argument('--gop', type=int, default=32)
    ap.add_argument('--epochs', type=int, default=10)
    ap.add_argument('--seeds', type=int, nargs='+', default=[8807, 1, 2, 3, 4, 5, 6, 7])
    ap.add_argument('--precisions', nargs='+', default=['f32', 'bf16'], choices=['f32', 'bf16'])
    ap.add_argument('--decays', type=float, nargs='+', default=[0.9, 0.97, 0.99])
    ap.add_argument('--decode', type=int, default=1, help='frames of every run to decode and compare with the input')
    ap.add_argument('--no-cost', dest='cost', action='store_false', help='skip the per-step cost of the averaging launch')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'avg_ab.txt'))
    ap.add_argument('--step-timeout', type=int, default=240, help='seconds one (precision, seed) child may take')
    ap.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--cost-worker', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if args.cost_worker:
        return cost_worker(args)
    runs, costs, failed = [], [], None
    common = ['--config', args.config, '--gop', str(args.gop), '--epochs', str(args.epochs), '--decode', str(args.decode),
              '--decays'] + ['%r' % d for d in args.decays]
    jobs = [('--worker', prec, seed) for prec in args.precisions for seed in args.seeds]
    if args.cost:
        jobs += [('--cost-worker', prec, args.seeds[0]) for prec in args.precisions]
    for mode, prec, seed in jobs:
        cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, os.path.abspath(__file__), mode, '--seeds', str(seed),
               '--precisions', prec] + common
        done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        for ln in done.stdout.splitlines():
            if ln.startswith('{'):
                (costs if mode == '--cost-worker' else runs).append(json.loads(ln))
                print(ln, flush=True)
        if done.returncode != 0:          # a fault, an abort or the time limit: nothing more is started on the GPU
            failed = 'the child for %s seed %d (%s) ended with status %d: %s' % (prec, seed, mode, done.returncode, done.stderr[-400:].replace('\n', ' | '))
            break
    text = report(args, runs, costs, failed)
    with open(args.out, 'w') as f:
        f.write(text)
    print(text)
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
