"""Does the rate-checked quantiser range (codec.encode_gop qrange_search=) lower the coded rate, and what does the search cost?
Complete overfits with the reference's recipe (as tools/qat_ab.py runs them) on one resident GOP, in both training precisions, over
the seeds of profiles/qat_ab.txt; every trained model is then coded three times by the real codec - plain, with the search on 4
evaluated frames (the default), with the search on all frames - so the three arms differ in the quantiser's range alone.

Per run: total bits/point with the model (test_utils.py:146-157's accounting), the chosen trim, the gap between the coded point_bpp
and the loss of the coded epoch, the wall time of the search per GOP (search_s: the quantiser launch, candidates x evaluated frames
forwards, two host reads).  The report gives medians and spread over the seeds, never one seed.

  python tools/qrange_ab.py [--config loot10] [--gop 32] [--epochs 10] [--seeds 8807 1 2 3 4 5 6 7] [--precisions f32 bf16]
                            [--out profiles/qrange_ab.txt] [--step-timeout 240]

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

ARMS = (('plain', None), ('search 4', 4), ('search all', 0))


def worker(args):
    """The three arms of one (precision, seed): one JSON line each on stdout."""
    import torch
    from linr_pcgc_amd import codec, overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam
    prec, seed = args.precisions[0], args.seeds[0]
    clouds = [synthetic.sequence_frame_device(args.config, t, 'cuda') for t in range(args.gop)]
    gop = overfit.Gop(None, clouds, None, 64, 'cuda')
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=seed)
    model.train_precision = prec
    info = {}
    overfit.overfit_gop(model, FlatAdam(model), gop, args.epochs, info=info)
    for arm, frames in ARMS:
        kw = {} if frames is None else {'qrange_search': True, 'qrange_frames': frames}
        enc = codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda'), gop, 8, precision=prec, **kw)
        ok = None
        if args.decode:
            todo = list(range(min(args.decode, len(gop))))
            dec = codec.decode_gop(overfit.gen_model(gop.scale_num, 'cuda'), enc, frames=todo)
            ok = all(torch.equal(d, torch.as_tensor(gop.infos[i]['ori']).cuda() + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32))
                     for d, i in zip(dec, todo))
        bpp, found = enc['bpp'], enc.get('qrange')
        print(json.dumps({'train': prec, 'seed': seed, 'arm': arm, 'coded_loss': round(info['coded_loss'], 5),
                          'point_bpp': round(bpp['point_bpp'], 5), 'model_bpp': round(bpp['model_bpp'], 5), 'bpp_all': round(bpp['bpp_all'], 5),
                          'gap': round(bpp['point_bpp'] - info['coded_loss'], 5), 'min_param': enc['side_info']['min_param'],
                          'max_param': enc['side_info']['max_param'], 'trim': found['chosen'] if found else None,
                          'candidates': len(found['trims']) if found else None, 'search_s': round(found['search_s'], 5) if found else None,
                          'lossless': ok}), flush=True)


def spread(xs):
    xs = sorted(xs)
    return '%.4f  [%.4f .. %.4f]' % (statistics.median(xs), xs[0], xs[-1])


def report(args, runs, failed):
    lines = ['# Rate-checked quantiser range A/B (tools/qrange_ab.py): %s, GOP of %d frames, %d epochs, seeds %s; the codec runs in the' %
             (args.config, args.gop, args.epochs, ' '.join(str(s) for s in args.seeds)),
             '# training precision.  ONE trained model per (precision, seed), coded three times: plain (the default), the search with 4 evaluated',
             '# frames, the search with all frames; default trims.  Every cell: median over the seeds [min .. max].  gap = coded point_bpp - loss',
             '# of the coded epoch; rel gap = gap / that loss; search ms = wall time of the search per GOP.']
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
                spread([100.0 * r['gap'] / r['coded_loss'] for r in rs]), spread([r['model_bpp'] for r in rs]), spread(ms) if ms else '-'))
        lines.append('  per seed: bpp_all at %s   chosen trim   coded range' % ' / '.join(arms))
        for seed in args.seeds:
            row = [next((r for r in runs if r['train'] == prec and r['seed'] == seed and r['arm'] == a), None) for a in arms]
            if any(row):
                lines.append('    %5d  %s   trim %s   weights [%s]   coded loss %s' % (
                    seed, ' / '.join('%.4f' % r['bpp_all'] if r else '  -   ' for r in row),
                    ' / '.join('-' if not r or r['trim'] is None else str(r['trim']) for r in row),
                    ' / '.join('%.2f..%.2f' % (r['min_param'], r['max_param']) if r else '-' for r in row),
                    next(('%.4f' % r['coded_loss'] for r in row if r), '-')))
        both = [(a, b, c) for a, b, c in ([next((r for r in runs if r['train'] == prec and r['seed'] == s and r['arm'] == arm), None) for arm in arms]
                                          for s in args.seeds) if a and b and c]
        if both:
            for i, arm in ((1, arms[1]), (2, arms[2])):
                d = [100.0 * (t[i]['bpp_all'] - t[0]['bpp_all']) / t[0]['bpp_all'] for t in both]
                lines.append('  %s against plain, bpp_all per seed: %s %%   (%d of %d seeds lower, %d equal)' % (
                    arm, spread(d), sum(x < 0 for x in d), len(d), sum(x == 0 for x in d)))
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
    ap.add_argument('--decode', type=int, default=1, help='frames of every run to decode and compare with the input')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'qrange_ab.txt'))
    ap.add_argument('--step-timeout', type=int, default=240, help='seconds one (precision, seed) child may take')
    ap.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    runs, failed = [], None
    for prec in args.precisions:
        for seed in args.seeds:
            cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, os.path.abspath(__file__), '--worker', '--config', args.config,
                   '--gop', str(args.gop), '--epochs', str(args.epochs), '--seeds', str(seed), '--precisions', prec, '--decode', str(args.decode)]
            done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            for ln in done.stdout.splitlines():
                if ln.startswith('{'):
                    runs.append(json.loads(ln))
                    print(ln, flush=True)
            if done.returncode != 0:          # a fault, an abort or the time limit: nothing more is started on the GPU
                failed = 'the child for %s seed %d ended with status %d: %s' % (prec, seed, done.returncode, done.stderr[-400:].replace('\n', ' | '))
                break
        if failed:
            break
    text = report(args, runs, failed)
    with open(args.out, 'w') as f:
        f.write(text)
    print(text)
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
