"""Does the quantisation-aware overfit (overfit_gop qat_epochs=) close the gap between the training loss and the coded rate?
Complete overfits with the reference's recipe (main.py:297-437: Adam, StepLR per frame, lr clamp per epoch, best-epoch checkpoint)
on one resident GOP, the last 0 / 1 / 2 / all epochs quantisation-aware, in both training precisions, over the seeds of
profiles/r06_bf16_overfit_seeds.txt; every run goes through the real codec (bits/point as test_utils.py:146-157 counts them).
qat_epochs 0 is the plain overfit: the comparison is inside one build.

Per run: coded_epoch, coded_loss, the coded point_bpp / model_bpp / bpp_all, the gap point_bpp - coded_loss, min_param / max_param,
and every epoch timed with HIP events (ms per step of plain and of quantisation-aware epochs side by side).  The report gives
medians and spread over the seeds, never one seed.

  python tools/qat_ab.py [--config loot10] [--gop 32] [--epochs 10] [--seeds 8807 1 2 3 4 5 6 7] [--qat 0 1 2 10]
                         [--precisions f32 bf16] [--out profiles/qat_ab.txt] [--step-timeout 240]

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


def worker(args):
    """All --qat variants of one (precision, seed): one JSON line each on stdout."""
    import torch
    from linr_pcgc_amd import codec, overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam
    prec, seed = args.precisions[0], args.seeds[0]
    clouds = [synthetic.sequence_frame_device(args.config, t, 'cuda') for t in range(args.gop)]
    gop = overfit.Gop(None, clouds, None, 64, 'cuda')
    for qat in args.qat:
        model = overfit.gen_model(gop.scale_num, 'cuda', seed=seed)
        model.train_precision = prec
        opt = FlatAdam(model)
        info, ms = {}, []
        mark = [torch.cuda.Event(enable_timing=True)]

        def on_epoch(epoch, loss):
            end = torch.cuda.Event(enable_timing=True)
            end.record()
            end.synchronize()
            ms.append(mark[0].elapsed_time(end) / len(gop))
            mark[0] = torch.cuda.Event(enable_timing=True)
            mark[0].record()
        mark[0].record()
        if qat:
            losses = overfit.overfit_gop(model, opt, gop, args.epochs, info=info, on_epoch=on_epoch, qat_epochs=qat, qat_bitdepth=8)
            model.qat_epochs = min(qat, args.epochs)
        else:
            losses = overfit.overfit_gop(model, opt, gop, args.epochs, info=info, on_epoch=on_epoch)
        enc = codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda'), gop, 8, precision=prec)
        ok = None
        if args.decode:
            todo = list(range(min(args.decode, len(gop))))
            dec = codec.decode_gop(overfit.gen_model(gop.scale_num, 'cuda'), enc, frames=todo)
            ok = all(torch.equal(d, torch.as_tensor(gop.infos[i]['ori']).cuda() + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32))
                     for d, i in zip(dec, todo))
        q0 = info.get('qat_from', args.epochs)
        bpp = enc['bpp']
        print(json.dumps({'train': prec, 'seed': seed, 'qat_epochs': qat, 'loss_per_epoch': [round(x, 5) for x in losses],
                          'coded_epoch': info['coded_epoch'], 'coded_loss': round(info['coded_loss'], 5),
                          'point_bpp': round(bpp['point_bpp'], 5), 'model_bpp': round(bpp['model_bpp'], 5), 'bpp_all': round(bpp['bpp_all'], 5),
                          'gap': round(bpp['point_bpp'] - info['coded_loss'], 5), 'min_param': enc['side_info']['min_param'],
                          'max_param': enc['side_info']['max_param'],
                          # (epoch 0 of a run warms up: left out of both lists)
                          'ms_per_step_plain': [round(x, 4) for x in ms[1:q0]], 'ms_per_step_qat': [round(x, 4) for x in ms[max(q0, 1):]],
                          'lossless': ok}), flush=True)


def spread(xs):
    xs = sorted(xs)
    return '%.4f  [%.4f .. %.4f]' % (statistics.median(xs), xs[0], xs[-1])


def report(args, runs, failed):
    lines = ['# Quantisation-aware overfit A/B (tools/qat_ab.py): %s, GOP of %d frames, %d epochs, seeds %s; the codec runs in the' %
             (args.config, args.gop, args.epochs, ' '.join(str(s) for s in args.seeds)),
             '# training precision.  qat = the last N epochs are quantisation-aware (0: the plain overfit, the default).  Every cell: median over',
             '# the seeds [min .. max].  gap = coded point_bpp - loss of the coded epoch; rel gap = gap / that loss.']
    if failed:
        lines.append('# INCOMPLETE: %s' % failed)
    for prec in args.precisions:
        lines.append('')
        lines.append('## training precision %s' % prec)
        lines.append('  qat  seeds  bpp_all                      point_bpp                    coded_loss                   gap                           rel gap %                  model_bpp')
        for qat in args.qat:
            rs = [r for r in runs if r['train'] == prec and r['qat_epochs'] == qat]
            if not rs:
                continue
            lines.append('  %3d  %5d  %s  %s  %s  %s  %s  %s' % (
                qat, len(rs), spread([r['bpp_all'] for r in rs]), spread([r['point_bpp'] for r in rs]), spread([r['coded_loss'] for r in rs]),
                spread([r['gap'] for r in rs]), spread([100.0 * r['gap'] / r['coded_loss'] for r in rs]), spread([r['model_bpp'] for r in rs])))
        plain = [x for r in runs if r['train'] == prec for x in r['ms_per_step_plain']]
        aware = [x for r in runs if r['train'] == prec for x in r['ms_per_step_qat']]
        if plain and aware:
            lines.append('  ms per step (HIP events around every epoch, its host read of the loss included), medians over all epochs but the first of all runs:')
            lines.append('    plain %.4f   quantisation-aware %.4f   difference %.1f us' %
                         (statistics.median(plain), statistics.median(aware), 1e3 * (statistics.median(aware) - statistics.median(plain))))
        lines.append('  per seed: bpp_all at qat = %s' % ' / '.join(str(q) for q in args.qat))
        for seed in args.seeds:
            row = [next((r for r in runs if r['train'] == prec and r['seed'] == seed and r['qat_epochs'] == q), None) for q in args.qat]
            if any(row):
                lines.append('    %5d  %s   coded epoch %s   weights [%s]' % (
                    seed, ' / '.join('%.4f' % r['bpp_all'] if r else '  -   ' for r in row), ' / '.join(str(r['coded_epoch']) if r else '-' for r in row),
                    ' / '.join('%.2f..%.2f' % (r['min_param'], r['max_param']) if r else '-' for r in row)))
    bad = [r for r in runs if r['lossless'] is False]
    lines.append('')
    lines.append('decoded frames lossless: %s' % ('all' if not bad else 'NO: %s' % [(r['train'], r['seed'], r['qat_epochs']) for r in bad]))
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='loot10')
    ap.add_argument('--gop', type=int, default=32)
    ap.add_argument('--epochs', type=int, default=10)
    ap.add_argument('--seeds', type=int, nargs='+', default=[8807, 1, 2, 3, 4, 5, 6, 7])
    ap.add_argument('--qat', type=int, nargs='+', default=[0, 1, 2, 10])
    ap.add_argument('--precisions', nargs='+', default=['f32', 'bf16'], choices=['f32', 'bf16'])
    ap.add_argument('--decode', type=int, default=1, help='frames of every run to decode and compare with the input')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'qat_ab.txt'))
    ap.add_argument('--step-timeout', type=int, default=240, help='seconds one (precision, seed) child may take')
    ap.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    runs, failed = [], None
    for prec in args.precisions:
        for seed in args.seeds:
            cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, os.path.abspath(__file__), '--worker', '--config', args.config,
                   '--gop', str(args.gop), '--epochs', str(args.epochs), '--seeds', str(seed), '--precisions', prec, '--decode', str(args.decode),
                   '--qat'] + [str(q) for q in args.qat]
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
