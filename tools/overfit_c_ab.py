"""What does the one-call overfit (overfit.overfit_gop(c_loop=True), csrc/overfit.hip: linr_overfit_gop) buy over the Python loop?

In-process arms, alternating in one session on the same resident GOP - loop | call, one warm-up of each, then --runs of each (default
5); the time of an arm is the wall of overfit_gop up to a device synchronisation, from a fresh model of the same seed:

  loot10   GOP 32, --epochs epochs, fp32 and bf16, width 8            (the headline workload: the step is GPU-bound)
  loot10   GOP 4, width 16                                            (the channel-blocked executor; the loop runs its one-call step, too)
  sphere8  GOP 32 of small frames                                     (58 k rows: still GPU-bound)
  6-bit shells, GOP 32 of ~2 k-row frames, fp32, bf16 and width 16    (the step is launch- and host-bound)

Every pair of arms must leave the same parameters and moments (sha256), or the report says so.  Then run.py as the program, every run
a fresh child: serial | --c-overfit | --pipeline | --pipeline --c-overfit on loot10 (--frames, --gop): sec_per_frame, the sum of the
GOPs' overfit_s, and per loop the training slowdown beside the finish thread (overfit sum under --pipeline over the serial one).
"Faster" is written only where the medians differ by more than the spread of BOTH arms.

--hashes: print the sha256 of parameters, moments and bits after a loot10 GOP-4 overfit by the DEFAULT path in fp32, bf16 and width
16 and exit; run it in a checkout of the parent commit as well (--parent-tree DIR does) - the default path must not have moved.

  python tools/overfit_c_ab.py [--runs 5] [--program-runs 5] [--epochs 10] [--frames 300] [--gop 32] [--out profiles/overfit_c_loop.txt] [--parent-tree DIR]

Every child is a GPU step of its own under `timeout`; the first failure - a hash child, the in-process arms or a run.py child - ends the
run: nothing more is started on the GPU, what was measured so far is reported, and the exit status is 1.
"""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def make(overfit, gop, hidden, tp, c_step=False):
    from linr_pcgc_amd.model_core import FlatAdam
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807, hidden=hidden)
    model.train_precision = tp
    if c_step and model._wide is not None:
        model._wide.c_step = True
    return model, FlatAdam(model)


def hashes():
    """The default path only, with nothing this tool's own commit added: runs unchanged in a checkout of the parent."""
    import torch
    from linr_pcgc_amd import overfit, synthetic
    gop = overfit.Gop(None, [synthetic.sequence_frame_device('loot10', t, 'cuda') for t in range(4)], None, 64, 'cuda')
    out = {}
    for name, hidden, tp in (('f32', 8, 'f32'), ('bf16', 8, 'bf16'), ('w16', 16, 'f32')):
        model, opt = make(overfit, gop, hidden, tp)
        losses = overfit.overfit_gop(model, opt, gop, 2)
        torch.cuda.synchronize()
        out[name] = sha(model.flat_parameters(), opt.exp_avg, opt.exp_avg_sq, torch.tensor(losses, dtype=torch.float64))
    print('HASHES ' + json.dumps(out, sort_keys=True))


def spread(xs, fmt='%.4f'):
    xs = sorted(xs)
    return (fmt + '  [' + fmt + ' .. ' + fmt + ']') % (statistics.median(xs), xs[0], xs[-1])


def verdict(a, b, what_a, what_b):
    """a, b: the two arms' samples (lower is better)."""
    ma, mb = statistics.median(a), statistics.median(b)
    if max(b) < min(a):
        return '%s is faster than %s: %.1f %% (medians; the ranges do not overlap)' % (what_b, what_a, 100 * (ma - mb) / ma)
    if max(a) < min(b):
        return '%s is faster than %s: %.1f %% (medians; the ranges do not overlap)' % (what_a, what_b, 100 * (mb - ma) / mb)
    return 'not separated: the ranges of %s and %s overlap (medians %.4f / %.4f)' % (what_a, what_b, ma, mb)


def in_process(args, lines):
    import torch
    from linr_pcgc_amd import overfit, synthetic
    work = (('loot10 GOP 32 fp32 width 8', 'loot10', 32, 8, 'f32'), ('loot10 GOP 32 bf16 width 8', 'loot10', 32, 8, 'bf16'),
            ('loot10 GOP 4 width 16', 'loot10', 4, 16, 'f32'), ('sphere8 GOP 32 fp32 width 8', 'sphere8', 32, 8, 'f32'),
            ('6-bit shells GOP 32 fp32 width 8', 'shell6', 32, 8, 'f32'), ('6-bit shells GOP 32 bf16 width 8', 'shell6', 32, 8, 'bf16'),
            ('6-bit shells GOP 32 width 16', 'shell6', 32, 16, 'f32'))
    if args.only:
        work = tuple(w for w in work if w[1] in args.only.split(','))
    gops = {}
    for name, config, n, hidden, tp in work:
        if (config, n) not in gops:
            if config == 'shell6':          # 2.1 - 2.8 k-row frames (radius 20 + t % 4): the step is launch- and host-bound
                clouds = [synthetic.sphere_shell(6, 20 + t % 4) for t in range(n)]
            else:
                clouds = [synthetic.sequence_frame_device(config, t, 'cuda') for t in range(n)]
            gops[(config, n)] = overfit.Gop(None, clouds, None, 64, 'cuda')
        gop = gops[(config, n)]
        times, state = {'loop': [], 'call': []}, {}
        for rep in range(args.runs + 1):
            for arm in ('loop', 'call'):
                model, opt = make(overfit, gop, hidden, tp, c_step=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                overfit.overfit_gop(model, opt, gop, args.epochs, c_loop=arm == 'call')
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rep:          # rep 0 is the warm-up
                    times[arm].append(dt)
                state[arm] = sha(model.flat_parameters(), opt.exp_avg, opt.exp_avg_sq) + ' lr %r t %d' % (opt.lr, opt.t)
        steps = args.epochs * n
        lines.append('%s, %d epochs (%d steps, %d rows in the largest frame)' % (name, args.epochs, steps, max(f.rows for f in gop.frames)))
        for arm in ('loop', 'call'):
            lines.append('  %-5s  s per overfit %s   ms per step %s' % (arm, spread(times[arm]), spread([1e3 * t / steps for t in times[arm]], '%.3f')))
        lines.append('  ' + verdict(times['loop'], times['call'], 'the Python loop', 'the one call'))
        lines.append('  state left behind: ' + ('identical (%s)' % state['loop'] if state['loop'] == state['call'] else
                                              'DIFFERENT: loop %s, call %s' % (state['loop'], state['call'])))
        lines.append('')
        print('\n'.join(lines[-6:]), flush=True)


def tree_hash(root):
    h = hashlib.sha256()
    for d, dirs, names in os.walk(root):
        dirs.sort()
        for n in sorted(names):
            p = os.path.join(d, n)
            h.update(os.path.relpath(p, root).encode() + b'\0')
            with open(p, 'rb') as f:
                h.update(f.read())
    return h.hexdigest()[:16]


VARIANTS = (('serial', []), ('serial-c', ['--c-overfit']), ('pipeline', ['--pipeline']), ('pipeline-c', ['--pipeline', '--c-overfit']))


def one_run(args, flags):
    out = tempfile.mkdtemp(prefix='overfit_c_ab_')
    try:
        cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, '-m', 'linr_pcgc_amd.run', '--config', 'loot10', '--frames',
               str(args.frames), '--gop', str(args.gop), '--first-epoch', str(args.epochs), '--others-epoch', str(args.epochs), '--out', out] + flags
        done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        if done.returncode != 0:
            return None, 'a child (%s) ended with status %d: %s' % (' '.join(flags), done.returncode, done.stderr[-400:].replace('\n', ' | '))
        summary = json.loads([ln for ln in done.stdout.splitlines() if ln.startswith('{')][-1])
        with open(os.path.join(out, 'results_rank0.json')) as f:
            results = json.load(f)
        return {'sec_per_frame': summary['sec_per_frame'], 'overfit_sum_s': sum(r['overfit_s'] for r in results.values()),
                'files': tree_hash(os.path.join(out, 'result_enc'))}, None
    finally:
        shutil.rmtree(out, ignore_errors=True)


def programs(args, lines):
    runs, failed = {v: [] for v, _ in VARIANTS}, None
    for rep in range(args.program_runs):
        for v, flags in VARIANTS:
            r, failed = one_run(args, flags)
            if failed:
                break
            runs[v].append(r)
            print(v, r, flush=True)
        if failed:
            break
    lines.append('run.py on loot10, %d frames in GOPs of %d, %d + %d epochs, %d runs of each variant, alternating, fresh processes' %
                 (args.frames, args.gop, args.epochs, args.epochs, args.program_runs))
    if failed:
        lines.append('  INCOMPLETE: ' + failed)
    for v, _ in VARIANTS:
        if runs[v]:
            lines.append('  %-11s ms per frame %s   overfit sum s %s   files %s' % (
                v, spread([1e3 * r['sec_per_frame'] for r in runs[v]], '%.2f'), spread([r['overfit_sum_s'] for r in runs[v]], '%.3f'),
                ','.join(sorted({r['files'] for r in runs[v]}))))
    if all(runs[v] for v, _ in VARIANTS):
        files = {r['files'] for v, _ in VARIANTS for r in runs[v]}
        lines.append('  encoded files: ' + ('the same in every run' if len(files) == 1 else 'DIFFERENT: %s' % sorted(files)))
        med = {v: statistics.median([r['overfit_sum_s'] for r in runs[v]]) for v, _ in VARIANTS}
        lines.append('  training beside the finish thread: Python loop %+.1f %%, one call %+.1f %% (overfit sum under --pipeline against serial, medians)'
                     % (100 * (med['pipeline'] / med['serial'] - 1), 100 * (med['pipeline-c'] / med['serial-c'] - 1)))
        for a, b in (('serial', 'serial-c'), ('pipeline', 'pipeline-c')):
            lines.append('  wall per frame, %s against %s: %s' % (a, b, verdict([r['sec_per_frame'] for r in runs[a]],
                                                                                   [r['sec_per_frame'] for r in runs[b]], a, b)))
            lines.append('  overfit sum,    %s against %s: %s' % (a, b, verdict([r['overfit_sum_s'] for r in runs[a]],
                                                                                   [r['overfit_sum_s'] for r in runs[b]], a, b)))
    lines.append('')
    return failed


def child_hashes(tree, timeout):
    done = subprocess.run(['timeout', '-k', '10', str(timeout), sys.executable, os.path.abspath(__file__), '--hashes'], cwd=tree,
                          env=dict(os.environ, PYTHONPATH=tree), capture_output=True, text=True)
    got = [ln for ln in done.stdout.splitlines() if ln.startswith('HASHES ')]
    if done.returncode != 0 or not got:
        return None, 'status %d: %s' % (done.returncode, done.stderr[-400:].replace('\n', ' | '))
    return json.loads(got[-1][7:]), None


def main():
    ap = argparse.ArgumentParser('overfit_c_ab')
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--program-runs', type=int, default=5)
    ap.add_argument('--epochs', type=int, default=10)
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--gop', type=int, default=32)
    ap.add_argument('--step-timeout', type=int, default=300)
    ap.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit: the default path must give its hashes')
    ap.add_argument('--skip-programs', action='store_true')
    ap.add_argument('--only', default=None, help='comma-separated configs of the in-process arms: loot10, sphere8, shell6')
    ap.add_argument('--hashes', action='store_true')
    ap.add_argument('--commit', default='the working tree')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.getcwd() if args.hashes else ROOT)
    if args.hashes:
        hashes()
        return 0
    lines = ['# One-call overfit A/B (tools/overfit_c_ab.py) on %s: loop = overfit_gop\'s Python loop, call = overfit_gop(c_loop=True)' % args.commit,
             '# (linr_overfit_gop).  Arms alternate in one session, one warm-up of each, then %d runs of each.  Cells: median [min .. max].' % args.runs, '']
    # A fault, an abort or the time limit of any GPU step - a child's status, or an exception of the in-process arms - ends the run:
    # nothing more is started on the GPU, what was measured so far is written, and the status is 1.
    failed = None
    if args.parent_tree:
        mine, failed = child_hashes(ROOT, args.step_timeout)
        theirs = None
        if not failed:
            theirs, failed = child_hashes(os.path.abspath(args.parent_tree), args.step_timeout)
        if failed:
            lines.append('default path against the parent commit: INCOMPLETE (the hash child of %s: %s)' % ('this tree' if mine is None else 'the parent tree', failed))
        else:
            lines.append('default path (no flag, no environment variable) against the parent commit, loot10 GOP 4, 2 epochs, sha256 of parameters, moments, losses:')
            for k in sorted(mine):
                lines.append('  %-5s %s  parent %s  %s' % (k, mine[k], theirs[k], 'equal' if mine[k] == theirs[k] else 'DIFFERENT'))
        lines.append('')
        print('\n'.join(lines), flush=True)
    if not failed:
        try:
            in_process(args, lines)
        except Exception as e:          # (a HIP error surfaces as one: the process starts nothing more)
            failed = 'the in-process arms ended with %s: %s' % (type(e).__name__, str(e)[:400])
            lines.append('INCOMPLETE: ' + failed)
    if not failed and not args.skip_programs:
        failed = programs(args, lines)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
