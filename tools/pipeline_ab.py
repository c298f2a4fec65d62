"""Does run.py --pipeline hide the serial tail of a GOP (codec forward, range coding, file writes, the decode check) under the next GOP's
training?  BASELINE config[2] on one GPU - 300 loot10 frames in GOPs of 32, 10 + 10 epochs - as the program itself
(python -m linr_pcgc_amd.run), every run a fresh child process that starts with nothing resident:

  serial | --pipeline,   alternating, --runs of each (default 3), once without --decode and once with it.

Per run: sec_per_frame, the sum of the GOPs' overfit_s (how much training slows down beside the finish thread), finish_wait_s,
gpu_train_fraction (for a serial run: the same ratio, sum of overfit_s over the wall) and a hash of everything under result_enc/ -
both variants must leave the same files.  The report gives every run and the medians with their spread; a difference counts
only if the medians differ by more than the spread of the runs on either side.

  python tools/pipeline_ab.py [--runs 3] [--frames 300] [--gop 32] [--epochs 10] [--out profiles/gop_pipeline.txt]
                              [--step-timeout 300] [--commit TEXT]

Every child is a GPU step of its own under `timeout`; the first one that fails ends the run (nothing more is started on the GPU) and
what was measured so far is reported.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = (('serial', []), ('pipeline', ['--pipeline']))


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


def one_run(args, variant, flags, decode):
    out = tempfile.mkdtemp(prefix='pipeline_ab_')
    try:
        cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, '-m', 'linr_pcgc_amd.run', '--config', args.config,
               '--frames', str(args.frames), '--gop', str(args.gop), '--first-epoch', str(args.epochs), '--others-epoch', str(args.epochs),
               '--out', out] + flags + (['--decode'] if decode else [])
        done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        if done.returncode != 0:
            return None, 'the %s child (decode=%s) ended with status %d: %s' % (variant, decode, done.returncode, done.stderr[-400:].replace('\n', ' | '))
        summary = json.loads([ln for ln in done.stdout.splitlines() if ln.startswith('{')][-1])
        with open(os.path.join(out, 'results_rank0.json')) as f:
            results = json.load(f)
        overfit = sum(r['overfit_s'] for r in results.values())
        return {'variant': variant, 'decode': decode, 'sec_per_frame': summary['sec_per_frame'], 'wall_s': summary['wall_s'],
                'overfit_sum_s': round(overfit, 4), 'encode_sum_s': round(sum(r['encode_s'] for r in results.values()), 4),
                'decode_sum_s': round(sum(r['decode_s'] for r in results.values()), 4),
                'finish_wait_s': summary.get('finish_wait_s'), 'gpu_train_fraction': summary.get('gpu_train_fraction', round(overfit / summary['wall_s'], 4)),
                'phase_b_efficiency': summary['phase_b_efficiency'], 'bits_per_point': summary['bits_per_point'], 'lossless': summary['lossless'],
                'files': tree_hash(os.path.join(out, 'result_enc'))}, None
    finally:
        shutil.rmtree(out, ignore_errors=True)


def spread(xs, scale=1.0, fmt='%.3f'):
    xs = sorted(x * scale for x in xs if x is not None)
    if not xs:
        return '-'
    return (fmt + '  [' + fmt + ' .. ' + fmt + ']') % (statistics.median(xs), xs[0], xs[-1])


def report(args, runs, failed):
    lines = ['# GOP pipeline A/B (tools/pipeline_ab.py) on %s: %s, %d frames in GOPs of %d, %d + %d epochs, one GPU, %d runs of each variant,' %
             (args.commit, args.config, args.frames, args.gop, args.epochs, args.epochs, args.runs),
             '# alternating, every run a fresh process.  serial = the plain flow; pipeline = run.py --pipeline.  Cells: median [min .. max].']
    if failed:
        lines.append('# INCOMPLETE: %s' % failed)
    for decode in (False, True):
        rs = [r for r in runs if r['decode'] == decode]
        if not rs:
            continue
        lines += ['', '## %s' % ('with --decode (every frame decoded from the files and compared)' if decode else 'without --decode'),
                  '  variant        runs  ms per frame               sum overfit_s              finish_wait_s              gpu_train_fraction']
        for variant, _ in VARIANTS:
            v = [r for r in rs if r['variant'] == variant]
            if v:
                lines.append('  %-13s  %4d  %s  %s  %s  %s' % (variant, len(v), spread([r['sec_per_frame'] for r in v], 1e3),
                                                              spread([r['overfit_sum_s'] for r in v]), spread([r['finish_wait_s'] for r in v]),
                                                              spread([r['gpu_train_fraction'] for r in v], fmt='%.4f')))
        lines.append('  every run (in the order they ran): variant  ms/frame  wall_s  overfit  encode  decode  wait  train_fraction  phase_b_eff  files')
        for r in rs:
            lines.append('    %-13s %7.3f  %7.3f  %7.3f  %6.3f  %6.3f  %s  %.4f  %s  %s' % (
                r['variant'], 1e3 * r['sec_per_frame'], r['wall_s'], r['overfit_sum_s'], r['encode_sum_s'], r['decode_sum_s'],
                '%6.3f' % r['finish_wait_s'] if r['finish_wait_s'] is not None else '     -', r['gpu_train_fraction'], r['phase_b_efficiency'], r['files']))
        same = len({r['files'] for r in rs}) == 1 and len({r['bits_per_point'] for r in rs}) == 1
        lines.append('  files under result_enc/ and bits_per_point the same in all runs: %s' % ('yes' if same else 'NO'))
        if decode:
            lines.append('  lossless in all runs: %s' % ('yes' if all(r['lossless'] is True for r in rs) else 'NO'))
        base = sorted(r['sec_per_frame'] for r in rs if r['variant'] == 'serial')
        for variant in [name for name, _ in VARIANTS[1:]]:
            v = sorted(r['sec_per_frame'] for r in rs if r['variant'] == variant)
            if base and v:
                clear = v[-1] < base[0] or base[-1] < v[0]          # the medians differ by more than either side's spread: no overlap
                lines.append('  %s against serial: median %+.1f %%, the two ranges %s' % (
                    variant, 100.0 * (statistics.median(v) / statistics.median(base) - 1.0), 'do not overlap' if clear else 'OVERLAP: no difference shown'))
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='loot10')
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--gop', type=int, default=32)
    ap.add_argument('--epochs', type=int, default=10)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gop_pipeline.txt'))
    ap.add_argument('--step-timeout', type=int, default=300, help='seconds one child may take')
    ap.add_argument('--commit', default=None, help='what the report says it was run on (default: git rev-parse HEAD)')
    ap.add_argument('--decode-modes', nargs='+', default=['off', 'on'], choices=['off', 'on'])
    args = ap.parse_args()
    if args.commit is None:
        try:
            args.commit = 'commit ' + subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except (OSError, subprocess.CalledProcessError):
            args.commit = 'an unknown commit'
    runs, failed = [], None
    for decode in [m == 'on' for m in args.decode_modes]:
        for _ in range(args.runs):
            for variant, flags in VARIANTS:
                r, failed = one_run(args, variant, flags, decode)
                if failed:          # a fault, an abort or the time limit: nothing more is started on the GPU
                    break
                runs.append(r)
                print(json.dumps(r), flush=True)
            if failed:
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
