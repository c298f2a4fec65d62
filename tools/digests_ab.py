"""A/B of self-checking streams (run.py --digests; codec.encode_gop digests=True, codec.decode_gop verify=True) on one GPU, all arms in
one session: the loot10 GOP of 32 frames that bench.py codes, model of seed 8807 trained --epochs epochs (default 10).  Arms:

  * P - a checkout of the parent commit, built beside this one (--parent DIR: its root; without it the arm is left out);
  * 0 - this tree without digests (the default path, which is supposed to be the parent's);
  * D - this tree with digests and verification.

Two builds of the package cannot live in one process, so every measurement is a fresh child process of this file (--worker) with the
arm's tree in front of sys.path: it stages and trains the GOP, warms every path up once (which is also the check that the geometry
equals the input) and times once each: the codec leg (encode_gop, ms per frame) and decode_gop behind its once-per-GOP set-up at
workers=1, workers=8 and lockstep=32 (ms per frame).  The children run P, 0, D, P, 0, D, ... --runs times (default 5) so that drift
hits all alike; reported: median (min .. max), and an arm is called faster or slower than P only where the medians differ by more than
the two min-max spreads together ("not separated" otherwise).  Arm D's children also bracket the digest kernels themselves with
events: the encoder's launches of the whole GOP (codec.gop_digests_launch) and one call on the finest level of frame 0.
A child that faults, aborts or runs into its time limit ends the session: nothing more is started on the GPU.
Measurement aid (profiles/digests.txt).

    python tools/digests_ab.py [--parent DIR] [--gop 32] [--epochs 10] [--runs 5] [--out profiles/digests.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(t):
    return statistics.median(t), min(t), max(t)


def verdict(arm, base):
    """arm against base (lists of times): faster / slower only beyond the two spreads together."""
    (m, lo, hi), (m0, lo0, hi0) = stats(arm), stats(base)
    both = (hi - lo) + (hi0 - lo0)
    if abs(m0 - m) <= both:
        return 'not separated (difference %+.3f, spreads together %.3f)' % (m - m0, both)
    return '%s by %.3f (%.2fx), spreads together %.3f' % ('faster' if m < m0 else 'SLOWER', abs(m0 - m), m / m0, both)


def worker(args):
    """One arm's measurement in this process; prints one JSON line."""
    sys.path.insert(0, args.root)
    import torch
    from linr_pcgc_amd import codec, overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam
    assert os.path.dirname(os.path.dirname(os.path.abspath(codec.__file__))) == os.path.abspath(args.root)
    digests = args.worker == 'D'
    n = args.gop
    n_threads = max(1, min(16, len(os.sched_getaffinity(0))))
    torch.set_num_threads(4)
    gop = overfit.Gop(None, [synthetic.sequence_frame_device(args.config, t, 'cuda') for t in range(n)], None, 64, 'cuda')
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807)
    if args.epochs:
        overfit.overfit_gop(model, FlatAdam(model), gop, args.epochs)
    shell = lambda: overfit.gen_model(gop.scale_num, 'cuda')                         # noqa: E731
    truth = [torch.as_tensor(gop.infos[i]['ori']).cuda() + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32) for i in range(n)]
    enc_kw = {'digests': True} if digests else {}

    def encode():
        torch.cuda.synchronize()
        t0 = time.time()
        enc = codec.encode_gop(model, shell(), gop, 8, n_threads=n_threads, **enc_kw)
        torch.cuda.synchronize()
        return (time.time() - t0) * 1e3 / n, enc

    def decode(enc, kw):
        timing = {}
        torch.cuda.synchronize()
        t0 = time.time()
        dec = codec.decode_gop(shell(), enc, 'cuda', timing=timing, n_threads=n_threads, **kw)
        torch.cuda.synchronize()
        return (time.time() - t0 - timing['setup_s']) * 1e3 / n, dec

    modes = [('workers=1', {'workers': 1}), ('workers=8', {'workers': 8}), ('lockstep=%d' % min(32, n), {'lockstep': min(32, n)})]
    _, enc = encode()                                                                  # warm-up and the geometry
    for _, kw in modes:
        dec = decode(enc, kw)[1]
        if len(dec) != n or not all(torch.equal(a, b) for a, b in zip(dec, truth)):
            print(json.dumps({'error': 'does not decode to the input'}))
            return 1
    out = {'arm': args.worker, 'points': sum(gop.point_nums), 'bpp_all': enc['bpp']['bpp_all'],
           'stream_bytes': sum(len(b) for f in enc['frames'] for b in f), 'digests_bytes': len(enc.get('digests_bin') or b''),
           'digest_bits': enc.get('digest_bits', 0), 'scales': len(enc['frames'][0]), 'codec_ms': encode()[0]}
    for name, kw in modes:
        out[name] = decode(enc, kw)[0]
    if digests:
        from linr_pcgc_amd import ops
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        codec.gop_digests_launch(gop)
        torch.cuda.synchronize()
        a.record()
        codec.gop_digests_launch(gop)
        b.record()
        torch.cuda.synchronize()
        out['kernels_gop_ms_per_frame'] = a.elapsed_time(b) / n
        finest = gop.infos[0]['all_input_info'][0]['ground_truth']
        ops.coords_digest(finest, origins=[gop.coord_mins[0]])
        torch.cuda.synchronize()
        a.record()
        for _ in range(20):
            ops.coords_digest(finest, origins=[gop.coord_mins[0]])
        b.record()
        torch.cuda.synchronize()
        out['kernels_finest_us'] = a.elapsed_time(b) * 1e3 / 20
        out['finest_rows'] = int(finest.shape[0])
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='loot10')
    ap.add_argument('--gop', type=int, default=32)
    ap.add_argument('--epochs', type=int, default=10)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--parent', default=None, help='root of a built checkout of the parent commit (arm P)')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--step-timeout', type=int, default=240, help='seconds one child may take')
    ap.add_argument('--worker', default=None, choices=['P', '0', 'D'], help=argparse.SUPPRESS)
    ap.add_argument('--root', default=HERE, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    arms = ([('P', os.path.abspath(args.parent))] if args.parent else []) + [('0', HERE), ('D', HERE)]
    say('# self-checking streams A/B (tools/digests_ab.py): %s, GOP of %d frames, %d epochs, %d runs of each arm, every run a fresh process; arms %s'
        % (args.config, args.gop, args.epochs, args.runs, ' '.join(a for a, _ in arms)))
    if not args.parent:
        say('# no --parent: arm P (a build of the parent commit) was NOT measured')
    got, failed = {a: [] for a, _ in arms}, None
    for _ in range(args.runs):
        for arm, root in arms:
            try:
                done = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', arm, '--root', root, '--config', args.config,
                                       '--gop', str(args.gop), '--epochs', str(args.epochs)], capture_output=True, text=True,
                                      timeout=args.step_timeout, cwd=root)
            except subprocess.TimeoutExpired:
                failed = 'arm %s ran into its time limit of %d s' % (arm, args.step_timeout)
                break
            last = [ln for ln in done.stdout.splitlines() if ln.startswith('{')]
            if done.returncode != 0 or not last or 'error' in json.loads(last[-1]):
                failed = 'arm %s ended with status %d: %s' % (arm, done.returncode, (last[-1] if last else done.stderr[-600:]))
                break
            got[arm].append(json.loads(last[-1]))
            print(last[-1], flush=True)
        if failed:          # a fault, an abort or the time limit: nothing more is started on the GPU
            say('# INCOMPLETE: %s' % failed)
            break
    keys = ['codec_ms', 'workers=1', 'workers=8', 'lockstep=%d' % min(32, args.gop)]
    say('ms per frame, median (min .. max); codec_ms = encode_gop, the others decode_gop behind its set-up')
    for key in keys:
        for arm, _ in arms:
            v = [r[key] for r in got[arm]]
            if not v:
                continue
            base = [r[key] for r in got[arms[0][0]]]
            say('  %-12s arm %s  %8.3f (%8.3f .. %8.3f)%s' % ((key, arm) + stats(v) + (
                '' if arm == arms[0][0] or not base else '   against %s: %s' % (arms[0][0], verdict(v, base)),)))
    d = got['D']
    if d:
        r = d[0]
        z = got['0'][0] if got['0'] else None
        say('rate: digests.bin %d bytes (%d frames x %d scales x 4), %d bits with the field, beside %d stream bytes: +%.4f %%; bpp_all %.6f%s'
            % (r['digests_bytes'], args.gop, r['scales'], r['digest_bits'], r['stream_bytes'], 100.0 * r['digest_bits'] / (8 * r['stream_bytes']),
               r['bpp_all'], '' if z is None else ' against %.6f without' % z['bpp_all']))
        say('digest kernels by event brackets: the encoder\'s launches of the GOP %.4f ms per frame (median; %.4f .. %.4f); one call on the finest '
            'level (%d rows, launch pair) %.2f us (median; %.2f .. %.2f)'
            % (stats([x['kernels_gop_ms_per_frame'] for x in d]) + (r['finest_rows'],) + stats([x['kernels_finest_us'] for x in d])))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
