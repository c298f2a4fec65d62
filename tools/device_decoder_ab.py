"""A/B of the device range decoder (codec.decode_gop device_decoder=True) against the host decoders, one process, one GPU, all arms in
one session: the loot10 GOP of 32 frames that bench.py codes, model of seed 8807 trained --epochs epochs (default 10, so that the
streams have the entropy of real ones), coded with S in --chunks (default 0 16384 65536; 0 = plain streams).  Per S and per decoder:

  * decode_gop(workers=1)   - frame by frame, the latency arm;
  * decode_gop(workers=8)   - 8 frames in flight;
  * decode_gop(lockstep=32) - the whole GOP in lock step;

each after one warm-up (which is also the check that the geometry equals the input and the host path's), --runs timed runs (default 5)
with the arms alternating so that drift hits all alike; ms per frame behind decode_gop's once-per-GOP set-up: median (min .. max).
The baseline of a device arm is the host arm of the SAME run (the host path is the code the option does not touch); an arm is called
faster or slower only where the medians differ by more than the two min-max spreads together.

With --pipeline-runs N > 0 (default 0) the decode check of run.py follows, by tools/pipeline_ab.py's method - every run a fresh child
process of `python -m linr_pcgc_amd.run --decode`, serial and --pipeline, without and with --device-decoder, alternating, N of each:
the sum of the GOPs' decode_s (the decode check, which under --pipeline runs beside the next GOP's training), ms per frame of the run,
and the hash of result_enc/, which must be the same in all.  Measurement aid (profiles/device_decoder_ab.txt).

    python tools/device_decoder_ab.py [--gop 32] [--epochs 10] [--runs 5] [--chunks 0 16384 65536] [--out profiles/device_decoder_ab.txt]
                                      [--pipeline-runs 3 --pipeline-frames 96 --pipeline-chunk 16384]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch  # noqa: E402

from linr_pcgc_amd import codec, overfit, synthetic  # noqa: E402
from linr_pcgc_amd.model_core import FlatAdam  # noqa: E402


def stats(t):
    return statistics.median(t), min(t), max(t)


def verdict(arm, base):
    """arm against base (lists of times): faster / slower only beyond the two spreads together."""
    (m, lo, hi), (m0, lo0, hi0) = stats(arm), stats(base)
    both = (hi - lo) + (hi0 - lo0)
    if abs(m0 - m) <= both:
        return 'not separated (difference %.3f, spreads together %.3f)' % (m0 - m, both)
    return '%s by %.3f (%.2fx), spreads together %.3f' % ('faster' if m < m0 else 'SLOWER', abs(m0 - m), m0 / m, both)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='loot10')
    ap.add_argument('--gop', type=int, default=32)
    ap.add_argument('--epochs', type=int, default=10)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--chunks', type=int, nargs='*', default=[0, 16384, 65536])
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--pipeline-runs', type=int, default=0)
    ap.add_argument('--pipeline-frames', type=int, default=96)
    ap.add_argument('--pipeline-chunk', type=int, default=16384)
    ap.add_argument('--step-timeout', type=int, default=300, help='seconds one run.py child may take')
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    n = args.gop
    n_cpu = len(os.sched_getaffinity(0))
    n_threads = max(1, min(16, n_cpu))
    torch.set_num_threads(4)
    say('# device range decoder A/B (tools/device_decoder_ab.py): %s, GOP of %d frames, %d epochs; %d usable cpus, %d host coder threads; %s'
        % (args.config, n, args.epochs, n_cpu, n_threads, torch.cuda.get_device_name(0)))
    if args.runs > 0:          # (--runs 0: the run.py part alone)
        clouds = [synthetic.sequence_frame_device(args.config, t, 'cuda') for t in range(n)]
        gop = overfit.Gop(None, clouds, None, 64, 'cuda')
        del clouds
        model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807)
        if args.epochs:
            say('# trained %d epochs: %.3f bpp' % (args.epochs, min(overfit.overfit_gop(model, FlatAdam(model), gop, args.epochs))))
        shell = lambda: overfit.gen_model(gop.scale_num, 'cuda')                         # noqa: E731
        truth = [torch.as_tensor(gop.infos[i]['ori']).cuda() + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32) for i in range(n)]
        f0 = gop.frames[0]
        say('# %d points; frame 0: %d rows, scales of %s rows' % (sum(gop.point_nums), f0.rows, [int(f0.row_off[i + 1] - f0.row_off[i]) for i in range(f0.n_scales)]))
        encs = {S: codec.encode_gop(model, shell(), gop, 8, n_threads=n_threads, stream_chunk=S) for S in args.chunks}

        modes = [('workers=1', {'workers': 1}), ('workers=8', {'workers': 8}), ('lockstep=%d' % min(32, n), {'lockstep': min(32, n)})]
        arms = [(S, mode, kw, dev) for S in args.chunks for mode, kw in modes for dev in (False, True)]

        def decode(S, kw, dev):
            """(ms per frame behind the once-per-GOP set-up, the decoded frames)"""
            timing = {}
            torch.cuda.synchronize()
            t0 = time.time()
            dec = codec.decode_gop(shell(), encs[S], 'cuda', timing=timing, n_threads=n_threads, device_decoder=dev, **kw)
            torch.cuda.synchronize()
            return (time.time() - t0 - timing['setup_s']) * 1e3 / n, dec

        for S, mode, kw, dev in arms:                                                     # warm-up and the geometry
            _, dec = decode(S, kw, dev)
            if len(dec) != n or not all(torch.equal(a, b) for a, b in zip(dec, truth)):
                say('S = %d, %s, device_decoder=%s: does NOT decode to the input' % (S, mode, dev))
                return 1
        say('# every arm decodes every frame to the input (and so to what the host path decodes)')
        times = {(S, mode, dev): [] for S, mode, _, dev in arms}
        for _ in range(args.runs):
            for S, mode, kw, dev in arms:
                times[S, mode, dev].append(decode(S, kw, dev)[0])
        say('decode_gop, ms per frame behind the set-up: median (min .. max) of %d runs; host = device_decoder=False, the unchanged path' % args.runs)
        for S in args.chunks:
            for mode, _ in modes:
                h, d = times[S, mode, False], times[S, mode, True]
                say('  S = %6d  %-12s host %8.3f (%8.3f .. %8.3f)   device %8.3f (%8.3f .. %8.3f)   device is %s'
                    % ((S, mode) + stats(h) + stats(d) + (verdict(d, h),)))

    rc = 0
    if args.pipeline_runs > 0:
        import pipeline_ab
        torch.cuda.empty_cache()
        pa = argparse.Namespace(config=args.config, frames=args.pipeline_frames, gop=args.gop, epochs=args.epochs, step_timeout=args.step_timeout)
        chunk = ['--stream-chunk', str(args.pipeline_chunk)] if args.pipeline_chunk else []
        variants = [('serial, host', chunk), ('serial, device', chunk + ['--device-decoder']),
                    ('pipeline, host', chunk + ['--pipeline']), ('pipeline, device', chunk + ['--pipeline', '--device-decoder'])]
        runs, failed = [], None
        for _ in range(args.pipeline_runs):
            for name, flags in variants:
                r, failed = pipeline_ab.one_run(pa, name, flags, True)
                if failed:          # a fault, an abort or the time limit: nothing more is started on the GPU
                    break
                runs.append(r)
                print(r, flush=True)
            if failed:
                break
        say('')
        say('## the decode check of run.py --decode (tools/pipeline_ab.py\'s method): %d frames in GOPs of %d, %d + %d epochs, --stream-chunk %d, '
            '%d fresh child processes of each variant, alternating' % (args.pipeline_frames, args.gop, args.epochs, args.epochs, args.pipeline_chunk,
                                                                       args.pipeline_runs))
        if failed:
            say('# INCOMPLETE: %s' % failed)
            rc = 1
        say('  variant            runs  sum of decode_s: median (min .. max)   ms per frame of the run: median (min .. max)')
        for name, _ in variants:
            v = [r for r in runs if r['variant'] == name]
            if v:
                say('  %-17s  %4d  %8.3f (%8.3f .. %8.3f)              %8.3f (%8.3f .. %8.3f)'
                    % ((name, len(v)) + stats([r['decode_sum_s'] for r in v]) + stats([1e3 * r['sec_per_frame'] for r in v])))
        for a, b in (('serial, device', 'serial, host'), ('pipeline, device', 'pipeline, host')):
            va, vb = [r['decode_sum_s'] for r in runs if r['variant'] == a], [r['decode_sum_s'] for r in runs if r['variant'] == b]
            if va and vb:
                say('  decode_s, %s against %s: %s' % (a, b, verdict(va, vb)))
        for kind in ('host', 'device'):
            vs = [r['decode_sum_s'] for r in runs if r['variant'] == 'serial, ' + kind]
            vp = [r['decode_sum_s'] for r in runs if r['variant'] == 'pipeline, ' + kind]
            if vs and vp:
                say('  %s decoder: the check beside a training GOP takes %.2fx as long as alone (medians)' % (kind, statistics.median(vp) / statistics.median(vs)))
        if runs:
            say('  files under result_enc/ the same in all runs: %s; lossless in all runs: %s'
                % ('yes' if len({r['files'] for r in runs}) == 1 else 'NO', 'yes' if all(r['lossless'] is True for r in runs) else 'NO'))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return rc


if __name__ == '__main__':
    sys.exit(main())
