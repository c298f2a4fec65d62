"""A/B of chunked stage streams (codec.encode_gop stream_chunk=S, side_info.json's stream_chunk) against the plain streams, one process,
one GPU: the loot10 GOP of 32 frames that bench.py codes, model of seed 8807 trained --epochs epochs (default 10, so that the streams
have the entropy of real ones), for S in --chunks (default 0 16384 65536 262144; 0 = the plain streams, the path this option does not
touch).  Per S:
  * the bytes of all frame streams and the difference in bpp_all against S = 0 (exact, deterministic), and the chunks per frame;
  * the codec leg (encode_gop, ms per frame) on the default path, with device_codes and with device_coder at coder_group 32: one
    warm-up each - which also checks that the three write the same streams -, then --runs timed runs, the arms and the chunk sizes
    alternating so that drift hits all alike; median, min, max;
  * the decode of ONE frame (decode_gop(frames=[0], workers=1, n_threads=t)) for t in 1, 4, 8, 16: median, min, max in ms;
  * the decode of the whole GOP with 8 frames in flight (decode_gop(workers=8)), ms per frame;
    both without decode_gop's once-per-GOP set-up (model.bin -> parameters; its timing['setup_s']);
every decode checked lossless.  An arm is called faster than its S = 0 arm only where the medians differ by more than the two
min-max spreads together.  Measurement aid (profiles/stream_chunks.txt).

    python tools/stream_chunks_ab.py [--gop 32] [--epochs 10] [--runs 5] [--chunks 0 16384 65536 262144]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from linr_pcgc_amd import codec, overfit, synthetic  # noqa: E402
from linr_pcgc_amd.model_core import FlatAdam  # noqa: E402
from linr_pcgc_amd.stream_chunks import chunk_count  # noqa: E402


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
    ap.add_argument('--chunks', type=int, nargs='*', default=[0, 16384, 65536, 262144])
    ap.add_argument('--coder-group', type=int, default=32)
    args = ap.parse_args()
    if 0 not in args.chunks:
        args.chunks = [0] + args.chunks
    n = args.gop
    n_cpu = len(os.sched_getaffinity(0))
    n_threads = max(1, min(16, n_cpu))
    torch.set_num_threads(4)
    print('%d usable cpus, %d coder threads; gpu: %s' % (n_cpu, n_threads, torch.cuda.get_device_name(0)))
    clouds = [synthetic.sequence_frame_device(args.config, t, 'cuda') for t in range(n)]
    gop = overfit.Gop(None, clouds, None, 64, 'cuda')
    del clouds
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807)
    if args.epochs:
        print('trained %d epochs: %.3f bpp' % (args.epochs, min(overfit.overfit_gop(model, FlatAdam(model), gop, args.epochs))))
    shell = lambda: overfit.gen_model(gop.scale_num, 'cuda')                         # noqa: E731
    truth = [torch.as_tensor(gop.infos[i]['ori']).cuda() + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32) for i in range(n)]
    f0 = gop.frames[0]
    ns = [int(f0.row_off[i + 1] - f0.row_off[i]) for i in range(f0.n_scales)]
    print('%s: %d frames, %d points; frame 0: %d rows, scales of %s rows' % (args.config, n, sum(gop.point_nums), f0.rows, ns))

    arms = [('default', {}), ('device codes', {'device_codes': True}),
            ('device coder, group %d' % args.coder_group, {'device_coder': True, 'coder_group': args.coder_group})]

    def encode(S, kw):
        torch.cuda.synchronize()
        t0 = time.time()
        enc = codec.encode_gop(model, shell(), gop, 8, n_threads=n_threads, stream_chunk=S, **kw)
        torch.cuda.synchronize()
        return (time.time() - t0) * 1e3 / n, enc

    # ---- rate (exact) and the identity of the three coders ------------------------------------------------------------------------
    encs = {}
    for S in args.chunks:
        got = [encode(S, kw)[1] for _, kw in arms]                                   # the warm-up of every arm, too
        same = all(e['frames'] == got[0]['frames'] and e['side_info'] == got[0]['side_info'] for e in got[1:])
        encs[S] = got[0]
        nbytes = sum(len(b) for fb in got[0]['frames'] for b in fb)
        base = encs[0]
        print('S = %7d: %9d stream bytes (%+d against S = 0), bpp_all %.6f (%+.6f, %+.4f %%), %d chunks in frame 0 (%d streams); the three '
              'coders identical: %s' % (S, nbytes, nbytes - sum(len(b) for fb in base['frames'] for b in fb), got[0]['bpp']['bpp_all'],
                                        got[0]['bpp']['bpp_all'] - base['bpp']['bpp_all'],
                                        100 * (got[0]['bpp']['bpp_all'] / base['bpp']['bpp_all'] - 1), 8 * sum(chunk_count(m, S) for m in ns),
                                        8 * len(ns), same))
        if not same:
            sys.exit(1)
        del got

    # ---- the codec leg -------------------------------------------------------------------------------------------------------------
    times = {(S, name): [] for S in args.chunks for name, _ in arms}
    for _ in range(args.runs):
        for name, kw in arms:
            for S in args.chunks:
                times[S, name].append(encode(S, kw)[0])
    print('codec leg, encode_gop ms per frame: median (min .. max) of %d runs' % args.runs)
    for name, _ in arms:
        for S in args.chunks:
            m, lo, hi = stats(times[S, name])
            print('  %-24s S = %7d: %7.3f (%7.3f .. %7.3f)%s' % (name, S, m, lo, hi, '' if S == 0 else '  ' + verdict(times[S, name], times[0, name])))

    # ---- decode -------------------------------------------------------------------------------------------------------------------
    def decode(S, **kw):
        """(ms behind the once-per-GOP set-up - model.bin -> parameters, the coarsest coordinates -, the decoded frames)"""
        timing = {}
        torch.cuda.synchronize()
        t0 = time.time()
        dec = codec.decode_gop(shell(), encs[S], 'cuda', timing=timing, **kw)
        torch.cuda.synchronize()
        return (time.time() - t0 - timing['setup_s']) * 1e3, dec

    single = {}
    threads = [t for t in (1, 4, 8, 16) if t == 1 or t <= n_threads]
    for S in args.chunks:
        for t in threads:
            _, dec = decode(S, frames=[0], workers=1, n_threads=t)
            if not torch.equal(dec[0], truth[0]):
                print('S = %d, %d threads: frame 0 does NOT decode to the input' % (S, t))
                sys.exit(1)
    for _ in range(args.runs):
        for S in args.chunks:
            for t in threads:
                single.setdefault((S, t), []).append(decode(S, frames=[0], workers=1, n_threads=t)[0])
    print('decode of ONE frame (frame 0, behind the once-per-GOP set-up), ms: median (min .. max) of %d runs; S = 0 is the plain path, where the '
          'thread count has nothing to divide' % args.runs)
    for S in args.chunks:
        for t in threads:
            m, lo, hi = stats(single[S, t])
            print('  S = %7d, %2d threads: %7.3f (%7.3f .. %7.3f)%s' % (S, t, m, lo, hi, '' if S == 0 else '  ' + verdict(single[S, t], single[0, 1])))
    flight = {}
    for S in args.chunks:
        _, dec = decode(S, workers=8)
        if not all(torch.equal(a, b) for a, b in zip(dec, truth)):
            print('S = %d: the GOP does NOT decode to the input' % S)
            sys.exit(1)
    for _ in range(args.runs):
        for S in args.chunks:
            flight.setdefault(S, []).append(decode(S, workers=8)[0] / n)
    print('decode of the GOP, 8 frames in flight (decode_gop(workers=8); %d threads per frame with chunks), ms per frame' % max(1, n_threads // 8))
    for S in args.chunks:
        m, lo, hi = stats(flight[S])
        print('  S = %7d: %7.3f (%7.3f .. %7.3f)%s' % (S, m, lo, hi, '' if S == 0 else '  ' + verdict(flight[S], flight[0])))


if __name__ == '__main__':
    main()
