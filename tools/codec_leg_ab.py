"""A/B of the codec leg's encoder with and without device-side code values (codec.encode_gop(device_codes=...)).

Stages one GOP of a synthetic configuration as bench/headline.py does (default: loot10, 32 frames, untrained model of seed 8807:
the stream sizes differ from a trained model's, the symbol counts and copies do not), checks that both paths give the same
streams, then times encode_gop 5 times each after one warm-up, alternating the two paths so that drift hits both alike.  Also
reports the host-only coder time of frame 0 (the batch entries on buffers already in host memory) and the bytes copied to the
host per frame.  Measurement aid (profiles/device_codes_ab.txt).

    python tools/codec_leg_ab.py [--config loot10] [--gop 32] [--runs 5]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from linr_pcgc_amd import codec, overfit, synthetic  # noqa: E402
from linr_pcgc_amd.model_codec import Model_Estimate  # noqa: E402
from linr_pcgc_amd.model_core import codes_word_off, encode_streams, encode_streams_codes  # noqa: E402


def cpu_model():
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='loot10')
    ap.add_argument('--gop', type=int, default=32)
    ap.add_argument('--runs', type=int, default=5)
    args = ap.parse_args()
    n_cpu = len(os.sched_getaffinity(0))
    n_threads = max(1, min(16, n_cpu))
    print('cpu: %s; %d usable, %d coder threads; gpu: %s' % (cpu_model(), n_cpu, n_threads, torch.cuda.get_device_name(0)))
    clouds = [synthetic.sequence_frame_device(args.config, t, 'cuda') for t in range(args.gop)]
    gop = overfit.Gop(None, clouds, None, 64, 'cuda')
    del clouds
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807)
    shell = overfit.gen_model(gop.scale_num, 'cuda')
    rows = [f.rows for f in gop.frames]
    words = [int(codes_word_off(f.row_off)[-1]) for f in gop.frames]
    print('%s: %d frames, frame 0: %d points, %d rows, %d scales' % (args.config, len(gop), gop.point_nums[0], rows[0], gop.scale_num))
    b_def, b_dev = 8 * 5 * np.mean(rows), 8 * (2 * np.mean(rows) + 4 * np.mean(words))
    print('bytes to the host per frame: default %.0f (fp32 probability + symbol byte), device codes %.0f (uint16 code value + '
          'symbol bit planes): %.3f of it' % (b_def, b_dev, b_dev / b_def))

    def encode(dc):
        torch.cuda.synchronize()
        t0 = time.time()
        enc = codec.encode_gop(model, shell, gop, 8, n_threads=n_threads, device_codes=dc)
        torch.cuda.synchronize()
        return time.time() - t0, enc

    _, e0 = encode(False)                                    # warm-up of both paths, and the identity check
    _, e1 = encode(True)
    same = e0['frames'] == e1['frames']
    print('streams identical: %s (%d bytes)' % (same, sum(len(b) for fb in e0['frames'] for b in fb)))
    times = {False: [], True: []}
    for _ in range(args.runs):
        for dc in (False, True):
            times[dc].append(encode(dc)[0])
    for dc, name in ((False, 'default     '), (True, 'device codes')):
        t = times[dc]
        print('encode_gop %s: median %.2f ms/frame, min %.2f, max %.2f; runs (s/GOP): %s'
              % (name, 1e3 * statistics.median(t) / len(gop), 1e3 * min(t) / len(gop), 1e3 * max(t) / len(gop), ' '.join('%.4f' % v for v in t)))
    m0, m1 = statistics.median(times[False]), statistics.median(times[True])
    spread = max(max(t) - min(t) for t in times.values())
    print('difference of the medians: %.2f ms/frame (default - device codes); largest run-to-run spread %.2f ms/frame -> %s'
          % (1e3 * (m0 - m1) / len(gop), 1e3 * spread / len(gop),
             'device codes faster beyond the spread' if m0 - m1 > spread else 'NOT faster beyond the spread'))

    # host-only coder time of frame 0: the batch entries on buffers already in host memory, 8 threads (what one frame gets in encode_gop)
    coded = Model_Estimate().compress_model(model, 8, True, shell)['new_model']
    f = gop.frames[0]
    probs, _ = coded.frame_probs(f)
    c1, sym, _ = coded.frame_codes(f)
    p_h, o_h = probs.cpu().numpy(), f.occ.t().contiguous().cpu().numpy().astype(np.uint8)
    c_h, s_h = c1.cpu().numpy(), sym.cpu().numpy()
    woff = codes_word_off(f.row_off)
    ps, ss, cs, ws, ns = [], [], [], [], []
    for i in range(f.n_scales):
        a, b = int(f.row_off[i]), int(f.row_off[i + 1])
        for k in range(8):
            ps.append(p_h[k, a:b]); ss.append(o_h[k, a:b]); cs.append(c_h[k, a:b]); ws.append(s_h[k, woff[i]:woff[i + 1]]); ns.append(b - a)
    per = max(1, n_threads // 2)
    host = {'default': [], 'device codes': []}
    for _ in range(args.runs + 1):
        t0 = time.time(); r0 = encode_streams(ps, ss, per); t1 = time.time(); r1 = encode_streams_codes(cs, ws, ns, per); t2 = time.time()
        host['default'].append(t1 - t0); host['device codes'].append(t2 - t1)
    print('host-only coder, frame 0, %d threads (identical: %s): %s'
          % (per, r0 == r1, '; '.join('%s median %.2f ms (runs %s)' % (k, 1e3 * statistics.median(v[1:]), ' '.join('%.2f' % (1e3 * x) for x in v[1:]))
                                      for k, v in host.items())))
    if not same or r0 != r1:
        sys.exit(1)


if __name__ == '__main__':
    main()
