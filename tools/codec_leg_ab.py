"""A/B of the codec leg's encoder: the default path, device-side code values (codec.encode_gop(device_codes=True)) and the device
range coder (device_coder=True) at several group sizes.

Stages one GOP of a synthetic configuration as bench/headline.py does (default: loot10, 32 frames, untrained model of seed 8807:
the stream sizes differ from a trained model's, the symbol counts and copies do not), checks that both paths give the same
streams, then times encode_gop 5 times each after one warm-up, alternating the paths so that drift hits all alike.  Also
reports the host-only coder time of frame 0 (the batch entries on buffers already in host memory), the bytes copied to the
host per frame, and the device coder's time per group from HIP events around linr_rc_encode_codes (table upload, rc_encode_k,
scan, rc_pack_k), with the symbols of the group's longest stream: the per-symbol rate of one wave.  Measurement aid
(profiles/device_codes_ab.txt, profiles/device_coder_ab.txt).

    python tools/codec_leg_ab.py [--config loot10] [--gop 32] [--runs 5] [--coder-groups 1 8 32]
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
from linr_pcgc_amd.model_core import DeviceCoderSet, codes_word_off, encode_streams, encode_streams_codes  # noqa: E402


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
    ap.add_argument('--coder-groups', type=int, nargs='*', default=[1, 8, 32], help='group sizes of the device-coder arms')
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

    arms = [('default', {}), ('device codes', {'device_codes': True})]
    arms += [('device coder, group %d' % g, {'device_coder': True, 'coder_group': g}) for g in args.coder_groups]

    def encode(kw):
        torch.cuda.synchronize()
        t0 = time.time()
        enc = codec.encode_gop(model, shell, gop, 8, n_threads=n_threads, **kw)
        torch.cuda.synchronize()
        return time.time() - t0, enc

    encs = [encode(kw)[1] for _, kw in arms]                 # warm-up of every path, and the identity check
    same = all(e['frames'] == encs[0]['frames'] for e in encs[1:])
    print('streams identical: %s (%d bytes)' % (same, sum(len(b) for fb in encs[0]['frames'] for b in fb)))
    del encs
    times = {name: [] for name, _ in arms}
    for _ in range(args.runs):
        for name, kw in arms:
            times[name].append(encode(kw)[0])
    width = max(len(name) for name, _ in arms)
    for name, _ in arms:
        t = times[name]
        print('encode_gop %-*s: median %.2f ms/frame, min %.2f, max %.2f; runs (s/GOP): %s'
              % (width, name, 1e3 * statistics.median(t) / len(gop), 1e3 * min(t) / len(gop), 1e3 * max(t) / len(gop),
                 ' '.join('%.4f' % v for v in t)))
    med = {name: statistics.median(t) for name, t in times.items()}
    spr = {name: max(t) - min(t) for name, t in times.items()}
    m0, m1 = med['default'], med['device codes']
    spread = max(spr['default'], spr['device codes'])
    print('difference of the medians: %.2f ms/frame (default - device codes); largest run-to-run spread %.2f ms/frame -> %s'
          % (1e3 * (m0 - m1) / len(gop), 1e3 * spread / len(gop),
             'device codes faster beyond the spread' if m0 - m1 > spread else 'NOT faster beyond the spread'))
    best = min(('default', 'device codes'), key=lambda k: med[k])
    for name, kw in arms[2:]:
        gain, both = med[best] - med[name], spr[best] + spr[name]
        print('%s against the better host arm (%s): %.2f ms/frame less, the two spreads together %.2f ms/frame -> %s'
              % (name, best, 1e3 * gain / len(gop), 1e3 * both / len(gop),
                 'faster beyond the spreads' if gain > both else 'NOT faster beyond the spreads'))

    # the device coder alone: HIP events around linr_rc_encode_codes for one group whose code values are already on the device
    coded_dev = Model_Estimate().compress_model(model, 8, True, shell)['new_model']
    for g in args.coder_groups:
        group = gop.frames[:g]
        parts, desc, cb, wb = [], [], 0, 0
        for f in group:
            woff = codes_word_off(f.row_off)
            rows, words = f.rows, int(woff[-1])
            parts.append((cb, rows, wb, words))
            for i in range(f.n_scales):
                a, n = int(f.row_off[i]), int(f.row_off[i + 1] - f.row_off[i])
                desc += [(cb + k * rows + a, wb + k * words + int(woff[i]), n) for k in range(8)]
            cb, wb = cb + 8 * rows, wb + 8 * words
        desc = np.asarray(desc, dtype=np.int64)
        c1 = torch.empty(cb, dtype=torch.uint16, device='cuda')
        sym = torch.empty(wb, dtype=torch.uint32, device='cuda')
        for f, (a, rows, b, words) in zip(group, parts):
            coded_dev.frame_codes(f, out=(c1[a:a + 8 * rows].view(8, rows), sym[b:b + 8 * words].view(8, words)))
        coder = DeviceCoderSet(len(desc), DeviceCoderSet.table(desc)[1], 'cuda')
        longest = int(desc[:, 2].max())
        # once with the untrained model's code values (about one bit per symbol), once with code values that give every symbol
        # 0.136 bit (the symbol coded owns 0.91 of the interval): the rate of a trained model, a renormalisation every seventh symbol
        for what in ('untrained model', '0.136 bit per symbol'):
            ms = []
            for _ in range(args.runs + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                coder.launch(c1, sym, desc)
                e1.record()
                got = coder.collect()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            m = statistics.median(ms[1:])
            print('device coder alone, group %d, %s: %d streams, %d symbols, longest stream %d symbols, %d stream bytes; median %.3f ms '
                  'per group (%.3f ms/frame, %.1f ns per symbol of the longest stream); runs %s'
                  % (len(group), what, len(desc), int(desc[:, 2].sum()), longest, sum(len(x) for x in got), m, m / len(group),
                     1e6 * m / longest, ' '.join('%.3f' % v for v in ms[1:])))
            for f, (a, rows, b, words) in zip(group, parts):          # c1 = 5898 where the symbol is 1, 65536 - 5898 where it is 0
                c1[a:a + 8 * rows].view(torch.int16).view(8, rows).copy_(
                    torch.where(f.occ.t() != 0, 5898, -5898).to(torch.int16))
        del c1, sym, coder

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
