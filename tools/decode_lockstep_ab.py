"""A/B of the lock-step GOP decoder (codec.decode_gop lockstep=B) against the per-frame decoder, one process, one GPU: the loot10
GOP of 32 frames that bench.py codes (model trained argv[2] epochs, default 10, so that the streams have the entropy of real ones),
decoded as decode_gop(), decode_gop(workers=8) - the comparator, whose code path the lock-step decoder does not touch - and
decode_gop(lockstep=B) for B = 4, 8, 16, 32.  One warm-up per variant, then 5 timed runs behind a device synchronisation; median and
min-max in ms per frame; every variant checked lossless; the largest lock-step workspace.  Then one group of 8 frames scale by
scale: the lock-step call with 16 and with 1 host thread beside the sum of the 8 per-frame calls, which tells the host range
decoding (what the threads divide) from the launches and round trips (what the group divides)."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from linr_pcgc_amd import codec, overfit, synthetic                     # noqa: E402
from linr_pcgc_amd.model_codec import Model_Estimate                    # noqa: E402
from linr_pcgc_amd.model_core import FlatAdam                           # noqa: E402
from linr_pcgc_amd.module_utils import unique_sorted                    # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 10
RUNS = 5
torch.set_num_threads(4)
clouds = [synthetic.sequence_frame_device('loot10', t, 'cuda') for t in range(n)]
gop = overfit.Gop(None, clouds, None, 64, 'cuda')
model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807)
if epochs:
    print('trained %d epochs: %.3f bpp' % (epochs, min(overfit.overfit_gop(model, FlatAdam(model), gop, epochs))))
enc = codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda'), gop, 8)
truth = [torch.as_tensor(gop.infos[i]['ori']).cuda() + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32) for i in range(n)]
print('%d frames, %d points, %d host threads available' % (n, sum(gop.point_nums), len(os.sched_getaffinity(0))))

variants = [('decode_gop()', {}), ('decode_gop(workers=8)', {'workers': 8})]
variants += [('decode_gop(lockstep=%d)' % b, {'lockstep': b}) for b in (4, 8, 16, 32) if b <= n]
peak = [0]


def run(kw):
    shell = overfit.gen_model(gop.scale_num, 'cuda')
    timing = {}
    torch.cuda.synchronize()
    t0 = time.time()
    dec = codec.decode_gop(shell, enc, 'cuda', timing=timing, **kw)
    torch.cuda.synchronize()
    peak[0] = max(peak[0], timing.get('lockstep_ws_bytes', 0))
    return dec, (time.time() - t0) * 1e3 / n


rows = {}
for name, kw in variants:
    dec, _ = run(kw)                                                     # warm-up, and the lossless check
    ok = all(torch.equal(a, b) for a, b in zip(dec, truth))
    rows[name] = (sorted(run(kw)[1] for _ in range(RUNS)), ok)
print('%-26s %8s %8s %8s  %s' % ('variant (ms per frame)', 'median', 'min', 'max', 'lossless'))
for name, (t, ok) in rows.items():
    print('%-26s %8.3f %8.3f %8.3f  %s' % (name, statistics.median(t), t[0], t[-1], ok))
cmp_t = rows['decode_gop(workers=8)'][0]
cmp_med = statistics.median(cmp_t)
for name, (t, ok) in rows.items():
    if 'lockstep' in name:
        med = statistics.median(t)
        apart = (med < cmp_t[0] or med > cmp_t[-1]) and (cmp_med < t[0] or cmp_med > t[-1])
        print('%s vs workers=8: %.2fx, %s' % (name, cmp_med / med, ('faster' if med < cmp_med else 'slower') if apart else
                                              'not separated (a median lies inside the other min-max)'))

# ---- one group of 8 frames, scale by scale -------------------------------------------------------------------------------------
side = dict(enc['side_info'])
side.pop('arith_version', None)
side['final_bytes'] = enc['model_bin']
m, _ = Model_Estimate().decompress_model(overfit.gen_model(gop.scale_num, 'cuda'), side)
m.inference_precision = side.get('precision', 'f32')
lows, _ = codec.dec_all_frame_low_xyz(enc['low_enc_bytes'])
G = min(8, n)


def timed(fn):
    best, out = 1e9, None
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.time()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, (time.time() - t0) * 1e3)
    return best, out


lv = [unique_sorted(torch.tensor(lows[i].astype('int32'), device='cuda')) for i in range(G)]
bits = max(1, int(max(int(x.max()) for x in lv)).bit_length())
print('one group of %d frames, ms per scale (best of 3): rows | lock-step 16 threads | lock-step 1 thread | sum of %d per-frame calls' % (G, G))
for s_idx in range(gop.scale_num - 1, -1, -1):
    bits = min(bits + 1, 21)
    encs = [enc['frames'][i][s_idx] for i in range(G)]
    t16, nxt = timed(lambda: m.decode_scale_batch(lv, s_idx, encs, 16))
    t1, _ = timed(lambda: m.decode_scale_batch(lv, s_idx, encs, 1))
    tp, per = timed(lambda: [m.decode_scale(lv[i], s_idx, encs[i], bits) for i in range(G)])
    assert all(torch.equal(a, b) for a, b in zip(nxt, per))
    print('scale %d: %9d rows  %8.3f  %8.3f  %8.3f' % (s_idx, sum(int(x.shape[0]) for x in lv), t16, t1, tp))
    lv = nxt
print('largest lock-step workspace (lockstep=%d): %.1f MiB' % (min(32, n), peak[0] / 2 ** 20))
