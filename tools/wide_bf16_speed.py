"""Wide models (hidden_channel_conv 16 / 32) on frame 0 of a config: one codec forward (frame_probs) and the stage-serial decode of
the frame (all scales, 8 stage forwards + range decoding), fp32 wide executor vs the bf16 / uint8-weight one; median of repeated runs.
--prof: only the bf16 forward at the given width, a few times (for a kernel-trace run)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from linr_pcgc_amd import overfit, synthetic                 # noqa: E402
from linr_pcgc_amd.model_codec import Model_Estimate          # noqa: E402
from linr_pcgc_amd.model_core import encode_streams           # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='loot10')
    ap.add_argument('--widths', default='16,32')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--prof', action='store_true')
    a = ap.parse_args()
    gop = overfit.Gop(None, [synthetic.sequence_frame_device(a.config, 0, 'cuda')], None, 64, 'cuda')
    frame = gop.frames[0]
    for hidden in [int(w) for w in a.widths.split(',')]:
        m = overfit.gen_model(gop.scale_num, 'cuda', seed=8807, hidden=hidden)
        coded = Model_Estimate().compress_model(m, 8, True, overfit.gen_model(gop.scale_num, 'cuda', hidden=hidden))['new_model']
        if a.prof:
            for _ in range(3):
                coded.frame_probs(frame, precision='bf16')
            torch.cuda.synchronize()
            continue
        row = {}
        for prec in ('f32', 'bf16'):
            coded.frame_probs(frame, precision=prec)
            row['fwd_' + prec] = timed(lambda: coded.frame_probs(frame, precision=prec), a.reps)
            probs, _ = coded.frame_probs(frame, precision=prec)
            p_host = probs.cpu().numpy()
            occ = frame.occ.t().contiguous().cpu().numpy().astype('uint8')
            streams = []
            for i in range(frame.n_scales):
                r0, r1 = int(frame.row_off[i]), int(frame.row_off[i + 1])
                streams.append(encode_streams([p_host[k][r0:r1] for k in range(8)], [occ[k][r0:r1] for k in range(8)]))
            keep = frame.occ.clone()

            def dec():
                coded.decode_frame(frame, streams, precision=prec)
            row['dec_' + prec] = timed(dec, max(3, a.reps // 3))
            assert torch.equal(frame.occ, keep), 'decode is not lossless'
        print('%s frame 0 (%d rows) hidden %2d: forward fp32 %.2f ms, bf16 %.2f ms (%.2fx); decode fp32 %.1f ms, bf16 %.1f ms (%.2fx)'
              % (a.config, frame.rows, hidden, row['fwd_f32'], row['fwd_bf16'], row['fwd_bf16'] / row['fwd_f32'], row['dec_f32'],
                 row['dec_bf16'], row['dec_bf16'] / row['dec_f32']), flush=True)


if __name__ == '__main__':
    main()
