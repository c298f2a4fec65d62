"""Shared by the legs of bench.py: CLI, constants, logging, small timing helpers."""
import argparse
import ctypes   # noqa: F401
import json     # noqa: F401
import os
import sys      # noqa: F401
import time     # noqa: F401

import numpy as np   # noqa: F401
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EPOCHS = 10          # first_epoch / others_epoch of BASELINE config[1]
PROF_EVERY = int(os.environ.get('LINR_BENCH_PROF_EVERY',
    8))          # live kernel timing samples every 8th timed step (every step when --steps <= 32)
TABLE_STEPS = 32     # fully instrumented extra steps behind the overfit (per-kernel table)
HBM_PEAK_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=320)
    ap.add_argument('--warmup', type=int, default=32)
    ap.add_argument('--ramp-s', dest='ramp_s', type=float, default=1.0,
                    help='seconds of untimed steps before the warm-up steps (clock ramp of a fresh box); 0 disables')
    ap.add_argument('--config', default='loot10', help='synthetic sequence (linr_pcgc_amd.synthetic.CONFIGS)')
    ap.add_argument('--gop', type=int, default=32)
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--sequence', action='store_true', help='headline = the whole BASELINE config[2] sequence (strong scaling)')
    ap.add_argument('--no-sequence', action='store_true', help='skip the config[2] sequence leg after the headline')
    ap.add_argument('--seq-frames', type=int, default=300)
    ap.add_argument('--seq-epochs', type=int, default=EPOCHS)
    ap.add_argument('--seq-decode-frames', type=int, default=1, help='frames per GOP decoded and checked in the sequence leg')
    ap.add_argument('--cpu-sample-rows', type=int, default=0, help='0 = whole frame 0')
    ap.add_argument('--full', action='store_true',
                    help='also run every leg beside the headline: decode check, roofline / per-kernel table, bf16 legs, bits/point '
                         'over seeds, rough figure, hidden 16, CPU baseline + full-size parity, config[2] sequence (resident and '
                         'cold), staging split, config[4] per rank; without it a run times the headline only')
    ap.add_argument('--dump-outputs', dest='dump_outputs', metavar='DIR', default=None,
                    help='write what the last timed step computed (its frame\'s bits, the parameters and Adam moments after it) '
                         'as DIR/<name>.npy')
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    if args.dump_outputs and args.sequence:
        ap.error('--dump-outputs describes the overfit headline; it is not available with --sequence')
    return args


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """arrays: name -> tensor / array; written as out_dir/<name>.npy in float32 (float64 stays float64)."""
    os.makedirs(out_dir, exist_ok=True)
    host = {}
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        host[name] = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
    total = sum(a.nbytes for a in host.values())
    assert total <= DUMP_LIMIT_BYTES, 'outputs of %d bytes exceed the %d-byte limit' % (total, DUMP_LIMIT_BYTES)
    for name, a in host.items():
        np.save(os.path.join(out_dir, name + '.npy'), a)
    log('outputs of the last timed step written to %s: %s' % (out_dir, ', '.join('%s %s %s' % (n, a.dtype, a.shape)
                                                                                  for n, a in host.items())))


def _time_launches(go, iters):
    for _ in range(5):
        go()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        go()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / iters


def _popcount32(t):
    """Set bits per element of an int32 tensor (the 27-bit masks of the compressed kernel map)."""
    v = t.to(torch.int64) & 0xFFFFFFFF
    v = v - ((v >> 1) & 0x55555555)
    v = (v & 0x33333333) + ((v >> 2) & 0x33333333)
    v = (v + (v >> 4)) & 0x0F0F0F0F
    return (v * 0x01010101 >> 24) & 0xFF


def steps_done_so_far(steps, rest, total):
    """True when the run covered exactly one complete overfit (the best-epoch bookkeeping is per overfit)."""
    return steps + rest == total


def log(msg):
    if int(os.environ.get('RANK', 0)) == 0:
        print('[bench %7.1fs] %s' % (time.time() - T_START, msg), file=sys.stderr, flush=True)


T_START = time.time()


def host_threads():
    """CPU threads this process may really use (the GPU box gives one GPU a 16-core share)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, 16))
