"""Host-side arithmetic coder speed (ns / binary symbol) on this machine: linr_ac_encode_binary (probabilities + symbol bytes),
linr_ac_encode_binary_codes (code values + symbol bit planes) and linr_ac_decode_binary on the same symbols, one thread.  Two
streams: probabilities from beta(0.3, 0.3), and a trained model's rate (the symbol coded owns 0.91 of the interval, 0.136 bit per
symbol: most symbols shift nothing out).

    python tools/ac_speed.py [--reps 3]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (loads libamdhip64 before the library)
from linr_pcgc_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
args = ap.parse_args()
L = _lib.lib()
rng = np.random.default_rng(0)
n = 2_000_000
p_beta = np.clip(rng.beta(0.3, 0.3, size=n), 1e-4, 1 - 1e-4).astype(np.float32)
s_beta = (rng.random(n) < p_beta).astype(np.uint8)
s_rate = rng.integers(0, 2, n).astype(np.uint8)
p_rate = np.where(s_rate != 0, 0.91, 0.09).astype(np.float32)
out = np.empty(2 * n + 64, np.uint8)
out_c = np.empty(2 * n + 64, np.uint8)
dec = np.empty(n, np.uint8)
for name, p, s in (('beta(0.3, 0.3)', p_beta, s_beta), ('trained rate', p_rate, s_rate)):
    # the library's code value, in float32 like the library: (rint((1 - p) * 65534) + 1) & 0xFFFF
    c1 = ((np.rint((np.float32(1) - p) * np.float32(65534)).astype(np.int64) + 1) & 0xFFFF).astype(np.uint16)
    w = np.packbits(np.concatenate([s, np.zeros(-n % 32, np.uint8)]), bitorder='little').view('<u4').astype(np.uint32)
    for rep in range(args.reps):
        t = time.perf_counter(); ln = L.linr_ac_encode_binary(p.ctypes.data, s.ctypes.data, n, out.ctypes.data, out.size); te = time.perf_counter() - t
        t = time.perf_counter(); lc = L.linr_ac_encode_binary_codes(c1.ctypes.data, w.ctypes.data, n, out_c.ctypes.data, out_c.size); tc = time.perf_counter() - t
        t = time.perf_counter(); L.linr_ac_decode_binary(p.ctypes.data, n, out.ctypes.data, ln, dec.ctypes.data); td = time.perf_counter() - t
        print('%-14s bits/sym %.3f  enc %.2f ns/sym  enc codes %.2f ns/sym  dec %.2f ns/sym  ok=%s'
              % (name, ln * 8 / n, te / n * 1e9, tc / n * 1e9, td / n * 1e9,
                 bool((dec == s).all()) and lc == ln and bool((out[:ln] == out_c[:ln]).all())))
print('cpus', len(os.sched_getaffinity(0)))
