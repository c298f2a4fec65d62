"""Child process of tests/test_gpu_params_avg.py: the averaging kernel's chained updates on every size, row count and stride of the
list, dumped as one .npz (the parent runs it under LINR_DEBUG_POISON=1 and compares with the host twin)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out):
    import torch  # noqa: F401
    from test_gpu_params_avg import CASES, chain_device
    dump = {}
    for n, K, pad in CASES:
        dump['n%d_K%d_p%d' % (n, K, pad)] = chain_device(n, K, ((n + 3) & ~3) + pad)[-1]
    np.savez(out, **dump)


if __name__ == '__main__':
    main(sys.argv[1])
