"""The width-generic bf16 emulation (tests/wide_bf16_ref.py) at width 8 against the committed oracle of the width-8 executor
(oracle.network_bf16.forward_scale): bit for bit, at block_layers 1 and 2."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wide_bf16_ref as wref                 # noqa: E402
from oracle import network as onet           # noqa: E402
from oracle import network_bf16 as obf       # noqa: E402
from oracle import octree as ooct            # noqa: E402


def _sd(scale_num, block_layers, hidden=8, seed=8807):
    from linr_pcgc_amd.model_core import LINR_PCGC_Model
    torch.manual_seed(seed)
    m = LINR_PCGC_Model({'scale_num': scale_num, 'in_channel': 7, 'hidden_channel_conv': hidden, 'block_layers': block_layers,
                         'outstage': 8, 'instage': 1})
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(seed + block_layers)
    for k, v in sd.items():             # away from the initialisation: biases of all signs, larger kernels
        sd[k] = v + 0.05 * torch.randn(v.shape, generator=g)
    return sd


def _scale(golden_dir, s):
    g = np.load(os.path.join(golden_dir, 'octree_shell128.npz'))
    c = g['s%d_coord' % s]
    sc = {'coord': c, 'occ': g['s%d_occ' % s], 'offset_tensor': g['s%d_offset' % s], 'scale_idx': s, 'nbr': ooct.neighbour_table(c)}
    return onet.to_torch_scales([sc])[0]


@pytest.mark.parametrize('block_layers', [1, 2])
def test_generic_emulation_equals_the_width8_oracle(golden_dir, block_layers):
    sd = _sd(5, block_layers)
    for s in (2, 4):
        sc = _scale(golden_dir, s)
        with torch.no_grad():
            ref = obf.forward_scale(sd, sc)
            got = wref.forward_scale(sd, sc)
        for k in range(8):
            assert torch.equal(got['logits'][k], ref['logits'][k]), (s, k)
            assert torch.equal(got['probs'][k], ref['probs'][k]), (s, k)
        assert torch.equal(got['bits'], ref['bits'])


def test_generic_emulation_runs_wide_models(golden_dir):
    """At width 16 the emulation is a finite, proper probability model (the GPU tests compare the HIP executor against it)."""
    sd = _sd(5, 1, hidden=16)
    sc = _scale(golden_dir, 3)
    with torch.no_grad():
        out = wref.forward_scale(sd, sc)
    assert all(bool(torch.isfinite(z).all()) for z in out['logits'])
    assert all(bool(((p >= 0) & (p <= 1)).all()) for p in out['probs'])
    assert float(out['bits']) > 0
