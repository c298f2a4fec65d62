"""Guards of tests/bf16_train_deep_ref.py (the any-depth autograd emulation of the bf16 training executor), on the CPU:
  * at block_layers 1 it IS oracle/network_bf16.py's train_frame_bits: bits and every gradient bit for bit;
  * with every rounding off at block_layers 2, 3, 4 it is oracle/network.py's fp32 network - bits and every gradient within 1e-6
    relative (of the tensor's own largest entry): the wiring, the ResNetBlock's extra skip (models/resnet.py:156-162) above all.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bf16_train_deep_ref as dref           # noqa: E402
from oracle import network as onet           # noqa: E402
from oracle import network_bf16 as obf       # noqa: E402
from oracle import octree as ooct            # noqa: E402


def _sd(scale_num, block_layers, seed=8807):
    from linr_pcgc_amd.model_core import LINR_PCGC_Model
    torch.manual_seed(seed)
    m = LINR_PCGC_Model({'scale_num': scale_num, 'in_channel': 7, 'hidden_channel_conv': 8, 'block_layers': block_layers,
                         'outstage': 8, 'instage': 1})
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(seed + block_layers)
    for k, v in sd.items():             # away from the initialisation: biases of all signs
        sd[k] = v + 0.05 * torch.randn(v.shape, generator=g)
    return sd


def _scales(golden_dir, which, dtype=torch.float32):
    g = np.load(os.path.join(golden_dir, 'octree_shell128.npz'))
    out = []
    for s in which:
        c = g['s%d_coord' % s]
        out.append({'coord': c, 'occ': g['s%d_occ' % s], 'offset_tensor': g['s%d_offset' % s], 'scale_idx': s, 'nbr': ooct.neighbour_table(c)})
    return onet.to_torch_scales(out, dtype)


def _grads(fn, sd, scales):
    leaves = {k: v.clone().requires_grad_() for k, v in sd.items()}
    bits = fn(leaves, scales)
    bits.backward()
    return bits.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}


def test_depth_one_is_the_committed_emulation(golden_dir):
    sd = _sd(5, 1)
    scales = _scales(golden_dir, (2, 3, 4))
    ref_bits, ref = _grads(obf.train_frame_bits, sd, scales)
    bits, got = _grads(dref.train_frame_bits, sd, scales)
    assert torch.equal(bits, ref_bits)
    for k in ref:
        assert torch.equal(got[k], ref[k]), k


@pytest.mark.parametrize('block_layers', [2, 3, 4])
def test_without_roundings_it_is_the_fp32_network(golden_dir, block_layers):
    """In float64, so that 1e-6 is a statement about the wiring and not about two fp32 summation orders."""
    sd = {k: v.double() for k, v in _sd(5, block_layers).items()}
    scales = _scales(golden_dir, (2, 3, 4), torch.float64)
    ref_bits, ref = _grads(onet.frame_bits, sd, scales)
    with dref.rounding(False):
        bits, got = _grads(dref.train_frame_bits, sd, scales)
    assert obf.st is not dref._ident and obf.wq is not dref._ident, 'the switch must put the roundings back'
    assert abs(float(bits) - float(ref_bits)) <= 1e-6 * float(ref_bits)
    for k in ref:
        gmax = float(ref[k].abs().max())
        assert float((got[k] - ref[k]).abs().max()) <= 1e-6 * gmax, k
    # and the roundings are on again: the emulation differs from the fp32 network
    on_bits, _ = _grads(dref.train_frame_bits, {k: v.float() for k, v in sd.items()}, _scales(golden_dir, (4,)))
    off_bits, _ = _grads(onet.frame_bits, {k: v.float() for k, v in sd.items()}, _scales(golden_dir, (4,)))
    assert float(on_bits) != float(off_bits)


def test_the_extra_skip_is_one_stored_matrix(golden_dir):
    """S = st(I_last + A): with roundings on, block_layers 2 differs from the same network without the skip's own rounding only through
    that rounding - i.e. the emulation at depth 2 is NOT inception_t(inception_t(a)) + a unrounded."""
    sd = _sd(5, 2)
    sc = _scales(golden_dir, (4,))[0]
    p = 'upsampler.block_in'
    with torch.no_grad():
        x = obf.st(onet.scale_context(sd, sc['offset_tensor'], sc['scale_idx']))
        a = obf.st(torch.relu(obf.conv3t(x, sc['nbr'], sd[p + '.0.kernel'], sd[p + '.0.bias'])))
        i1 = obf.inception_t(obf.inception_t(a, sc['nbr'], sd, p + '.2.layers.0'), sc['nbr'], sd, p + '.2.layers.1')
        want = obf.st(obf.conv3t(obf.rb(i1 + a), sc['nbr'], sd[p + '.3.kernel'], sd[p + '.3.bias']))
        got = dref.make_block_t(x, sc['nbr'], sd, p)
    assert torch.equal(got, want)
