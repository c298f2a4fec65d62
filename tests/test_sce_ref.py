"""CPU checks of tests/sce_ref.py, the float64 reference of the scale context that tests/test_gpu_multi_tile.py holds the kernels to,
against oracle.network.scale_context (models/model_core.py:48-53) and float64 autograd: values, every gradient in the flat layout of
linr_sce_bwd_params, exact zeros for absent and zero-row scales, the `_abs` companions and the smallest ReLU input."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sce_ref as sr                        # noqa: E402
from oracle import network as onet          # noqa: E402

# the multi-scale frame of the GPU test with fewer rows: scales 3 and 5 absent, scale 0 named but empty, not in order
FRAMES = {'single': (1, [(0, 37)]), 'three': (5, [(2, 300), (0, 77), (4, 19)]), 'absent_and_empty': (6, [(4, 1031), (0, 0), (2, 1), (1, 257)])}


def _autograd(flat64, S, row_off, scale_idx, off, gx0):
    """x0, hid, ghid and the flat gradient of sum gx0 . x0 from the oracle's scale_context and autograd, float64"""
    leaf = flat64.clone().requires_grad_()
    sd = sr.state_dict_of(leaf, S)
    x0s, hids, ghids, loss = [], [], [], 0.0
    for j, si in enumerate(int(s) for s in scale_idx):
        a, b = int(row_off[j]), int(row_off[j + 1])
        x0 = onet.scale_context(sd, off[a:b], si)
        x0s.append(x0.detach())
        loss = loss + (x0 * gx0[a:b]).sum()
        # the hidden layer and its gradient through a graph of their own: hpre as a leaf
        mix = torch.cat([sd['scale_emb.weight'][si].detach().expand(b - a, -1), off[a:b]], 1)
        hpre = F.linear(mix, sd['scale_mlp.%d.0.weight' % si].detach(), sd['scale_mlp.%d.0.bias' % si].detach()).requires_grad_()
        h = F.relu(hpre)
        y = F.linear(h, sd['scale_mlp.%d.2.weight' % si].detach(), sd['scale_mlp.%d.2.bias' % si].detach())
        hids.append(h.detach())
        ghids.append(torch.autograd.grad((y * gx0[a:b]).sum(), hpre)[0] if b > a else torch.zeros(0, 16, dtype=torch.float64))
    loss.backward()
    return torch.cat(x0s), torch.cat(hids), torch.cat(ghids), leaf.grad


@pytest.mark.parametrize('name', sorted(FRAMES))
def test_reference_equals_the_oracle_and_float64_autograd(name):
    S, ranges = FRAMES[name]
    flat = sr.draw_params(S, 11)
    row_off, scale_idx, off, gx0 = sr.draw_frame(ranges, 12)
    assert set(np.unique(off.numpy())) <= {0.0, 1.0}
    got = sr.reference(flat, S, row_off, scale_idx, off, gx0)
    x0, hid, ghid, grads = _autograd(flat.double(), S, row_off, scale_idx, off.double(), gx0.double())
    for key, want in (('x0', x0), ('hid', hid), ('ghid', ghid), ('grads', grads)):
        assert got[key].dtype == torch.float64 and got[key].shape == want.shape
        assert float((got[key] - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max())), key
    assert sr.names(S)[0] == 'scale_emb.weight' and len(sr.names(S)) == 1 + 4 * S and grads.numel() == sr.param_count(S)
    # the flat layout is the state dict's order (what linr_sce_bwd_params writes): spot-check one tensor by name
    sd_g = sr.state_dict_of(got['grads'], S)
    si = int(scale_idx[0])
    a, b = int(row_off[0]), int(row_off[1])
    assert float((sd_g['scale_mlp.%d.2.bias' % si] - gx0[a:b].double().sum(0)).abs().max()) <= 1e-12
    # scales without rows: exact zeros, embedding rows included
    used = {int(s) for j, s in enumerate(scale_idx) if row_off[j + 1] > row_off[j]}
    for s in range(S):
        if s not in used:
            for key in ('grads', 'grads_abs'):
                p = sr.unpack(got[key], S)
                assert bool((p['emb'][s] == 0).all()) and all(bool((t == 0).all()) for t in p[s])
    if name == 'absent_and_empty':
        assert used == {1, 2, 4}
    # the smallest ReLU input, against the oracle's pieces
    sd = sr.state_dict_of(flat.double(), S)
    want = min(float(F.linear(torch.cat([sd['scale_emb.weight'][int(s)].expand(int(row_off[j + 1] - row_off[j]), -1),
                                         off[int(row_off[j]):int(row_off[j + 1])].double()], 1),
                              sd['scale_mlp.%d.0.weight' % int(s)], sd['scale_mlp.%d.0.bias' % int(s)]).abs().min())
               for j, s in enumerate(scale_idx) if row_off[j + 1] > row_off[j])
    assert got['min_pre'] == want and want > 0


def test_abs_companions_bound_their_values_and_equal_them_on_nonnegative_inputs():
    S, ranges = FRAMES['absent_and_empty']
    flat = sr.draw_params(S, 5)
    row_off, scale_idx, off, gx0 = sr.draw_frame(ranges, 6)
    got = sr.reference(flat, S, row_off, scale_idx, off, gx0)
    for key in ('x0', 'hid', 'ghid', 'grads'):
        assert bool((got[key + '_abs'] >= got[key].abs() * (1 - 1e-14)).all()), key
    # non-negative parameters and gradients: every ReLU is open, every term positive - the companion IS the value
    pos = sr.reference(flat.abs(), S, row_off, scale_idx, off, gx0.abs())
    for key in ('x0', 'hid', 'ghid', 'grads'):
        assert float((pos[key + '_abs'] - pos[key]).abs().max()) <= 1e-13 * float(pos[key].abs().max()), key
    # ... and it is what the signed inputs' companion is, where the mask does not enter
    for key in ('x0', 'hid'):
        assert torch.equal(pos[key + '_abs'], got[key + '_abs'])


def test_two_ranges_of_one_scale_are_summed_and_no_gradient_without_gx0():
    flat = sr.draw_params(3, 1)
    row_off, scale_idx, off, gx0 = sr.draw_frame([(1, 40), (1, 24)], 2)
    two = sr.reference(flat, 3, row_off, scale_idx, off, gx0)
    one = sr.reference(flat, 3, np.asarray([0, 64]), np.asarray([1], dtype=np.int32), off, gx0)
    assert float((two['grads'] - one['grads']).abs().max()) <= 1e-13 and torch.equal(two['x0'], one['x0'])
    assert 'grads' not in sr.reference(flat, 3, row_off, scale_idx, off)
