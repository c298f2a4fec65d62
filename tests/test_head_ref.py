"""CPU checks of tests/head_ref.py, the float64 reference of the heads on saturated logits, against torch's own fp32
binary_cross_entropy + autograd (what the reference runs: models/upsample.py:160, models/model_core.py:72-81):
  |z| <= 8           the project's tolerances (tests/gpu_common.py): bits rel 1e-5, gradients 1e-4 of the largest
  saturated classes  the exact values: 100 nats, gz == 0 for p in {0, 1}
  the inputs of tests/test_gpu_heads_saturated.py: the fp32 oracle within 1e-5 relative of the float64 bits, every class drawn."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_ref as hr          # noqa: E402


def _torch_fp32(z32, t, gscale):
    """nats per row and d (gscale * sum nats) / dz as torch computes them in fp32"""
    z = z32.clone().requires_grad_()
    per = F.binary_cross_entropy(torch.sigmoid(z), t, reduction='none')
    (per.sum() * gscale).backward()
    return per.detach(), z.grad


def test_ordinary_rows_match_torch_fp32():
    gen = torch.Generator().manual_seed(3)
    z = (torch.rand(4096, generator=gen) * 16 - 8).double()
    t = (torch.rand(4096, generator=gen) < 0.5).float()
    p32 = hr.sigmoid32(z)
    per, gz = _torch_fp32(z.float(), t, 0.37)
    assert float((p32 - torch.sigmoid(z.float())).abs().max()) <= 1.2e-7            # one ulp below 1
    ref = hr.nats(p32, t)
    assert abs(float(ref.sum()) - float(per.double().sum())) <= 1e-5 * float(ref.sum())
    g = hr.gz_of(p32, t, 0.37)
    assert float((g - gz.double()).abs().max()) <= 1e-4 * float(g.abs().max())
    assert float((g - 0.37 * (p32.double() - t.double())).abs().max()) <= 1e-15      # unclamped: quotient and product cancel
    # ... and the helper's own formulas run in float32 (the "fp32 oracle" of the backward tests) agree with autograd as closely
    g32 = hr.gz_of(p32, t, 0.37, torch.float32)
    assert g32.dtype == torch.float32 and float((g32.double() - gz.double()).abs().max()) <= 1e-6 * float(g.abs().max())


def test_saturated_rows_have_the_exact_values():
    z = torch.tensor([20.0, 25.0, 60.0, 200.0, -20.0, -27.0, -28.0, -80.0, -95.0, -104.0, -110.0, -200.0], dtype=torch.float64)
    p32 = hr.sigmoid32(z)
    assert bool((p32[:4] == 1.0).all()) and bool((p32[-3:] == 0.0).all()) and 0.0 < float(p32[7]) < 1e-34
    for tv in (0.0, 1.0):
        t = torch.full((len(z),), tv)
        per, gz = _torch_fp32(z.float(), t, 1.0)
        ref, g = hr.nats(p32, t), hr.gz_of(p32, t, 1.0)
        # torch's fp32 BCELoss on the same rows: the same nats to fp32 resolution, the clamps exactly
        assert float((ref - per.double()).abs().max()) <= 1e-5 * 100
        sat = (p32 == 0) | (p32 == 1)
        assert bool((g[sat] == 0).all()) and bool((gz[sat] == 0).all())
        wrong = (p32 == 1.0) if tv == 0.0 else (p32 == 0.0)
        assert bool((ref[wrong] == 100.0).all()) and bool((per[wrong] == 100.0).all())
        assert bool((ref[sat & ~wrong] == 0.0).all())
        assert float((g - gz.double()).abs().max()) <= 1e-6                          # incl. both sides of the 1e-12 switch (z = -27, -28)
    # the switch itself: below it the gradient of a contradicted row DEcreases with |z|
    g = hr.gz_of(hr.sigmoid32(torch.tensor([-27.0, -28.0, -40.0])), torch.ones(3), 1.0)
    assert abs(float(g[0]) + 1.0) < 1e-9 and -1.0 < float(g[1]) < -0.5 and abs(float(g[2]) + 1e12 * np.exp(-40.0)) < 1e-10


def test_supplied_probabilities():
    v = hr.supplied_probabilities()
    assert len(v) == 11 and v.dtype == np.float32 and 0 < float(v[2]) < 2e-45 and float(v[9]) == 1.0 - 2.0 ** -24
    for n in hr.NS:
        p, t = hr.supplied_rows(n)
        g = hr.gz_of(p, t, 1.0)
        assert float(p[n - 1]) == float(np.float32(1e-6)) and float(t[n - 1]) == 1.0
        assert float(g.abs().max()) <= 1.0 and abs(float(g[n - 1])) >= 1.0 - 2e-6
        if n >= 63:
            assert all(bool(((p == float(x)) & (t == tv)).any()) for x in v for tv in (0.0, 1.0))


@pytest.mark.parametrize('C', [8, 16, 32])
def test_head_backward_equals_autograd_in_float64(C):
    """The explicit backward of the helper against autograd of the same head in float64 on ordinary logits (where gz = gscale (p - t))."""
    gen = torch.Generator().manual_seed(C)
    c = torch.randn(300, C, generator=gen, dtype=torch.float64)
    w1, b1 = torch.randn(24, C, generator=gen, dtype=torch.float64) * 0.3, torch.randn(24, generator=gen, dtype=torch.float64) * 0.1
    w2, b2 = torch.randn(24, generator=gen, dtype=torch.float64) * 0.3, torch.randn(1, generator=gen, dtype=torch.float64) * 0.1
    t = (torch.rand(300, generator=gen) < 0.5).double()
    leaves = [x.clone().requires_grad_() for x in (c, w1, b1, w2, b2)]
    z = hr.head_logits(*leaves)
    (F.binary_cross_entropy(torch.sigmoid(z), t, reduction='sum') * 0.37).backward()
    # the stored probability is fp32: the reference differs from float64 autograd by that rounding of p (6e-8) and by no more
    got = hr.head_backward(c, hr.sigmoid32(z.detach()), t, w1, b1, w2, 0.37)
    for name, leaf in zip(('gc', 'gw1', 'gb1', 'gw2', 'gb2'), leaves):
        assert float((got[name] - leaf.grad).abs().max()) <= 2e-7 * max(1.0, float(leaf.grad.abs().max())), name


@pytest.mark.parametrize('C', [8, 16, 32])
@pytest.mark.parametrize('n', hr.NS)
def test_forward_inputs_are_well_conditioned(n, C):
    """The inputs of the op-level forward tests: logits of standard deviation ~40, every class of choose_targets drawn, no row in the
    forbidden pieces, and the fp32 oracle within 1e-5 relative of the float64 reference's bits - the bound the kernels are then held to is
    the oracle's own distance, not theirs."""
    k = hr.saturated_case(n, C)
    z, t = k['z64'].numpy(), k['t'].numpy()
    assert bool((t[(z > 8) & (z < 20)] == 1).all()) and bool((t[z < -80] == 0).all())
    if n >= 257:
        assert 30.0 <= float(k['z64'].std()) <= 50.0
        assert all(k['counts'][c] >= 8 for c in hr.CLASSES), k['counts']
        assert float(hr.nats(k['p32'], k['t']).max()) == 100.0
    o32 = hr.oracle32_bits(k)
    if k['bits64'] == 0.0:
        # n = 1 at width 16: one agreeing saturated row (z = -25.5, t = 0), exactly 0 nats as the helper and the kernels form them
        # (log(1 - p) with 1 - p == 1.0f).  torch's CPU BCELoss takes log1p(-p) instead: p = 8e-12 nats, below half an ulp of 1 per row.
        assert n == 1 and 0.0 <= o32 <= 2.0 ** -25 / hr.LN2
    else:
        assert abs(o32 - k['bits64']) <= 1e-5 * k['bits64'], (o32, k['bits64'], k['counts'])
