"""Reference (not a test): the autograd emulation of the bf16 training executor for ANY block_layers of block_in.

oracle/network_bf16.py's train_forward_scale stops at block_layers 1 (its make_block_t raises on a second Inception layer).  This module
is the same emulation built from that module's own pieces - st (a stored matrix: bf16 going forward AND backward), wq (bf16 kernel value,
gradient to the fp32 master), conv3t, inception_t - with make_block_t chaining nl layers and applying the ResNetBlock's extra skip
(models/resnet.py:156-162: out = layers(x) + x when there is more than one layer) as ONE stored matrix st(out + a), the rounding of
csrc/net_bf16.hip: badd_rows_k.  The roundings the executor (csrc/train_bf16.hip) then has, by autograd:
  forward   layer l >= 1 reads the stored I_{l-1}; S = bf16(I_{nl-1} + A); the tail convolution reads S
  backward  gS = bf16(bwd(tail)); gI_{nl-1} = gS; gI_{l-1} = bf16(bwd(gH_l[:, 0:4]; W00_l) + gI_l + gH_l[:, 4:8] @ W10_l^T) (no ReLU
            mask: a layer's input is not a ReLU output); gA = bf16((.. of layer 0 .. + gS) * (A > 0))

`rounding(False)` turns every rounding off (st and wq become the identity): the wiring alone, which must then equal oracle/network.py's
fp32 network - tests/test_bf16_train_deep_ref.py pins both ends.
"""
import contextlib

import torch.nn.functional as F

from oracle import network as onet
from oracle import network_bf16 as obf

_ident = lambda x: x


@contextlib.contextmanager
def rounding(on):
    """Inside: every rounding of the emulation on (the default) or off.  oracle/network_bf16.py's st / wq are looked up through the
    module at call time (conv3t and inception_t call them as globals), so they are swapped there and put back."""
    keep = (obf.st, obf.wq)
    if not on:
        obf.st, obf.wq = _ident, _ident
    try:
        yield
    finally:
        obf.st, obf.wq = keep


def make_block_t(x, nbr, sd, p, res=None):
    a = obf.st(F.relu(obf.conv3t(x, nbr, sd[p + '.0.kernel'], sd[p + '.0.bias'])))
    out, nl = a, 0
    while (p + '.2.layers.%d.conv0_0.kernel' % nl) in sd:
        out = obf.inception_t(out, nbr, sd, p + '.2.layers.%d' % nl)
        nl += 1
    if nl > 1:
        out = obf.st(out + a)
    o = obf.conv3t(out, nbr, sd[p + '.3.kernel'], sd[p + '.3.bias'])
    return obf.st(o if res is None else o + res)


def train_forward_scale(sd, scale):
    """oracle/network_bf16.py: train_forward_scale with the make_block_t above; sd = the fp32 MASTER state dict."""
    u = 'upsampler.'
    nbr, occ = scale['nbr'], scale['occ']
    x_low = obf.st(onet.scale_context(sd, scale['offset_tensor'], scale['scale_idx']))
    x_glob = make_block_t(x_low, nbr, sd, u + 'block_in')
    logits, probs = [], []
    prior = x_glob
    for k in range(8):
        c = obf.st(obf.conv3t(prior, nbr, sd[u + 'prune_blocks.%d.0.conv.kernel' % k], sd[u + 'prune_blocks.%d.0.conv.bias' % k]))
        z = onet.mlp(c, sd, u + 'inner_mlps.%d.0' % k)
        logits.append(z)
        probs.append(z.sigmoid())
        if k == 7:
            break
        prior = make_block_t(occ[:, :k + 1], nbr, sd, u + 'outter_blocks.%d' % k, res=x_glob)
    return {'logits': logits, 'probs': probs, 'bits': onet.bits_of(probs, occ)}


def train_frame_bits(sd, scales):
    total = 0
    for s in scales:
        total = total + train_forward_scale(sd, s)['bits']
    return total
