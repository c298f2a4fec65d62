"""hidden_channel_conv = 16 (main.py:520; models/upsample.py:38-76, models/resnet.py:12-51): the channel-blocked executor
(linr_pcgc_amd/wide_net.py) against the oracle - forward bits and probabilities, every parameter gradient against autograd,
training steps against torch.optim.Adam on the oracle, and a lossless encode / decode round trip through the codec."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import network as onet          # noqa: E402
from oracle import octree as ooct           # noqa: E402
from gpu_common import C_ROUND, _U, _close, _grads_close_per_tensor, _relu_tie_slack, _smallest_relu_input, _within_rounding          # noqa: E402,F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pkg():
    import linr_pcgc_amd
    from linr_pcgc_amd import _lib
    _lib.lib()
    return linr_pcgc_amd


@pytest.fixture(scope='module')
def shell(golden_dir):
    g = np.load(os.path.join(golden_dir, 'octree_shell128.npz'))
    scales = []
    for s in range(int(g['scale_num'])):
        c = g['s%d_coord' % s]
        scales.append({'coord': c, 'occ': g['s%d_occ' % s], 'offset_tensor': g['s%d_offset' % s], 'scale_idx': s,
                       'nbr': ooct.neighbour_table(c)})
    return {'scales': scales, 'point_num': int(len(g['ori']))}


def _model(hidden, scale_num=5, block_layers=1, seed=8807):
    from linr_pcgc_amd.model_core import LINR_PCGC_Model
    torch.manual_seed(seed)
    model = LINR_PCGC_Model({'scale_num': scale_num, 'in_channel': 7, 'hidden_channel_conv': hidden, 'block_layers': block_layers,
                             'outstage': 8, 'instage': 1})
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return model.cuda(), sd


def test_wide_state_dict_has_the_reference_shapes(pkg):
    """Names and shapes follow models/upsample.py:38-76 / models/resnet.py:12-51 with channels = 16."""
    model, sd = _model(16)
    assert sd['upsampler.block_in.0.kernel'].shape == (27, 8, 16)
    assert sd['upsampler.block_in.2.layers.0.conv0_0.kernel'].shape == (27, 16, 8)
    assert sd['upsampler.block_in.2.layers.0.conv1_0.kernel'].shape == (16, 8)
    assert sd['upsampler.block_in.2.layers.0.conv1_2.kernel'].shape == (8, 8)
    assert sd['upsampler.block_in.3.kernel'].shape == (27, 16, 16)
    assert sd['upsampler.inner_mlps.3.0.0.weight'].shape == (24, 16)
    assert sd['upsampler.prune_blocks.5.0.conv.kernel'].shape == (27, 16, 16)
    assert sd['upsampler.outter_blocks.2.0.kernel'].shape == (27, 3, 16)
    assert len(sd) == 181          # scale_num 5: 1 + 4 x 5 + 14 + 8 x 4 + 8 x 2 + 7 x 14 (189 at scale_num 7), as at width 8
    with pytest.raises(ValueError):
        _model(12)


@pytest.mark.parametrize('hidden,block_layers', [(16, 1), (16, 2), (32, 1), (32, 3)])
def test_wide_forward_and_backward_match_the_oracle(pkg, shell, hidden, block_layers):
    model, sd = _model(hidden, block_layers=block_layers)
    frame = model.make_frame(shell['scales'])
    probs, bits = model.frame_probs(frame)
    tsc = onet.to_torch_scales(shell['scales'])
    ref_bits = 0.0
    for i, s in enumerate(tsc):
        out = onet.forward_scale(sd, s)
        sl = frame.scale_slice(i)
        for k in range(8):
            err = (probs[k, sl].double().cpu() - out['probs'][k].reshape(-1).double()).abs().max()
            assert float(err) <= 1e-4, (i, k, float(err))
        ref_bits += float(out['bits'])
    assert abs(float(bits) - ref_bits) <= 1e-5 * ref_bits, (float(bits), ref_bits)
    probs2, bits2 = model.frame_probs(frame)
    assert torch.equal(probs, probs2) and torch.equal(bits, bits2), 'forward must be bit-reproducible'
    # gradients through the executor's own tape against autograd of the oracle, every tensor against its own largest entry: the direct
    # fp32-vs-fp32 sanity bound (3e-3) and the criterion proper, HIP as close to the float64 oracle as the fp32 oracle is.  The shell
    # cannot be redrawn: its ReLU ties at fp32 resolution enter the float64 bound as slack (at width 32, block_layers 1: one input of
    # 1.3e-7 in head 1's hidden layer on scale 2 moves scale_mlp.2.0.weight's gradient by 5.717e-7 - the HIP's whole difference there)
    gscale = 1.0 / shell['point_num']
    grads = _tape_grads(model, frame, gscale)
    sdo, sd64 = _oracle_grads(sd, shell['scales'], gscale)
    _grads_close_per_tensor(grads, sdo, rtol=3e-3, sd64=sd64, slack=_relu_tie_slack(sd, shell['scales'], gscale))
    assert torch.equal(grads, _tape_grads(model, frame, gscale)), 'backward must be bit-reproducible'


def _tape_grads(model, frame, gscale):
    """d (gscale * bits) / d params through the executor's own tape (forward with keep, backward into the zeroed flat gradient)."""
    model._ensure_grad_views()
    b = torch.zeros(1, dtype=torch.float64, device='cuda')
    with torch.no_grad():
        model._flat_grad.zero_()
        tape = model._wide.forward(frame, 0, 8, None, b, keep=True)
        model._wide.backward(frame, tape, gscale)
    return model._flat_grad.clone()


def _oracle_grads(sd, scales, gscale):
    """Autograd of the oracle's gscale * frame bits with fp32 leaves and with float64 leaves (numpy scales, on the host)."""
    sdo = {k: v.clone().requires_grad_() for k, v in sd.items()}
    (onet.frame_bits(sdo, onet.to_torch_scales(scales)) * gscale).backward()
    sd64 = {k: v.double().clone().requires_grad_() for k, v in sd.items()}
    (onet.frame_bits(sd64, onet.to_torch_scales(scales, torch.float64)) * gscale).backward()
    return sdo, sd64


def test_wide_model_surface_autograd(pkg, shell):
    """loss = model(putin_args); loss.backward() like main.py:457-475, one scale."""
    model, sd = _model(16)
    s = shell['scales'][1]
    dev = 'cuda'
    inargs = {'coord': torch.as_tensor(s['coord']).to(dev), 'offset_tensor': torch.as_tensor(s['offset_tensor']).to(dev),
              'occ_lst': [torch.as_tensor(s['occ'][:, k:k + 1].copy()).to(dev) for k in range(8)], 'scale_idx': 1}
    loss = model(inargs) / 1000.0
    loss.backward()
    sdo = {k: v.clone().requires_grad_() for k, v in sd.items()}
    ref = onet.forward_scale(sdo, onet.to_torch_scales([s])[0])['bits'] / 1000.0
    assert abs(float(loss) - float(ref)) <= 1e-5 * float(ref)
    ref.backward()
    sd64 = {k: v.double().clone().requires_grad_() for k, v in sd.items()}
    (onet.forward_scale(sd64, onet.to_torch_scales([s], torch.float64)[0])['bits'] / 1000.0).backward()
    params = dict(model.named_parameters())
    assert sorted(params) == sorted(sdo)
    grads = torch.cat([params[name].grad.reshape(-1) for name in sdo])          # the oracle's order
    _grads_close_per_tensor(grads, sdo, rtol=3e-3, sd64=sd64, slack=_relu_tie_slack(sd, [s], 1.0 / 1000.0))


def test_wide_train_steps_track_torch_adam_and_decode_losslessly(pkg, shell):
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    model, sd = _model(16)
    frame = model.make_frame(shell['scales'])
    opt = FlatAdam(model)
    sdo = {k: v.clone().requires_grad_() for k, v in sd.items()}
    opt_o = torch.optim.Adam(list(sdo.values()), lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    tsc = onet.to_torch_scales(shell['scales'])
    pn = shell['point_num']
    first = None
    for it in range(4):
        bits = train_step(model, opt, frame, pn)
        opt_o.zero_grad()
        b_o = onet.frame_bits(sdo, tsc)
        (b_o / pn).backward()
        opt_o.step()
        assert abs(float(bits) - float(b_o)) <= 2e-4 * float(b_o), (it, float(bits), float(b_o))
        first = float(bits) if first is None else first
    assert first > 0          # (four Adam steps at lr 0.01 need not lower the loss yet; the oracle's trajectory is the criterion)
    # encoder probabilities == the staged decoder's, decoded occupancy == the input
    probs, _ = model.frame_probs(frame)
    from linr_pcgc_amd.model_core import encode_streams
    p_host = probs.cpu().numpy()
    occ = np.concatenate([s['occ'] for s in shell['scales']], axis=0)
    streams = []
    for i in range(frame.n_scales):
        sl = frame.scale_slice(i)
        streams.append(encode_streams([p_host[k, sl] for k in range(8)], [occ[sl, k].astype(np.uint8) for k in range(8)]))
    dec_frame = model.make_frame([{k: v for k, v in s.items() if k != 'occ'} for s in shell['scales']])
    out = model.decode_frame(dec_frame, streams)
    got = torch.cat(out, dim=1).cpu().numpy()
    assert np.array_equal(got, occ)


def test_wide_gop_encode_decode_roundtrip(pkg):
    """A 2-frame GOP of the 8-bit sphere through overfit -> encode_gop -> decode_gop with hidden_channel_conv = 16: lossless."""
    from linr_pcgc_amd import codec, overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam, LINR_PCGC_Model
    clouds = [synthetic.sequence_frame_device('sphere8', t, 'cuda') for t in range(2)]
    gop = overfit.Gop(None, clouds, None, 64, 'cuda')

    def gen(seed=None):
        if seed is not None:
            torch.manual_seed(seed)
        return LINR_PCGC_Model({'scale_num': gop.scale_num, 'in_channel': 7, 'hidden_channel_conv': 16, 'block_layers': 1,
                                'outstage': 8, 'instage': 1}).cuda()
    model = gen(8807)
    losses = overfit.overfit_gop(model, FlatAdam(model), gop, 3)
    assert losses[-1] < losses[0]
    enc = codec.encode_gop(model, gen(), gop, 8)
    dec = codec.decode_gop(gen(), enc, 'cuda', workers=1)
    for i in range(2):
        ref = torch.as_tensor(gop.infos[i]['ori']).cuda() + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32)
        assert torch.equal(dec[i], ref)


@pytest.mark.parametrize('cin,cout', [(16, 16), (8, 16), (16, 8), (32, 32), (3, 16), (16, 32)])
def test_wide_conv_entries_match_the_oracle_conv(pkg, shell, cin, cout):
    """linr_spconv_wide (forward with bias / residual / ReLU, backward-data with the ReLU mask) and linr_spconv_wgrad_wide against
    oracle.network.conv3 (MinkowskiConvolution kernel_size 3) and its autograd on the finest scale of the
    shell.  Tolerance: fp32 sums of up to 27 x 32 products in a different order (1e-5 relative to the largest entry)."""
    from linr_pcgc_amd import ops
    sc = shell['scales'][0]
    n = len(sc['coord'])
    nbr_o = torch.from_numpy(sc['nbr']).long().cuda()                          # oracle layout [n, 27]
    ld = (n + 63) // 64 * 64
    nbr = torch.full((27, ld), -1, dtype=torch.int32, device='cuda')           # library layout [27, ld]
    nbr[:, :n] = ops.kmap_build(torch.from_numpy(sc['coord']).cuda())
    lo, mask = ops.kmap_compress(nbr, n)
    tile8t = ops.kmap_tile8t(nbr, n)
    torch.manual_seed(cin * 100 + cout)
    W = (torch.randn(27, cin, cout, device='cuda') * 0.1).requires_grad_()
    b = torch.randn(1, cout, device='cuda', requires_grad=True)
    nbi, nbo = (cin + 7) // 8, cout // 8

    def blocks(t, nb):
        """[n, 8 nb] (zero-padded channels) -> blocks: views buf[i, 1:] of [n + 1, 8] buffers whose row 0 is zero."""
        buf = torch.zeros((nb, n + 1, 8), device='cuda')
        for i in range(nb):
            w = min(8, t.shape[1] - 8 * i)
            buf[i, 1:, :w] = t[:, 8 * i:8 * i + w]
        return buf, [buf[i, 1:] for i in range(nb)]

    x = torch.randn(n, cin, device='cuda', requires_grad=True)
    res = torch.randn(n, cout, device='cuda')
    xbuf, xs = blocks(x.detach(), nbi)
    if cin % 8:
        xbuf[-1, 1:, cin % 8:] = 7.0                                           # channels past cin must be ignored
    _, rs = blocks(res, nbo)
    outs = ops.spconv_wide(xs, lo, mask, n, W.detach(), b.detach().reshape(-1), res=rs, relu=True)
    pre = onet.conv3(x, nbr_o, W, b) + res
    ref = torch.relu(pre)
    got = torch.cat(outs, dim=1)
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())

    g = torch.randn(n, cout, device='cuda')
    _, gs = blocks(g, nbo)
    y = onet.conv3(x, nbr_o, W, b)
    gx_ref, gw_ref, gb_ref = torch.autograd.grad(y, [x, W, b], g)
    gw, gb = ops.spconv_wgrad_wide(xs, gs, nbr, tile8t, n, cin, cout)
    assert float((gw - gw_ref).abs().max()) <= 1e-5 * float(gw_ref.abs().max())
    assert float((gb - gb_ref.reshape(-1)).abs().max()) <= 1e-5 * float(gb_ref.abs().max())
    if cin % 8 == 0:
        act = torch.randn(n, cin, device='cuda')
        _, acts = blocks(act, nbi)
        gi = ops.spconv_wide(gs, lo, mask, n, W.detach(), None, bwd=True, act=acts)
        want = gx_ref * (act > 0)
        assert float((torch.cat(gi, dim=1) - want).abs().max()) <= 1e-5 * float(want.abs().max())


def _to_blocks(t, padded=True):
    """[n, 8 nb] -> nb blocks [n, 8] (views buf[i, 1:] of [n + 1, 8] buffers whose row 0 is zero when padded)."""
    n, nb = t.shape[0], t.shape[1] // 8
    buf = torch.zeros((nb, n + 1, 8), device=t.device)
    for i in range(nb):
        buf[i, 1:] = t[:, 8 * i:8 * i + 8]
    return [buf[i, 1:] for i in range(nb)]


@pytest.mark.parametrize('cin,cout,layout', [(16, 8, 'me'), (32, 16, 'me'), (8, 8, 'me'), (16, 16, 'me'), (16, 24, 'torch'), (32, 24, 'torch')])
def test_wide_pointwise_entries_match_torch(pkg, cin, cout, layout):
    """linr_linear_wide (forward with bias / residual / ReLU; backward-data with accumulation and the ReLU mask) and
    linr_linear_wgrad_wide on blocked activations against torch matmuls and autograd (MinkowskiConvolution kernel_size 1:
    models/resnet.py:25-46; nn.Linear of the head: models/upsample.py:73-76).  n = 1000: not a multiple of any tile.  Tolerance: fp32
    sums of <= 32 products in another order (1e-5 of the largest entry); the weight gradients sum 1000 rows (1e-4)."""
    from linr_pcgc_amd import ops
    n = 1000
    torch.manual_seed(7 * cin + cout)
    x = torch.randn(n, cin, device='cuda', requires_grad=True)
    W = (torch.randn((cin, cout) if layout == 'me' else (cout, cin), device='cuda') * 0.3).requires_grad_()
    b = torch.randn(cout, device='cuda', requires_grad=True)
    ws = (cout, 1) if layout == 'me' else (1, cin)
    blocked_out = cout % 8 == 0 and layout == 'me'
    xs = _to_blocks(x.detach())
    res = torch.randn(n, cout, device='cuda')
    y_ref = x @ (W if layout == 'me' else W.t()) + b
    outs = _to_blocks(torch.zeros(n, cout, device='cuda')) if blocked_out else [torch.empty(n, cout, device='cuda')]
    ops.linear_wide(xs, cin, W.detach(), ws[0], ws[1], b.detach(), cout, outs, out_blocked=blocked_out,
                    res=_to_blocks(res) if blocked_out else [res], relu=True)
    want = torch.relu(y_ref + res)
    got = torch.cat(outs, dim=1)
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
    # backward-data (+ old, masked) and the weight gradients
    g = torch.randn(n, cout, device='cuda')
    gx_ref, gw_ref, gb_ref = torch.autograd.grad(y_ref, [x, W, b], g)
    gs = _to_blocks(g) if blocked_out else [g]
    old, act = torch.randn(n, cin, device='cuda'), torch.randn(n, cin, device='cuda')
    gins = _to_blocks(old)
    ops.linear_wide(gs, cout, W.detach(), ws[1], ws[0], None, cin, gins, in_blocked=blocked_out, act=_to_blocks(act), accumulate=True)
    want = (gx_ref + old) * (act > 0)
    assert float((torch.cat(gins, dim=1) - want).abs().max()) <= 1e-5 * float(want.abs().max())
    gw, gb = torch.full_like(W, float('nan')), torch.full_like(b, float('nan'))
    ops.linear_wgrad_wide(xs, cin, gs, cout, gw, ws[0], ws[1], gb, g_blocked=blocked_out)
    assert float((gw - gw_ref).abs().max()) <= 1e-4 * float(gw_ref.abs().max())
    assert float((gb - gb_ref).abs().max()) <= 1e-4 * float(gb_ref.abs().max())
    ops.linear_wgrad_wide(xs, cin, gs, cout, gw, ws[0], ws[1], gb, g_blocked=blocked_out, accumulate=True)       # LINR_ACCUM
    assert float((gw - 2 * gw_ref).abs().max()) <= 2e-4 * float(gw_ref.abs().max())


@pytest.mark.parametrize('C,stages,n', [(16, 8, 1000), (32, 3, 777), (16, 1, 64 * 300 + 5)])
def test_wide_head_entries_match_torch(pkg, C, stages, n):
    """linr_head_wide_fwd (p and the stage's bits) and linr_head_wide_bwd (all stages in one grouped launch: gc and the parameter
    gradients [W1 | b1 | w2 | b2] per stage) against torch: Linear(C, 24) -> ReLU -> Linear(24, 1) -> sigmoid -> BCELoss(sum) / ln 2
    (models/upsample.py:137-161, model_core.py:72-81) and its autograd.  Tolerances: p 1e-6 absolute, bits 1e-6 relative, gradients
    1e-4 of the largest entry (sums over n rows in another order)."""
    from linr_pcgc_amd import ops
    torch.manual_seed(C + stages)
    occ = (torch.rand(n, 8, device='cuda') < 0.4).float()
    per = 24 * C + 49
    grads = torch.full((stages * per,), float('nan'), device='cuda')
    cs, ps, gcs, params, refs = [], [], [], [], []
    bits = torch.zeros(1, dtype=torch.float64, device='cuda')
    bits_ref = 0.0
    gscale = 0.37
    for k in range(stages):
        c = torch.randn(n, C, device='cuda', requires_grad=True)
        w1 = (torch.randn(24, C, device='cuda') * 0.3).requires_grad_()
        b1 = (torch.randn(24, device='cuda') * 0.3).requires_grad_()
        w2 = (torch.randn(1, 24, device='cuda') * 0.3).requires_grad_()
        b2 = (torch.randn(1, device='cuda') * 0.3).requires_grad_()
        z = torch.relu(c @ w1.t() + b1) @ w2.t() + b2
        p_ref = torch.sigmoid(z).reshape(-1)
        nats = torch.nn.functional.binary_cross_entropy(p_ref, occ[:, k], reduction='sum')
        bits_ref += float(nats) / np.log(2.0)
        refs.append(torch.autograd.grad(nats * gscale, [c, w1, b1, w2, b2]))
        blocks = _to_blocks(c.detach())
        p = torch.empty(n, device='cuda')
        ops.head_wide_fwd(blocks, w1.detach(), b1.detach(), w2.detach(), b2.detach(), occ[:, k], p, bits)
        assert float((p - p_ref).abs().max()) <= 1e-6
        cs.append(blocks); ps.append(p); gcs.append(_to_blocks(torch.zeros(n, C, device='cuda')))
        params.append((w1.detach(), b1.detach(), w2.detach()))
    assert abs(float(bits) - bits_ref) <= 1e-6 * bits_ref
    p_only = torch.empty(n, device='cuda')                      # without a target: probabilities only (the decoder's call)
    ops.head_wide_fwd(cs[0], params[0][0], params[0][1], params[0][2], torch.zeros(1, device='cuda'), None, p_only)
    ops.head_wide_bwd(cs, ps, [occ[:, k] for k in range(stages)], [q[0] for q in params], [q[1] for q in params], [q[2] for q in params],
                      gscale, gcs, grads)
    for k in range(stages):
        gc_ref, gw1, gb1, gw2, gb2 = refs[k]
        got = torch.cat(gcs[k], dim=1)
        assert float((got - gc_ref).abs().max()) <= 1e-5 * float(gc_ref.abs().max())
        want = torch.cat([gw1.reshape(-1), gb1, gw2.reshape(-1), gb2])
        assert float((grads[k * per:(k + 1) * per] - want).abs().max()) <= 1e-4 * float(want.abs().max())


def test_wide_deferred_reductions_equal_the_immediate_ones(pkg, shell):
    """linr_wide_reduce_many over the partials that linr_spconv_wgrad_wide / linr_linear_wgrad_wide leave behind with gW = NULL gives the
    bits of the entries' own reductions (same slab, same fixed-order sums), for several layers in ONE launch."""
    from linr_pcgc_amd import ops
    sc = shell['scales'][0]
    n = len(sc['coord'])
    ld = (n + 63) // 64 * 64
    nbr = torch.full((27, ld), -1, dtype=torch.int32, device='cuda')
    nbr[:, :n] = ops.kmap_build(torch.from_numpy(sc['coord']).cuda())
    tile8t = ops.kmap_tile8t(nbr, n)
    torch.manual_seed(5)
    deferred, want, got = [], [], []
    for cin, cout in [(16, 16), (3, 16), (32, 8), (16, 32)]:
        xs, gs = _to_blocks(torch.randn(n, (cin + 7) // 8 * 8, device='cuda')), _to_blocks(torch.randn(n, cout, device='cuda'))
        want.append(ops.spconv_wgrad_wide(xs, gs, nbr, tile8t, n, cin, cout))
        gw, gb = torch.full((27, cin, cout), float('nan'), device='cuda'), torch.full((cout,), float('nan'), device='cuda')
        ops.spconv_wgrad_wide(xs, gs, nbr, tile8t, n, cin, cout, gw=gw, gb=gb, defer=deferred)
        got.append((gw, gb))
    for cin, cout, ws in [(16, 8, (8, 1)), (32, 16, (16, 1)), (16, 24, (1, 16))]:
        blocked = cout % 8 == 0 and ws[1] == 1
        xs = _to_blocks(torch.randn(n, cin, device='cuda'))
        g = torch.randn(n, cout, device='cuda')
        gs = _to_blocks(g) if blocked else [g]
        a = (torch.full((cin * cout,), float('nan'), device='cuda'), torch.full((cout,), float('nan'), device='cuda'))
        b = (torch.full((cin * cout,), float('nan'), device='cuda'), torch.full((cout,), float('nan'), device='cuda'))
        ops.linear_wgrad_wide(xs, cin, gs, cout, a[0], ws[0], ws[1], a[1], g_blocked=blocked)
        ops.linear_wgrad_wide(xs, cin, gs, cout, b[0], ws[0], ws[1], b[1], g_blocked=blocked, defer=deferred)
        want.append(a); got.append(b)
    assert len(deferred) == 7 and bool(torch.isnan(got[0][0]).all())
    ops.wide_reduce_many(deferred)
    assert deferred == []
    for (w0, w1), (g0, g1) in zip(want, got):
        assert torch.equal(w0, g0) and torch.equal(w1, g1)


def test_sum_many_adds_in_list_order(pkg):
    """linr_sum_many: dst (+)= src[0] + src[1] + ... with the sources added in list order - bitwise what chained additions give."""
    import ctypes
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    torch.manual_seed(3)
    n = 4 * 12345
    srcs = [torch.randn(n, device='cuda') for _ in range(7)]
    dst = torch.randn(n, device='cuda')
    want = dst.clone()
    for t in srcs:
        want = want + t
    arr = (ctypes.c_void_p * 7)(*[t.data_ptr() for t in srcs])
    _lib.check(L.linr_sum_many(arr, 7, n, dst.data_ptr(), 1, torch.cuda.current_stream().cuda_stream), 'linr_sum_many')
    assert torch.equal(dst, want)
    _lib.check(L.linr_sum_many(arr, 3, n, dst.data_ptr(), 0, torch.cuda.current_stream().cuda_stream), 'linr_sum_many')
    assert torch.equal(dst, (srcs[0] + srcs[1]) + srcs[2])


def test_wide_results_do_not_depend_on_leftover_onchip_state(pkg):
    """The wide executor's kernels may not read LDS or registers they did not write (tests/test_gpu_parity.py::
    test_results_do_not_depend_on_leftover_onchip_state for the 8-wide executor): with every entry of csrc/wide.hip preceded by the
    kernel that fills the LDS and vector registers of all CUs with 0xFFFFFFFF (linr_debug_poison bit 16; the scale context's kernels:
    bits 11, 12) three training steps at width 16 give the same parameters, moments and bits, bit for bit."""
    from linr_pcgc_amd import _lib, overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    gop = overfit.Gop(None, [synthetic.sequence_frame_device('sphere8', 0, 'cuda')], None, 64, 'cuda')
    L = _lib.lib()

    def run(mask):
        m = overfit.gen_model(gop.scale_num, 'cuda', seed=8807, hidden=16)
        o = FlatAdam(m)
        bits = torch.zeros(3, dtype=torch.float64, device='cuda')
        L.linr_debug_poison(mask)
        try:
            for s in range(3):
                train_step(m, o, gop.frames[0], gop.point_nums[0], out=bits[s:s + 1])
            torch.cuda.synchronize()
        finally:
            L.linr_debug_poison(0x1FFFF if os.environ.get('LINR_DEBUG_POISON') else 0)
        return m.flat_parameters().clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), bits.cpu()
    clean, dirty = run(0), run(0x1FFFF)
    assert bool(torch.isfinite(dirty[0]).all())
    for a, b in zip(clean, dirty):
        assert torch.equal(a, b)


@pytest.mark.parametrize('hidden,block_layers', [(16, 1), (32, 1), (16, 2), (32, 3)])
def test_wide_fused_pointwise_epilogues_equal_the_separate_launches(pkg, hidden, block_layers):
    """conv1_0 / conv1_2 of a wide Inception layer and their backward-data passes in the convolutions' epilogues (linr_spconv_wide's pw)
    keep the fmaf chains of the stand-alone pointwise kernel: two training steps give the same parameters, moments and bits, bit for
    bit, as with LINR_WIDE_FUSE_PW=0 (fuse_pw False on the executor: one launch per pointwise layer)."""
    from linr_pcgc_amd import overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    gop = overfit.Gop(None, [synthetic.sequence_frame_device('sphere8', 0, 'cuda')], None, 64, 'cuda', block_layers=block_layers)

    def run(fuse):
        m = overfit.gen_model(gop.scale_num, 'cuda', seed=8807, hidden=hidden, block_layers=block_layers)
        m._wide.fuse_pw = fuse
        o = FlatAdam(m)
        bits = torch.zeros(2, dtype=torch.float64, device='cuda')
        for s in range(2):
            train_step(m, o, gop.frames[0], gop.point_nums[0], out=bits[s:s + 1])
        torch.cuda.synchronize()
        return m.flat_parameters().clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), bits.cpu()
    a, b = run(True), run(False)
    assert bool(torch.isfinite(a[0]).all())
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_wide_passes_of_two_models_and_frames_do_not_leak_into_each_other(pkg):
    """What a pass runs on travels in the pass object and nowhere else: between the training forward and the backward of a 'bf16-mul'
    model A on one frame, a plain fp32 model B runs a forward on ANOTHER frame on the same thread.  A's gradient and bits are bitwise
    those of the undisturbed pass (its backward still sees its own frame's tables, bf16 products and a fresh deferred list) and B's
    probabilities are bitwise those of B alone (fp32 products, its own frame)."""
    from linr_pcgc_amd import overfit, synthetic
    gop = overfit.Gop(None, [synthetic.sequence_frame_device('sphere8', t, 'cuda') for t in (0, 1)], None, 64, 'cuda', block_layers=1)
    fa, fb = gop.frames
    assert fa.rows != fb.rows
    A = overfit.gen_model(gop.scale_num, 'cuda', seed=8807, hidden=16)
    A.train_precision = 'bf16-mul'
    B = overfit.gen_model(gop.scale_num, 'cuda', seed=4242, hidden=16)

    def train_pass(between):
        A._ensure_grad_views()
        bits = torch.zeros(1, dtype=torch.float64, device='cuda')
        with torch.no_grad():
            A._flat_grad.zero_()
            tape = A._wide.forward(fa, 0, 8, None, bits, keep=True)
            other = between()
            A._wide.backward(fa, tape, 1.0 / gop.point_nums[0])
        return A._flat_grad.clone(), bits, other
    g_alone, bits_alone, _ = train_pass(lambda: None)
    p_alone, pbits_alone = B.frame_probs(fb)
    g, bits, (p, pbits) = train_pass(lambda: B.frame_probs(fb))
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert torch.equal(g, g_alone) and torch.equal(bits, bits_alone)
    assert torch.equal(p, p_alone) and torch.equal(pbits, pbits_alone)


# ---- tiny, ragged and multi-tile frames ------------------------------------------------------------------------------------------------
def _empty_scale(idx):
    return {'coord': np.zeros((0, 3), np.int32), 'occ': np.zeros((0, 8), np.float32), 'offset_tensor': np.zeros((0, 7), np.float32),
            'scale_idx': idx}


@pytest.mark.parametrize('n', [1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1025])
@pytest.mark.parametrize('hidden,block_layers', [(16, 2), (32, 1)])
def test_wide_tiny_and_ragged_frames(pkg, hidden, block_layers, n):
    """tests/test_gpu_configs.py::test_tiny_and_ragged_frames for the channel-blocked executor: one scale of n voxels beside a zero-row
    scale, n around the 8-row weight-gradient tiles (wwgrad_k), the 64-lane waves and the 256-row convolution / head / pointwise tiles,
    so most of the 256 persistent weight-gradient blocks and of the pointwise slab rows are empty.  Bits and probabilities against the
    oracle, every gradient (the tape's) against the float64-anchored criterion - the absent scale's MLP gradients exactly zero - and the
    staged forward bitwise equal to the one-shot one.  A cloud with a ReLU tie at fp32 resolution is redrawn (the criterion is the
    oracle's, not the kernels'); where six draws all have one (n = 1025: ~1e6 ReLU inputs) the last one's ties enter as slack."""
    model, sd = _model(hidden, scale_num=3, block_layers=block_layers)
    side = max(6, int(round((3 * n) ** (1 / 3))) + 2)          # a box that holds n distinct voxels at ~1/3 occupancy
    want = n
    for attempt in range(6):
        rng = np.random.default_rng(want + 1000 * attempt + hidden)
        c = ooct.unique_sorted(rng.integers(0, side, size=(4 * want, 3)))[:want]
        n = len(c)
        sc = {'coord': c, 'occ': (rng.random((n, 8)) < 0.5).astype(np.float32), 'offset_tensor': ooct.offset_tensor(c), 'scale_idx': 1,
              'nbr': ooct.neighbour_table(c)}
        if _smallest_relu_input(sd, sc) >= 3e-7:
            break
    assert n == want
    frame = model.make_frame([{k: v for k, v in sc.items() if k != 'nbr'}, _empty_scale(0)])
    assert frame.rows == n
    probs, bits = model.frame_probs(frame)
    out = onet.forward_scale(sd, onet.to_torch_scales([sc])[0])
    assert abs(float(bits) - float(out['bits'])) <= 1e-5 * float(out['bits']), (float(bits), float(out['bits']))
    for k in range(8):
        _close(probs[k], out['probs'][k].reshape(-1), 1e-4, 1e-4, 'probs of stage %d' % k)
    staged = torch.empty_like(probs)
    for k in range(8):
        model._stage_forward(frame, k, k + 1, staged, None, 'f32')
    assert torch.equal(probs, staged)
    grads = _tape_grads(model, frame, 1.0)
    assert bool(torch.isfinite(grads).all())
    sdo, sd64 = _oracle_grads(sd, [sc], 1.0)
    assert sdo['scale_mlp.0.0.weight'].grad is None          # the zero-row scale: no gradient at all, the executor's must be zero
    _grads_close_per_tensor(grads, sdo, sd64=sd64, slack=_relu_tie_slack(sd, [sc]))


@pytest.mark.parametrize('hidden', [16, 32])
def test_wide_ragged_multi_scale_frame_with_colliding_coordinates(pkg, hidden):
    """tests/test_gpu_configs.py::test_ragged_multi_scale_frame_with_colliding_coordinates for the channel-blocked executor: three scales
    of 257, 65 and 3 rows from the SAME 9^3 box batched at offsets that are no multiple of any tile; a voxel of one scale must not become
    a neighbour of another scale's.  Per-scale probabilities, the summed bits and every gradient (float64-anchored) against the oracle;
    ties that six draws cannot avoid enter as slack."""
    model, sd = _model(hidden, scale_num=3)
    for attempt in range(6):
        rng = np.random.default_rng(77 + attempt)
        scales = []
        for idx, n in ((0, 257), (1, 65), (2, 3)):
            c = ooct.unique_sorted(rng.integers(0, 9, size=(4 * n, 3)))[:n]
            scales.append({'coord': c, 'occ': (rng.random((len(c), 8)) < 0.5).astype(np.float32), 'offset_tensor': ooct.offset_tensor(c),
                           'scale_idx': idx, 'nbr': ooct.neighbour_table(c)})
        if min(_smallest_relu_input(sd, s) for s in scales) >= 3e-7:
            break
    frame = model.make_frame([{k: v for k, v in s.items() if k != 'nbr'} for s in scales])
    assert frame.rows == 325
    probs, bits = model.frame_probs(frame)
    ref = 0.0
    for i, s in enumerate(onet.to_torch_scales(scales)):
        out = onet.forward_scale(sd, s)
        sl = frame.scale_slice(i)
        for k in range(8):
            _close(probs[k, sl], out['probs'][k].reshape(-1), 1e-4, 1e-4, 'probs of scale %d, stage %d' % (i, k))
        ref += float(out['bits'])
    assert abs(float(bits) - ref) <= 1e-5 * ref, (float(bits), ref)
    grads = _tape_grads(model, frame, 1.0)
    sdo, sd64 = _oracle_grads(sd, scales, 1.0)
    _grads_close_per_tensor(grads, sdo, sd64=sd64, slack=_relu_tie_slack(sd, scales))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope='module')
def sphere9(pkg):
    """A 9-bit sphere shell (501,702 points; 7 scales, 215,286 rows, the finest 156,985): more rows than 2 workgroups per CU x 256, so
    the convolutions' workgroups loop over several row tiles and the pointwise weight gradients run their full 512 slab rows."""
    from linr_pcgc_amd import synthetic
    from linr_pcgc_amd.module_utils import prepare_frame
    pts = synthetic.sequence_frame({'bitdepth': 9, 'radius': 200, 'thickness': 0.5}, 0)
    return prepare_frame(pts, None, 64, device='cuda')


class _NoTF32:
    """fp32 matmuls of the GPU oracle in fp32 proper."""

    def __enter__(self):
        self.old = torch.backends.cuda.matmul.allow_tf32
        torch.backends.cuda.matmul.allow_tf32 = False

    def __exit__(self, *exc):
        torch.backends.cuda.matmul.allow_tf32 = self.old


def test_wide_multi_tile_frame_matches_the_oracle(pkg, sphere9):
    """The whole width-16 network on a frame of more than 2 x CUs x 256 rows (checked here, on any card): every convolution's
    workgroups walk several 256-row tiles, the weight-gradient blocks many 8-row tiles, the pointwise slabs all 512 rows.  Forward bits
    and probabilities, and every gradient of the training loss (bits / points) with the float64 anchor; the fp32 and float64 oracles run
    on the GPU, their backward one scale at a time (the im2col columns of one scale alive at once).  Measured on the MI355X: 119 s,
    peak 20.5 GB of device memory; worst fp32-vs-fp32 gradient difference 2.8e-4 of its tensor's largest entry."""
    import time
    t0 = time.perf_counter()
    torch.cuda.reset_peak_memory_stats()
    fr = sphere9
    model, sd = _model(16, scale_num=fr['scale_num'])
    frame = model.make_frame(fr['all_input_info'])
    assert frame.rows > 2 * _cus() * 256, (frame.rows, _cus())
    probs, bits = model.frame_probs(frame)
    gscale = 1.0 / fr['point_num']
    grads = _tape_grads(model, frame, gscale)
    sdo = {k: v.cuda().requires_grad_() for k, v in sd.items()}
    sd64 = {k: v.double().cuda().requires_grad_() for k, v in sd.items()}
    ref = 0.0
    with _NoTF32():
        for i, info in enumerate(fr['all_input_info']):
            nbr = torch.from_numpy(ooct.neighbour_table(info['coord'].cpu().numpy().astype(np.int32))).long().cuda()
            sl = frame.scale_slice(i)
            for leaves, dt in ((sdo, torch.float32), (sd64, torch.float64)):
                s = {'offset_tensor': info['offset_tensor'].to(dt), 'occ': info['occ'].to(dt), 'nbr': nbr, 'scale_idx': info['scale_idx']}
                out = onet.forward_scale(leaves, s)
                if dt == torch.float32:
                    for k in range(8):
                        _close(probs[k, sl], out['probs'][k].reshape(-1), 1e-4, 1e-4, 'probs of scale %d, stage %d' % (i, k))
                    ref += float(out['bits'])
                (out['bits'] * gscale).backward()
                del out
    assert abs(float(bits) - ref) <= 1e-5 * ref, (float(bits), ref)
    worst = _grads_close_per_tensor(grads, sdo, rtol=3e-3, sd64=sd64)
    print('multi-tile frame: %d rows, worst fp32-vs-fp32 gradient difference %.3e of its tensor\'s largest entry (%s); %.1f s, peak %.1f GB'
          % (frame.rows, worst[0], worst[1], time.perf_counter() - t0, torch.cuda.max_memory_allocated() / 2 ** 30))


# Op level at the multi-tile size: per-entry rounding bounds against float64 (C_ROUND, _within_rounding: tests/gpu_common.py).


def _nan_blocks(n, nb):
    return [torch.full((n, 8), float('nan'), device='cuda') for _ in range(nb)]


def _padded_blocks(t, nb):
    """[n, c <= 8 nb] -> nb blocks (views buf[i, 1:] of [n + 1, 8] buffers whose row 0 is zero; channels past c zero)."""
    n = t.shape[0]
    buf = torch.zeros((nb, n + 1, 8), device=t.device)
    for i in range(nb):
        w = min(8, t.shape[1] - 8 * i)
        buf[i, 1:, :w] = t[:, 8 * i:8 * i + w]
    return buf, [buf[i, 1:] for i in range(nb)]


@pytest.fixture(scope='module')
def finest9(sphere9):
    """The finest scale of the 9-bit shell: coordinates, the oracle's [n, 27] map and the library's maps."""
    from linr_pcgc_amd import ops
    c = sphere9['all_input_info'][0]['coord']
    n = c.shape[0]
    assert n > 2 * _cus() * 256, (n, _cus())
    ld = (n + 63) // 64 * 64
    nbr = torch.full((27, ld), -1, dtype=torch.int32, device='cuda')
    nbr[:, :n] = ops.kmap_build(c.to(torch.int32).contiguous())
    lo, mask = ops.kmap_compress(nbr, n)
    return {'n': n, 'nbr_o': torch.from_numpy(ooct.neighbour_table(c.cpu().numpy().astype(np.int32))).long().cuda(), 'nbr': nbr,
            'lo': lo, 'mask': mask, 'tile8t': ops.kmap_tile8t(nbr, n)}


@pytest.mark.parametrize('cin,cout', [(16, 16), (8, 16), (16, 8), (32, 32), (3, 16), (16, 32)])
def test_wide_conv_entries_multi_tile_against_float64(pkg, finest9, cin, cout):
    """test_wide_conv_entries_match_the_oracle_conv on the finest scale of the 9-bit shell (> 2 x CUs x 256 rows: the workgroups of
    linr_spconv_wide walk several tiles): forward with bias / residual / ReLU, backward-data with the ReLU mask, and the tiled one-launch
    weight gradient (linr_spconv_wgrad_wide: 256 blocks over ~600 rows each) against the float64 oracle.conv3 and its autograd on the
    GPU, every entry within its own rounding bound."""
    from linr_pcgc_amd import ops
    m = finest9
    n, nbr_o = m['n'], m['nbr_o']
    torch.manual_seed(cin * 100 + cout)
    W = torch.randn(27, cin, cout, device='cuda') * 0.1
    b = torch.randn(cout, device='cuda')
    x = torch.randn(n, cin, device='cuda')
    res = torch.randn(n, cout, device='cuda')
    g = torch.randn(n, cout, device='cuda')
    nbi, nbo = (cin + 7) // 8, cout // 8
    xbuf, xs = _padded_blocks(x, nbi)
    if cin % 8:
        xbuf[-1, 1:, cin % 8:] = 7.0                                           # channels past cin must be ignored
    W64, b64, x64 = W.double().requires_grad_(), b.double().reshape(1, -1).requires_grad_(), x.double().requires_grad_()
    outs = ops.spconv_wide(xs, m['lo'], m['mask'], n, W, b, res=_padded_blocks(res, nbo)[1], relu=True, outs=_nan_blocks(n, nbo))
    y64 = onet.conv3(x64, nbr_o, W64, b64)
    with torch.no_grad():
        exact = torch.relu(y64 + res.double())
        absum = onet.conv3(x64.abs(), nbr_o, W64.abs(), b64.abs()) + res.double().abs()
    worst = [_within_rounding(torch.cat(outs, dim=1), exact, absum, 'forward')]

    gx, gw, gb = torch.autograd.grad(y64, [x64, W64, b64], g.double())
    wabs = W64.detach().abs().requires_grad_()
    xabs = x64.detach().abs().requires_grad_()
    gabs = g.double().abs()
    gx_abs, gw_abs = torch.autograd.grad(onet.conv3(xabs, nbr_o, wabs, torch.zeros_like(b64)), [xabs, wabs], gabs)
    gws, gbs = torch.full((27, cin, cout), float('nan'), device='cuda'), torch.full((cout,), float('nan'), device='cuda')
    ops.spconv_wgrad_wide(xs, _to_blocks(g), m['nbr'], m['tile8t'], n, cin, cout, gw=gws, gb=gbs)
    worst.append(_within_rounding(gws, gw, gw_abs, 'kernel gradient'))
    worst.append(_within_rounding(gbs, gb.reshape(-1), gabs.sum(0), 'bias gradient'))
    if cin % 8 == 0:
        act = torch.randn(n, cin, device='cuda')
        gi = ops.spconv_wide(_to_blocks(g), m['lo'], m['mask'], n, W, None, bwd=True, act=_to_blocks(act), outs=_nan_blocks(n, nbi))
        worst.append(_within_rounding(torch.cat(gi, dim=1), gx * (act > 0), gx_abs, 'backward-data'))
    print('conv %d -> %d at %d rows: worst entry at %s of its bound' % (cin, cout, n, ['%.3g' % w for w in worst]))


@pytest.mark.parametrize('h', [8, 16])
def test_wide_paired_wgrad_multi_tile_against_float64(pkg, finest9, h):
    """linr_spconv_wgrad_wide2 (conv0_1 and conv1_1 of an Inception layer as one launch) and the deferred reductions of its shared slab
    (linr_wide_reduce_many, row stride = the pair's) on the finest scale of the 9-bit shell, against float64 autograd of oracle.conv3."""
    from linr_pcgc_amd import ops
    m = finest9
    n, nbr_o = m['n'], m['nbr_o']
    torch.manual_seed(h)
    outs, worst = [], []
    for _ in range(2):
        x, g = torch.randn(n, h, device='cuda'), torch.randn(n, h, device='cuda')
        gw, gb = torch.full((27, h, h), float('nan'), device='cuda'), torch.full((h,), float('nan'), device='cuda')
        outs.append((x, g, gw, gb))
    deferred = []
    (xa, ga, gwa, gba), (xb, gb_, gwb, gbb) = outs
    ops.spconv_wgrad_wide2(_to_blocks(xa), _to_blocks(ga), gwa, gba, _to_blocks(xb), _to_blocks(gb_), gwb, gbb, m['tile8t'], n, deferred)
    assert len(deferred) == 2
    ops.wide_reduce_many(deferred)
    for which, (x, g, gw, gb) in zip('AB', outs):
        W64 = torch.zeros(27, h, h, dtype=torch.float64, device='cuda', requires_grad=True)
        b64 = torch.zeros(1, h, dtype=torch.float64, device='cuda', requires_grad=True)
        gw64, gb64 = torch.autograd.grad(onet.conv3(x.double(), nbr_o, W64, b64), [W64, b64], g.double())
        gw_abs = torch.autograd.grad(onet.conv3(x.double().abs(), nbr_o, W64, b64), [W64], g.double().abs())[0]
        worst.append(_within_rounding(gw, gw64, gw_abs, 'kernel gradient ' + which))
        worst.append(_within_rounding(gb, gb64.reshape(-1), g.double().abs().sum(0), 'bias gradient ' + which))
    print('paired weight gradients h = %d at %d rows: worst entry at %s of its bound' % (h, n, ['%.3g' % w for w in worst]))


@pytest.mark.parametrize('cin,cout,layout', [(16, 8, 'me'), (32, 16, 'me'), (8, 8, 'me'), (16, 16, 'me'), (16, 24, 'torch'), (32, 24, 'torch')])
def test_wide_pointwise_entries_multi_tile_against_float64(pkg, cin, cout, layout):
    """test_wide_pointwise_entries_match_torch at n = 196,685 (> 512 x 256: all 512 slab rows of the weight gradient, each over several
    256-row tiles; no multiple of any tile): linr_linear_wide forward (bias / residual / ReLU) and backward-data (+ old, masked),
    linr_linear_wgrad_wide with its own reduction and deferred into linr_wide_reduce_many - every entry within its rounding bound of the
    float64 result."""
    from linr_pcgc_amd import ops
    n = 3 * 65536 + 77
    torch.manual_seed(7 * cin + cout + 1)
    x = torch.randn(n, cin, device='cuda')
    W = torch.randn((cin, cout) if layout == 'me' else (cout, cin), device='cuda') * 0.3
    b = torch.randn(cout, device='cuda')
    Wm = (W if layout == 'me' else W.t()).double()                             # [cin, cout]
    ws = (cout, 1) if layout == 'me' else (1, cin)
    blocked_out = cout % 8 == 0 and layout == 'me'
    res = torch.randn(n, cout, device='cuda')
    outs = _nan_blocks(n, cout // 8) if blocked_out else [torch.full((n, cout), float('nan'), device='cuda')]
    ops.linear_wide(_to_blocks(x), cin, W, ws[0], ws[1], b, cout, outs, out_blocked=blocked_out,
                    res=_to_blocks(res) if blocked_out else [res], relu=True)
    x64, r64 = x.double(), res.double()
    worst = [_within_rounding(torch.cat(outs, dim=1), torch.relu(x64 @ Wm + b.double() + r64),
                              x64.abs() @ Wm.abs() + b.double().abs() + r64.abs(), 'forward')]
    g = torch.randn(n, cout, device='cuda')
    gs = _to_blocks(g) if blocked_out else [g]
    g64 = g.double()
    old, act = torch.randn(n, cin, device='cuda'), torch.randn(n, cin, device='cuda')
    gins = _to_blocks(old)
    ops.linear_wide(gs, cout, W, ws[1], ws[0], None, cin, gins, in_blocked=blocked_out, act=_to_blocks(act), accumulate=True)
    worst.append(_within_rounding(torch.cat(gins, dim=1), (g64 @ Wm.t() + old.double()) * (act > 0),
                                  g64.abs() @ Wm.abs().t() + old.double().abs(), 'backward-data'))
    gw_exact, gb_exact = x64.t() @ g64, g64.sum(0)
    gw_abs, gb_abs = x64.abs().t() @ g64.abs(), g64.abs().sum(0)
    if layout == 'torch':
        gw_exact, gw_abs = gw_exact.t(), gw_abs.t()
    deferred = []
    for defer in (None, deferred):
        gw, gb = torch.full_like(W, float('nan')), torch.full_like(b, float('nan'))
        ops.linear_wgrad_wide(_to_blocks(x), cin, gs, cout, gw, ws[0], ws[1], gb, g_blocked=blocked_out, defer=defer)
        if defer is not None:
            assert len(deferred) == 1 and bool(torch.isnan(gw).all())
            ops.wide_reduce_many(deferred)
        what = 'deferred ' if defer is not None else ''
        worst.append(_within_rounding(gw, gw_exact, gw_abs, what + 'weight gradient'))
        worst.append(_within_rounding(gb, gb_exact, gb_abs, what + 'bias gradient'))
    print('pointwise %d -> %d (%s) at %d rows: worst entry at %s of its bound' % (cin, cout, layout, n, ['%.3g' % w for w in worst]))
