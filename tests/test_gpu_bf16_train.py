"""GPU tests of the bf16 TRAINING executor (BASELINE config[4] "bf16 SparseConv"; csrc/train_bf16.hip: linr_net_forward_train_bf16,
linr_net_backward_bf16, linr_net_train_step_bf16, linr_spconv_bwd_fused_bf16) - the overfit step of main.py:305-321 with bf16
feature / gradient rows, fp32 master parameters and fp32 accumulation, beside the fp32 executor.

The reference trains in fp32 only (MinkowskiEngine, models/resnet.py:12-60, models/upsample.py:88-97,137-217), so there is nothing
of it to compare a reduced-precision step with; what is checked, with the tolerances written here:
  * against the emulating oracle (oracle/network_bf16.py: train_forward_scale - the same roundings at the same points through
    autograd, another fp32 summation order): logits |d| <= 2e-2, bits rel <= 1e-3, every one of the 189 gradient tensors within
    2e-2 of ITS OWN largest entry;
  * against the fp32 oracle (oracle/network.py): bits within 1 %, the whole gradient vector at cosine >= 0.999 (every tensor >= 0.99);
  * the fused backward of one convolution as a stand-alone op against torch autograd on bf16-representable inputs: input
    gradient within one bf16 rounding, kernel / bias gradients within 1e-4 of their own largest entry (their products are exact
    in fp32; only the summation order differs);
  * four Adam steps track torch.optim.Adam on the emulating oracle; run-to-run bit-identical; a complete small overfit reaches
    the fp32 executor's bits/point within +1 % over three seeds and decodes losslessly through the bf16 / uint8-weight codec.
The forward and gradient checks of this file run on the golden shell (6,821 rows, finest scale 4,983) and on frames of 1 to 257 rows:
every backward kernel has ONE tile per wave there.  The sizes at which bbwd_k, bocc_wgrad7_k, thead_bwd_k and bocc7m_k walk several
tiles and wgrad_reduce_k takes its unrolled branch (32,900 and 131,329 rows on 256 CUs) are held to the emulating oracle and to the
sum of their scales' alone-frame gradients by tests/test_gpu_bf16_train_tiles.py.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import network as onet          # noqa: E402
from oracle import network_bf16 as obf      # noqa: E402
from oracle import octree as ooct           # noqa: E402
from gpu_common import _model_and_oracle, ADAM_DEFAULT, ADAM_DISTINCT, ADAM_DISTINCT_GSCALE_DIV    # noqa: E402


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bf16_bits(t):
    """float32 tensor (bf16-representable) -> int16 tensor of its bf16 bit patterns"""
    return t.to(torch.bfloat16).view(torch.int16)


def _from_bits(t):
    return t.view(torch.bfloat16).float()


def _logits(p):
    p = p.double()
    return torch.log(p) - torch.log1p(-p)


@pytest.fixture(scope='module')
def env(golden_dir):
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from linr_pcgc_amd import _lib, ops
    g = np.load(os.path.join(golden_dir, 'octree_shell128.npz'))
    dev = torch.device('cuda:0')
    out = []
    for s in (0, 2):                                   # the finest scale (ragged last tile) and a small one
        coord = g['s%d_coord' % s]
        nbr = ops.kmap_build(torch.from_numpy(coord).to(dev))
        lo, mask = ops.kmap_compress(nbr)
        out.append({'n': len(coord), 'lo': lo, 'mask': mask, 'ld': nbr.shape[1], 'nbr_t': torch.from_numpy(ooct.neighbour_table(coord)).long()})
    return {'L': _lib.lib(), 'lib': _lib, 'dev': dev, 'scales': out}


@pytest.mark.parametrize('which,nblocks', [(0, 256), (0, 2), (1, 256)])
def test_conv88_backward_fused_bf16_op(env, which, nblocks):
    """linr_spconv_bwd_fused_bf16: backward-data + kernel / bias gradient of a convolution 8->8 from ONE gather of the output
    gradient, bf16 rows in and out (ME.MinkowskiConvolution's backward under autograd, models/resnet.py:15-51)."""
    e = env['scales'][which]
    dev, n, L = env['dev'], e['n'], env['L']
    gen = torch.Generator().manual_seed(4100 + nblocks + which)
    x_h = obf.rb(torch.randn(n, 8, generator=gen))
    go_h = obf.rb(torch.randn(n, 8, generator=gen))
    w_h = torch.randn(27, 8, 8, generator=gen) * 0.2
    xo = x_h.clone().requires_grad_()
    wo = w_h.clone().requires_grad_()
    bo = torch.zeros(1, 8, requires_grad=True)
    obf.conv3t(xo, e['nbr_t'], wo, bo).backward(go_h)
    go = torch.zeros((n + 1, 8), dtype=torch.int16, device=dev)
    go[1:] = _bf16_bits(go_h).to(dev)
    x = torch.zeros((n + 1, 8), dtype=torch.int16, device=dev)
    x[1:] = _bf16_bits(x_h).to(dev)
    gin = torch.full((n + 1, 8), 0x7fc0, dtype=torch.int16, device=dev)          # NaN pattern: every row must be written
    w = w_h.to(dev).contiguous()
    slab = torch.full((nblocks, 1736), float('nan'), device=dev)
    rows = ctypes.c_int32(0)
    env['lib'].check(L.linr_spconv_bwd_fused_bf16(go[1:].data_ptr(), x[1:].data_ptr(), e['lo'].data_ptr(), e['mask'].data_ptr(),
                                                  e['ld'], n, w.data_ptr(), gin[1:].data_ptr(), slab.data_ptr(), nblocks,
                                                  ctypes.byref(rows), _stream()), 'linr_spconv_bwd_fused_bf16')
    torch.cuda.synchronize()
    r = rows.value
    assert 1 <= r <= nblocks
    assert bool(torch.isfinite(slab[:r]).all()) and bool(torch.isnan(slab[r:]).all()), 'exactly the reported slab rows are written'
    tot = slab[:r].double().sum(dim=0).cpu()
    for got, ref, what in ((tot[:1728].view(27, 8, 8), wo.grad.double(), 'kernel gradient'), (tot[1728:], bo.grad.reshape(-1).double(), 'bias gradient')):
        gmax = float(ref.abs().max())
        err = float((got - ref).abs().max())
        assert err <= 1e-4 * gmax, '%s: err %.3e, own max %.3e' % (what, err, gmax)
    got = _from_bits(gin[1:]).cpu().double()
    ref = xo.grad.double()
    assert bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 1e-4 * float(ref.abs().max())                   # one bf16 rounding of a sum computed in another order
    assert bool((err <= tol).all()), 'input gradient: max err %.3e' % float(err.max())
    # run-to-run reproducible (fixed fold order)
    slab2 = torch.zeros_like(slab)
    gin2 = torch.zeros_like(gin)
    env['lib'].check(L.linr_spconv_bwd_fused_bf16(go[1:].data_ptr(), x[1:].data_ptr(), e['lo'].data_ptr(), e['mask'].data_ptr(),
                                                  e['ld'], n, w.data_ptr(), gin2[1:].data_ptr(), slab2.data_ptr(), nblocks,
                                                  ctypes.byref(rows), _stream()), 'linr_spconv_bwd_fused_bf16')
    assert torch.equal(slab[:r], slab2[:r]) and torch.equal(gin[1:], gin2[1:])


def test_weight_gradients_of_the_16x16x32_path_are_exact_sums_up_to_fp32_summation_order(env):
    """the kernel / bias gradients of the fused bf16 backward moved to v_mfma_f32_16x16x32_bf16 in round 5 (K = 32
    rows per instruction: another fp32 summation order than the 4x4x4 form before it).  On bf16-representable inputs every product
    in[i][ci] * gout[j][co] is EXACT in fp32, so the only error a correct kernel can make is the rounding of its fp32 partial sums:
    anchored in float64, |error| <= 1e-5 of the tensor's own largest entry on a 39 k-row kernel map (sphere8's finest scale: ~150
    tiles per wave chain, 256 slab rows) - a kernel that dropped, duplicated or mis-paired rows would be off by 1e-3 or more."""
    from linr_pcgc_amd import ops, synthetic
    from linr_pcgc_amd.module_utils import prepare_frame
    dev, L = env['dev'], env['L']
    fr = prepare_frame(synthetic.sphere_shell(8, 100), None, 64, device=dev)
    coord = fr['all_input_info'][0]['coord']
    n = int(coord.shape[0])
    nbr = ops.kmap_build(coord)
    lo, mask = ops.kmap_compress(nbr)
    gen = torch.Generator().manual_seed(616)
    x_h = obf.rb(torch.randn(n, 8, generator=gen))
    go_h = obf.rb(torch.randn(n, 8, generator=gen) * (torch.rand(n, 1, generator=gen) < 0.7))      # some all-zero gradient rows
    w = (torch.randn(27, 8, 8, generator=gen) * 0.2).to(dev).contiguous()
    go = torch.zeros((n + 1, 8), dtype=torch.int16, device=dev)
    go[1:] = _bf16_bits(go_h).to(dev)
    x = torch.zeros((n + 1, 8), dtype=torch.int16, device=dev)
    x[1:] = _bf16_bits(x_h).to(dev)
    gin = torch.zeros((n + 1, 8), dtype=torch.int16, device=dev)
    for nblocks in (256, 32):
        slab = torch.full((nblocks, 1736), float('nan'), device=dev)
        rows = ctypes.c_int32(0)
        env['lib'].check(L.linr_spconv_bwd_fused_bf16(go[1:].data_ptr(), x[1:].data_ptr(), lo.data_ptr(), mask.data_ptr(), nbr.shape[1], n,
                                                      w.data_ptr(), gin[1:].data_ptr(), slab.data_ptr(), nblocks, ctypes.byref(rows), _stream()),
                         'linr_spconv_bwd_fused_bf16')
        torch.cuda.synchronize()
        tot = slab[:rows.value].double().sum(dim=0)
        xd, gd = x_h.to(dev).double(), go_h.to(dev).double()
        ref_w = torch.zeros(27, 8, 8, dtype=torch.float64, device=dev)
        for k in range(27):                              # out[j] = sum_k in[nbr(j, k)] W[k]  =>  gW[k] = sum_j in[nbr(j, k)]^T gout[j]
            idx = nbr[k, :n].long()
            ok = idx >= 0
            ref_w[k] = xd[idx[ok]].t() @ gd[ok]
        ref_b = gd.sum(dim=0)
        for got, ref, what in ((tot[:1728].view(27, 8, 8), ref_w, 'kernel gradient'), (tot[1728:], ref_b, 'bias gradient')):
            gmax = float(ref.abs().max())
            err = float((got - ref).abs().max())
            assert err <= 1e-5 * gmax, '%s with %d slab rows: err %.3e, own max %.3e (ratio %.2e)' % (what, nblocks, err, gmax, err / gmax)


def _moved_model(pkg, shell, steps):
    """a model `steps` fp32 Adam steps away from its initialisation (GPU) and its state dict (CPU)"""
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    model, _ = _model_and_oracle(pkg, 5)
    frame = model.make_frame(shell['scales'])
    opt = FlatAdam(model)
    for _ in range(steps):
        train_step(model, opt, frame, shell['point_num'])
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return model, sd, frame


@pytest.mark.parametrize('steps', [0, 10])
def test_bf16_train_forward_matches_the_emulating_oracle(pkg, shell, steps):
    from linr_pcgc_amd import engine
    model, sd, frame = _moved_model(pkg, shell, steps)
    probs = torch.empty((8, frame.rows), dtype=torch.float32, device='cuda')
    bits = torch.zeros(1, dtype=torch.float64, device='cuda')
    engine.net_forward_train_bf16(frame, model.flat_parameters(), probs, bits)
    probs2 = torch.empty_like(probs)
    bits2 = torch.zeros_like(bits)
    engine.net_forward_train_bf16(frame, model.flat_parameters(), probs2, bits2)
    assert torch.equal(probs, probs2) and torch.equal(bits, bits2)
    tsc = onet.to_torch_scales(shell['scales'])
    ref_bits, ref32_bits, worst = 0.0, 0.0, 0.0
    with torch.no_grad():
        for i, s in enumerate(tsc):
            o = obf.train_forward_scale(sd, s)
            o32 = onet.forward_scale(sd, s)
            ref_bits += float(o['bits'])
            ref32_bits += float(o32['bits'])
            sl = frame.scale_slice(i)
            for k in range(8):
                d = (_logits(probs[k, sl].cpu()) - o['logits'][k].reshape(-1).double()).abs()
                worst = max(worst, float(d.max()))
                d32 = (_logits(probs[k, sl].cpu()) - o32['logits'][k].reshape(-1).double()).abs()
                assert float(d32.max()) <= 1e-1, 'scale %d stage %d: logits %.3e from the fp32 oracle' % (i, k, float(d32.max()))
    assert worst <= 2e-2, 'logits: %.3e from the emulating oracle' % worst
    assert abs(float(bits) - ref_bits) <= 1e-3 * ref_bits, (float(bits), ref_bits)
    assert abs(float(bits) - ref32_bits) <= 1e-2 * ref32_bits, (float(bits), ref32_bits)


def test_first_convolutions_as_one_matrix_product_match_the_4x4x4_kernel(pkg, shell, monkeypatch):
    """bocc7m_k (v_mfma_f32_16x16x32_bf16: the seven first convolutions of the outter blocks as ONE matrix product, models/upsample.py:
    206-214) against bocc7_k (4x4x4 blocks, lane = row): the inputs are 0 / 1 and the kernels bf16, so every product is exact and the two
    differ by fp32 summation order only - a handful of activations round to the neighbouring bf16 value, which moves logits by a
    few 1e-3 at most and the frame's bits by < 1e-5."""
    from linr_pcgc_amd import engine
    model, sd, frame = _moved_model(pkg, shell, 10)
    out = {}
    for mode in ('0', '1'):
        monkeypatch.setenv('LINR_BOCC7_MFMA16', mode)
        probs = torch.empty((8, frame.rows), dtype=torch.float32, device='cuda')
        bits = torch.zeros(1, dtype=torch.float64, device='cuda')
        engine.net_forward_train_bf16(frame, model.flat_parameters(), probs, bits)
        out[mode] = (probs, float(bits))
    monkeypatch.delenv('LINR_BOCC7_MFMA16')
    d = (_logits(out['0'][0].cpu()) - _logits(out['1'][0].cpu())).abs()
    assert float(d.max()) <= 1e-2, float(d.max())
    assert float((d > 1e-4).double().mean()) <= 0.05, float((d > 1e-4).double().mean())
    assert abs(out['0'][1] - out['1'][1]) <= 1e-4 * out['0'][1], (out['0'][1], out['1'][1])
    assert bool(torch.equal(out['0'][0][0], out['1'][0][0])), 'stage 0 does not read the occupancy convolutions'


@pytest.mark.parametrize('steps', [0, 10])
def test_bf16_train_gradients_match_the_emulating_oracle(pkg, shell, steps):
    """every one of the 189 gradient tensors within 2e-2 of its own largest entry of the emulating oracle's autograd gradient,
    cosine >= 0.999 with the fp32 oracle's gradient over the whole vector (>= 0.99 per tensor)"""
    from linr_pcgc_amd import engine
    model, sd, frame = _moved_model(pkg, shell, steps)
    gscale = 1.0 / shell['point_num']
    grads = torch.zeros_like(model.flat_parameters())
    engine.net_forward_train_bf16(frame, model.flat_parameters(), None, None)
    engine.net_backward_bf16(frame, model.flat_parameters(), grads, gscale)
    grads2 = torch.zeros_like(grads)
    engine.net_backward_bf16(frame, model.flat_parameters(), grads2, gscale)
    assert torch.equal(grads, grads2), 'the backward pass must be reproducible'
    assert bool(torch.isfinite(grads).all())
    tsc = onet.to_torch_scales(shell['scales'])
    sdo = {k: v.clone().requires_grad_() for k, v in sd.items()}
    (obf.train_frame_bits(sdo, tsc) * gscale).backward()
    sd32 = {k: v.clone().requires_grad_() for k, v in sd.items()}
    (onet.frame_bits(sd32, tsc) * gscale).backward()
    off, report = 0, []
    g = grads.cpu().double()
    for name, v in sdo.items():
        n = v.numel()
        mine = g[off:off + n].view(v.shape)
        ref = v.grad.double()
        r32 = sd32[name].grad.double()
        gmax = float(ref.abs().max())
        err = float((mine - ref).abs().max())
        cos = float((mine * r32).sum() / (mine.norm() * r32.norm()).clamp_min(1e-300))
        report.append((err / max(gmax, 1e-300), cos, name))
        off += n
    bad = [(e, c, nm) for e, c, nm in report if e > 2e-2]
    assert not bad, 'gradient tensors off by more than 2e-2 of their own max: %s' % bad[:8]
    flat32 = torch.cat([sd32[k].grad.reshape(-1) for k in sd32]).double()
    cos_all = float((g * flat32).sum() / (g.norm() * flat32.norm()))
    assert cos_all >= 0.999, cos_all
    low = [(c, nm) for e, c, nm in report if c < 0.99]
    assert not low, 'per-tensor cosine with the fp32 gradient below 0.99: %s' % low[:8]


def test_bf16_train_step_tracks_adam_on_the_emulating_oracle(pkg, shell):
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    model, sd = _model_and_oracle(pkg, 5)
    model.train_precision = 'bf16'
    frame = model.make_frame(shell['scales'])
    opt = FlatAdam(model)
    sdo = {k: v.clone().requires_grad_() for k, v in sd.items()}
    opt_o = torch.optim.Adam(list(sdo.values()), lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    tsc = onet.to_torch_scales(shell['scales'])
    for it in range(4):
        bits = train_step(model, opt, frame, shell['point_num'])
        lo = obf.train_frame_bits(sdo, tsc)
        (lo / shell['point_num']).backward()
        opt_o.step()
        opt_o.zero_grad()
        assert abs(float(bits) - float(lo)) <= 2e-3 * float(lo), (it, float(bits), float(lo))
    flat_o = torch.cat([v.detach().reshape(-1) for v in sdo.values()])
    # Adam's first steps move every parameter by ~lr whatever the gradient's size, so a gradient entry whose sign is within the
    # rounding noise can differ by 2 lr per step: the bound is on the bulk, the worst entries are bounded by the steps taken
    d = (model.flat_parameters().cpu() - flat_o).abs()
    assert float(d.max()) <= 4 * 2 * 0.01 + 1e-6
    assert float(d.mean()) <= 2e-3, float(d.mean())


def test_bf16_overfit_is_deterministic_and_lowers_the_bits(pkg, shell):
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    outs = []
    for _ in range(2):
        model, _ = _model_and_oracle(pkg, 5)
        model.train_precision = 'bf16'
        frame = model.make_frame(shell['scales'])
        opt = FlatAdam(model)
        bits = [float(train_step(model, opt, frame, shell['point_num'])) for _ in range(12)]
        outs.append((bits, model.flat_parameters().clone()))
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][0][-1] < 0.8 * outs[0][0][0], outs[0][0]


def test_bf16_training_rejects_what_it_does_not_support(pkg, shell):
    from linr_pcgc_amd import _lib, overfit
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    model = overfit.gen_model(5, 'cuda', seed=1, block_layers=2)
    model.train_precision = 'bf16'
    frame = model.make_frame(shell['scales'])
    with pytest.raises(_lib.LinrError):
        train_step(model, FlatAdam(model), frame, shell['point_num'])
    with pytest.raises(_lib.LinrError):          # the library takes the frame's depth: without deep=True Python refuses it
        frame.train_bf16_arena()


def test_bf16_training_does_not_depend_on_leftover_state(pkg):
    """Neither on what the arena held before (it comes uninitialised: here filled with 0xFF bytes = NaN patterns) nor on the LDS /
    register contents another kernel left on the CUs (linr_debug_poison in front of every launch): three full-size training steps
    give bit-identical parameters, moments and bits."""
    from linr_pcgc_amd import _lib, overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    L = _lib.lib()
    cloud = synthetic.sequence_frame_device('loot10', 0, 'cuda')

    def run(dirty):
        gop = overfit.Gop(None, [cloud], None, 64, 'cuda')
        f = gop.frames[0]
        if dirty:
            nbytes = L.linr_net_train_bf16_arena_bytes(f.rows, 1)
            f.arena_train_bf16 = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device='cuda')
        m = overfit.gen_model(gop.scale_num, 'cuda', seed=8807)
        m.train_precision = 'bf16'
        o = FlatAdam(m)
        bits = torch.zeros(3, dtype=torch.float64, device='cuda')
        L.linr_debug_poison(0xFFFFFF if dirty else 0)
        try:
            for s in range(3):
                train_step(m, o, f, gop.point_nums[0], out=bits[s:s + 1])
            torch.cuda.synchronize()
        finally:
            L.linr_debug_poison(0xFFFFFF if os.environ.get('LINR_DEBUG_POISON') else 0)
        return m.flat_parameters().clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), bits.cpu()
    clean, dirty = run(False), run(True)
    assert bool(torch.isfinite(dirty[0]).all()) and bool(torch.isfinite(dirty[3]).all())
    assert float(dirty[3][2]) < float(dirty[3][0]), dirty[3]
    for a, b in zip(clean, dirty):
        assert torch.equal(a, b)


@pytest.mark.parametrize('n', [1, 2, 63, 65, 257])
def test_bf16_training_tiny_and_ragged_frames(n):
    """Edge cases: a single voxel, row counts around the 64-row tiles, a zero-row scale beside them: bits and every gradient tensor
    against the emulating oracle (2e-2 of the tensor's own largest entry; clouds whose smallest ReLU input is within rounding
    of zero are redrawn: a ReLU tie is not an error)."""
    from linr_pcgc_amd import engine, overfit
    for attempt in range(8):
        rng = np.random.default_rng(1000 * n + attempt)
        c = ooct.unique_sorted(rng.integers(0, 7, size=(4 * n, 3)))[:n]
        m = len(c)
        scales = [{'coord': c, 'occ': (rng.random((m, 8)) < 0.5).astype(np.float32), 'offset_tensor': ooct.offset_tensor(c), 'scale_idx': 1},
                  {'coord': np.zeros((0, 3), np.int32), 'occ': np.zeros((0, 8), np.float32), 'offset_tensor': np.zeros((0, 7), np.float32),
                   'scale_idx': 0}]
        model = overfit.gen_model(3, 'cuda', seed=5 + attempt)
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        sc = dict(scales[0])
        sc['nbr'] = ooct.neighbour_table(c)
        tsc = onet.to_torch_scales([sc])
        sdo = {k: v.clone().requires_grad_() for k, v in sd.items()}
        ref_bits = obf.train_frame_bits(sdo, tsc)
        ref_bits.backward()
        frame = model.make_frame(scales)
        bits = torch.zeros(1, dtype=torch.float64, device='cuda')
        grads = torch.zeros_like(model.flat_parameters())
        engine.net_forward_train_bf16(frame, model.flat_parameters(), None, bits)
        engine.net_backward_bf16(frame, model.flat_parameters(), grads, 1.0)
        assert bool(torch.isfinite(grads).all())
        assert abs(float(bits) - float(ref_bits)) <= 2e-3 * float(ref_bits) + 1e-3, (float(bits), float(ref_bits))
        off, bad = 0, []
        g = grads.cpu().double()
        for name, v in sdo.items():
            k = v.numel()
            ref = (v.grad if v.grad is not None else torch.zeros_like(v)).double()
            err = float((g[off:off + k].view(v.shape) - ref).abs().max())
            if err > 2e-2 * float(ref.abs().max()) + 1e-9:
                bad.append((name, err, float(ref.abs().max())))
            off += k
        if not bad:
            return
    raise AssertionError('gradients off on every redraw: %s' % bad[:6])


def _overfit_pair(config, gop_frames, epochs, seeds):
    """complete overfits of one GOP with the fp32 and the bf16 training executor from the same initialisations; real streams
    through the bf16 / uint8-weight codec, the first frame decoded"""
    from linr_pcgc_amd import codec, overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam
    clouds = [synthetic.sequence_frame_device(config, t, 'cuda') for t in range(gop_frames)]
    gop = overfit.Gop(None, clouds, None, 64, 'cuda')
    out = {'f32': [], 'bf16': []}
    for seed in seeds:
        for prec in ('f32', 'bf16'):
            model = overfit.gen_model(gop.scale_num, 'cuda', seed=seed)
            model.train_precision = prec
            opt = FlatAdam(model)
            overfit.overfit_gop(model, opt, gop, epochs)
            enc = codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda'), gop, precision='bf16')
            dec = codec.decode_gop(overfit.gen_model(gop.scale_num, 'cuda'), enc, frames=[0])
            ref = torch.as_tensor(gop.infos[0]['ori']).cuda() + torch.tensor(gop.coord_mins[0], device='cuda', dtype=torch.int32)
            assert torch.equal(dec[0], ref), 'decode must be bit-exact (%s, seed %d)' % (prec, seed)
            out[prec].append(enc['bpp']['bpp_all'])
    return out


def _assert_same_rate(r, what):
    """What the FULL-RECIPE tests assert: the reference's recipe (lr 0.01, 10 epochs, best-epoch checkpoint,
    8-bit weight codec) is chaotic in the rounding - one executor's seeds spread by +-3-6 % and an occasional run lands 12-25 % high
    when the 8-bit weight quantiser meets an outlier weight (profiles/r06_bf16_overfit_seeds.txt: 8 seeds of each executor) - so no
    3-seed statistic can carry SURVEY section 8c's +1 %.  That bound is asserted where it can be, per epoch and per seed, by
    test_bf16_tracks_fp32_outside_the_chaotic_regime below.  Here: a SANITY CAP - the MEDIAN bits/point over the seeds (robust
    against one outlier run of either executor) of bf16 training within +5 % of fp32 training; the measured ratios are printed."""
    med = lambda v: sorted(v)[len(v) // 2]
    n = len(r['f32'])
    m32, mbf = sum(r['f32']) / n, sum(r['bf16']) / n
    print('%s: bits/point fp32 %s  bf16 %s  ratio of means %.4f  ratio of medians %.4f'
          % (what, ['%.4f' % x for x in r['f32']], ['%.4f' % x for x in r['bf16']], mbf / m32, med(r['bf16']) / med(r['f32'])))
    assert med(r['bf16']) <= 1.05 * med(r['f32']), (r, med(r['f32']), med(r['bf16']))


def test_bf16_overfit_of_loot10_reaches_the_fp32_rate():
    """BASELINE config[1]'s GOP (32 frames of the loot stand-in, 10 epochs, the reference's recipe) trained with the bf16 executor over
    five initialisation seeds against the fp32 executor's: _assert_same_rate's +5 % cap on the medians (NOT the +1 % of SURVEY 8c:
    see there), every run lossless through the bf16 / uint8-weight codec."""
    _assert_same_rate(_overfit_pair('loot10', 32, 10, (8807, 1, 2, 3, 4)), 'loot10 GOP 32')


def test_bf16_overfit_of_owlii11_reaches_the_fp32_rate():
    """BASELINE config[4]'s geometry (Owlii stand-in: 11-bit, ~2.9 M points, 8 scales, ~1.24 M rows per frame), a 16-frame GOP, 10
    epochs, three seeds: the same +5 % cap on the medians (the 64-frame GOP of the config: bench.py's config4_gop64, lossless in both
    precisions from one seed)."""
    _assert_same_rate(_overfit_pair('owlii11', 16, 10, (8807, 1, 2)), 'owlii11 GOP 16')


@pytest.mark.parametrize('config,gop_frames', [('loot10', 32), ('owlii11', 16)])
def test_bf16_tracks_fp32_outside_the_chaotic_regime(config, gop_frames):
    """VERDICT r5 item 1(i) - the test that carries SURVEY section 8c's bf16 tolerance (+-1 %).  Same initialisations (seeds 8807, 1, 2),
    CONSTANT learning rate 1e-3 (a tenth of the recipe's: small steps keep the two trajectories together, so a biased kernel shows
    and rounding chaos does not), 3 epochs over the GOP, both executors: EVERY epoch's mean loss (bits per point of the training
    forward, main.py:305-321) of EVERY seed within +-1 % of the fp32 executor's - no averaging over seeds, no standard-error term."""
    from linr_pcgc_amd import overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam
    clouds = [synthetic.sequence_frame_device(config, t, 'cuda') for t in range(gop_frames)]
    gop = overfit.Gop(None, clouds, None, 64, 'cuda')
    worst = 0.0
    for seed in (8807, 1, 2):
        losses = {}
        for prec in ('f32', 'bf16'):
            model = overfit.gen_model(gop.scale_num, 'cuda', seed=seed)
            model.train_precision = prec
            opt = FlatAdam(model, lr=1e-3, gamma=1.0)
            losses[prec] = overfit.overfit_gop(model, opt, gop, 3, min_lr=0.0, keep='last')
        ratios = [b / f for b, f in zip(losses['bf16'], losses['f32'])]
        print('%s seed %d: fp32 %s  bf16 %s  ratios %s' % (config, seed, ['%.4f' % x for x in losses['f32']],
                                                           ['%.4f' % x for x in losses['bf16']], ['%.4f' % x for x in ratios]))
        assert losses['f32'][-1] < losses['f32'][0] and losses['bf16'][-1] < losses['bf16'][0], 'both executors must be learning'
        for e, q in enumerate(ratios):
            worst = max(worst, abs(q - 1.0))
            assert abs(q - 1.0) <= 0.01, 'seed %d epoch %d: bf16 / fp32 = %.4f (%s)' % (seed, e, q, losses)
    print('%s: worst |bf16 / fp32 - 1| over 3 seeds x 3 epochs = %.4f' % (config, worst))


def test_checkpoints_cross_the_two_training_executors(pkg, shell):
    """Both executors train the same fp32 master parameters with the same optimiser state (main.py:241-248: GOPs >= 1 warm-start from
    GOP 0's model AND optimiser): a GOP trained in bf16 hands over to one trained in fp32 and back, the loss keeps falling."""
    from linr_pcgc_amd import overfit
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    model = overfit.gen_model(5, 'cuda', seed=8807)
    model.train_precision = 'bf16'
    frame = model.make_frame(shell['scales'])
    opt = FlatAdam(model)
    first = [float(train_step(model, opt, frame, shell['point_num'])) for _ in range(8)]
    ck = overfit.checkpoint(model, opt, 0, first[-1])
    m2 = overfit.gen_model(5, 'cuda', seed=1)
    o2 = FlatAdam(m2)
    overfit.warm_start(m2, o2, ck)
    assert o2.t == opt.t and torch.equal(m2.flat_parameters(), model.flat_parameters())
    second = [float(train_step(m2, o2, m2.make_frame(shell['scales']), shell['point_num'])) for _ in range(8)]      # fp32 from here
    m2.train_precision = 'bf16'
    third = [float(train_step(m2, o2, m2.make_frame(shell['scales']), shell['point_num'])) for _ in range(8)]       # and back
    assert second[0] < first[0] and second[-1] < first[-1] and third[-1] < second[-1], (first, second, third)
    # the fp32 step right behind the hand-over sees (to bf16 rounding) the loss the bf16 executor would have seen next
    nxt = float(train_step(model, opt, frame, shell['point_num']))
    assert abs(second[0] - nxt) <= 5e-3 * nxt, (second[0], nxt)


def test_bf16_step_keeps_the_per_scale_adam_semantics(pkg, shell):
    _bf16_step_keeps_the_per_scale_adam_semantics(pkg, shell, ADAM_DEFAULT, 1.0)


def test_fused_bf16_step_passes_distinct_adam_arguments(pkg, shell):
    _bf16_step_keeps_the_per_scale_adam_semantics(pkg, shell, ADAM_DISTINCT, ADAM_DISTINCT_GSCALE_DIV)


def _bf16_step_keeps_the_per_scale_adam_semantics(pkg, shell, adam, gscale_div):
    """The context MLP of a scale no frame has contained yet is left alone (torch.optim.Adam skips .grad None; torch 1.13.1,
    enviroment.yaml:30), afterwards it is updated on every step, zero gradient or not (main.py:320): the bf16 step shares the fp32
    step's reduction and Adam.  Frames: 4 scales, 4 scales, 5 scales, 4 scales - the coarsest scale's MLP starts at step 3; the fused
    bf16 step against its own unfused entries (forward, backward, FlatAdam.step) bit for bit.  adam / gscale_div: the optimiser's
    arguments and the loss scale 1 / (gscale_div * point_num) of both paths (gpu_common.ADAM_DISTINCT)."""
    from linr_pcgc_amd import engine
    from linr_pcgc_amd.model_core import FlatAdam, LINR_PCGC_Model, train_step
    model, sd = _model_and_oracle(pkg, 5)
    model.train_precision = 'bf16'
    full = shell['scales']
    frames = [model.make_frame(full[:-1]), model.make_frame(full[:-1]), model.make_frame(full), model.make_frame(full[:-1])]
    opt = FlatAdam(model, **adam)
    point_num = gscale_div * shell['point_num']
    model2 = LINR_PCGC_Model({'scale_num': 5, 'in_channel': 7, 'hidden_channel_conv': 8, 'block_layers': 1, 'outstage': 8, 'instage': 1}).cuda()
    model2.load_state_dict(sd)
    opt2 = FlatAdam(model2, **adam)
    frames2 = [model2.make_frame(full[:-1]), model2.make_frame(full[:-1]), model2.make_frame(full), model2.make_frame(full[:-1])]
    w4 = lambda m: dict(m.named_parameters())['scale_mlp.4.0.weight'].detach().clone()
    w4_init = w4(model)
    for it in range(6):
        j = it % 4
        bits_fused = train_step(model, opt, frames[j], point_num)
        bits = torch.zeros(1, dtype=torch.float64, device='cuda')
        engine.net_forward_train_bf16(frames2[j], model2.flat_parameters(), None, bits)
        assert float(bits_fused) == float(bits), 'bits of the fused bf16 step differ from linr_net_forward_train_bf16 at step %d' % it
        opt2.zero_grad()
        engine.net_backward_bf16(frames2[j], model2.flat_parameters(), opt2.grad, 1.0 / point_num)
        opt2.step(frames2[j])
        if it < 2:
            assert torch.equal(w4(model), w4_init), 'scale 4 has had no gradient yet: its MLP must be untouched'
    assert not torch.equal(w4(model), w4_init)
    assert opt.t == 6 and opt.t_scale.tolist() == [6, 6, 6, 6, 4] and opt2.t_scale.tolist() == [6, 6, 6, 6, 4]
    assert torch.equal(model.flat_parameters(), model2.flat_parameters()), 'fused bf16 train_step and forward + backward + FlatAdam.step differ'
    assert torch.equal(opt.exp_avg, opt2.exp_avg) and torch.equal(opt.exp_avg_sq, opt2.exp_avg_sq)
