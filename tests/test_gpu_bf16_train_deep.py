"""GPU tests of the bf16 training executor at block_layers 2..4 of block_in (--block_layers, main.py:521; models/resnet.py:146-162): the
entries of csrc/train_bf16.hip (linr_net_forward_train_bf16, linr_net_backward_bf16, linr_net_train_step_bf16) on deeper frames,
which Python opens with deep=True and train_precision 'bf16-deep'.

The reference trains in fp32 only, so - as for tests/test_gpu_bf16_train.py, whose bounds for each pair are used unchanged:
  * against the emulating reference (tests/bf16_train_deep_ref.py: oracle/network_bf16.py's pieces chained over nl layers, the extra skip
    as ONE stored matrix; pinned on the CPU by tests/test_bf16_train_deep_ref.py): logits |d| <= 2e-2, bits rel <= 1e-3, every gradient
    tensor within 2e-2 of ITS OWN largest entry;
  * against the fp32 oracle (oracle/network.py): the gradient vector at cosine >= 0.999, every tensor >= 0.99;
  * run-to-run bit-identical.
Test inputs: the model at initialisation (seeded) and at initialisation plus seeded CPU noise of 0.5 x each tensor's own standard
deviation.  No training kernel produces a test input.
Sizes: the golden shell (6,821 rows: every backward launch at one tile per wave), frames of 1 to 257 rows beside a zero-row scale, and
the "middle" frame of tests/test_gpu_bf16_train_tiles.py (32,900 rows on 256 CUs), where the single-group launches of block_in's chain
and the grouped ones walk several tiles per wave - its helpers and criteria are imported, not restated.
Measured on the MI355X (256 CUs).  Golden shell, block_layers 2 / 3 / 4, initialisation and noise: logits within 2.7e-3 .. 6.5e-3, bits rel
<= 6.0e-7, worst gradient tensor at 2.9e-3 .. 5.2e-3 of its largest entry - but 1.90e-2 at block_layers 2 / initialisation, an outter
block's conv1_0.bias (all biases are zero there: ReLU inputs at rounding distance of zero) - cosine with fp32 >= 0.99996 overall,
lowest tensor 0.9921.  Middle frame, block_layers 3: worst err_T / max|T| 2.2e-7 against the fp32 executor's own 1.9e-7, worst err_T at
0.0115 of its bound, largest bound of a 3x3x3 kernel tensor 2.3e-4 of its largest entry; against the emulating reference logits 9.7e-3,
bits rel 1.9e-7, worst gradient tensor 1.5e-2.  End to end: fp32 3.3912 / 3.1876 / 2.9102, bf16-deep 3.3912 / 3.1876 / 2.9103 bits per
point (worst ratio 1.00003).  22 s for the file, 8 s of them the reference's passes over the middle frame.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bf16_train_deep_ref as dref                    # noqa: E402
import test_gpu_bf16_train_tiles as tiles             # noqa: E402
from oracle import network as onet                    # noqa: E402
from oracle import octree as ooct                     # noqa: E402


def _logits(p):
    p = p.double()
    return torch.log(p) - torch.log1p(-p)


def _model(pkg, scale_num, block_layers, seed=8807, noise=False):
    """The model at its (seeded) initialisation, or that plus N(0, (0.5 std_T)^2) drawn on the CPU per tensor T; its state dict (CPU)."""
    from gpu_common import _model_and_oracle
    model, sd = _model_and_oracle(pkg, scale_num, seed=seed, block_layers=block_layers)
    if noise:
        g = torch.Generator().manual_seed(seed + 31 * block_layers)
        moved = {}
        for k, v in sd.items():
            std = float(v.std()) if v.numel() > 1 else 0.0
            moved[k] = v + 0.5 * std * torch.randn(v.shape, generator=g)
        model.load_state_dict(moved)
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    assert model.block_layers == block_layers
    return model, sd


# ---- 1: golden shell ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('noise', [False, True], ids=['init', 'noise'])
@pytest.mark.parametrize('block_layers', [2, 3, 4])
def test_deep_forward_and_gradients_match_the_emulating_reference(pkg, shell, block_layers, noise):
    """Golden shell, block_layers 2 / 3 / 4: forward logits within 2e-2 and bits within 1e-3 relative of the emulating reference, every
    gradient tensor within 2e-2 of its own largest entry, cosine with the fp32 oracle's gradient >= 0.999 overall and >= 0.99 per
    tensor, two runs bit-identical (forward and backward)."""
    from linr_pcgc_amd import engine
    model, sd = _model(pkg, 5, block_layers, noise=noise)
    frame = model.make_frame(shell['scales'])
    flat = model.flat_parameters()
    gscale = 1.0 / shell['point_num']
    runs = []
    for _ in range(2):
        probs = torch.full((8, frame.rows), float('nan'), device='cuda')
        bits = torch.zeros(1, dtype=torch.float64, device='cuda')
        grads = torch.zeros_like(flat)
        engine.net_forward_train_bf16(frame, flat, probs, bits, deep=True)
        engine.net_backward_bf16(frame, flat, grads, gscale, deep=True)
        runs.append((probs, bits, grads))
    (probs, bits, grads), (probs2, bits2, grads2) = runs
    assert torch.equal(probs, probs2) and torch.equal(bits, bits2) and torch.equal(grads, grads2), 'two runs must be bit-identical'
    assert bool(torch.isfinite(probs).all()) and bool(torch.isfinite(grads).all())
    tsc = onet.to_torch_scales(shell['scales'])
    sdo = {k: v.clone().requires_grad_() for k, v in sd.items()}
    ref_bits, worst = 0.0, 0.0
    total = 0
    for i, s in enumerate(tsc):
        o = dref.train_forward_scale(sdo, s)
        ref_bits += float(o['bits'])
        total = total + o['bits']
        sl = frame.scale_slice(i)
        for k in range(8):
            d = (_logits(probs[k, sl].cpu()) - o['logits'][k].detach().reshape(-1).double()).abs()
            worst = max(worst, float(d.max()))
    (total * gscale).backward()
    sd32 = {k: v.clone().requires_grad_() for k, v in sd.items()}
    (onet.frame_bits(sd32, tsc) * gscale).backward()
    rel_bits = abs(float(bits) - ref_bits) / ref_bits
    off, report = 0, []
    g = grads.cpu().double()
    for name, v in sdo.items():
        n = v.numel()
        mine = g[off:off + n].view(v.shape)
        ref = (v.grad if v.grad is not None else torch.zeros_like(v)).double()
        r32 = (sd32[name].grad if sd32[name].grad is not None else torch.zeros_like(v)).double()
        gmax = float(ref.abs().max())
        err = float((mine - ref).abs().max())
        cos = float((mine * r32).sum() / (mine.norm() * r32.norm()).clamp_min(1e-300)) if float(r32.norm()) > 0 else 1.0
        report.append((err / max(gmax, 1e-300) if gmax > 0 else (0.0 if err == 0 else float('inf')), cos, name))
        off += n
    assert off == g.numel()
    flat32 = torch.cat([(sd32[k].grad if sd32[k].grad is not None else torch.zeros_like(sd32[k])).reshape(-1) for k in sd32]).double()
    cos_all = float((g * flat32).sum() / (g.norm() * flat32.norm()))
    w_err, w_cos = max(report), min((c, nm) for _, c, nm in report)
    print('block_layers %d, %s: logits %.3e, bits rel %.2e, worst gradient tensor at %.3e of its largest entry (%s), cosine with fp32 %.6f '
          'overall, lowest tensor %.5f (%s)' % (block_layers, 'noise' if noise else 'init', worst, rel_bits, w_err[0], w_err[2], cos_all,
                                                w_cos[0], w_cos[1]))
    assert worst <= 2e-2, 'logits: %.3e from the emulating reference' % worst
    assert rel_bits <= 1e-3, (float(bits), ref_bits)
    bad = [(e, c, nm) for e, c, nm in report if e > 2e-2]
    assert not bad, 'gradient tensors off by more than 2e-2 of their own max: %s' % bad[:8]
    assert cos_all >= 0.999, cos_all
    low = [(c, nm) for e, c, nm in report if c < 0.99]
    assert not low, 'per-tensor cosine with the fp32 gradient below 0.99: %s' % low[:8]


# ---- 2: tiny and ragged frames --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_deep_training_tiny_and_ragged_frames(n):
    """block_layers 2 on a single voxel, on row counts around the 64-row tiles, beside a zero-row scale: bits and every gradient tensor
    against the emulating reference, with the redraw rule of test_bf16_training_tiny_and_ragged_frames (2e-2 of the tensor's own
    largest entry; a cloud whose gradients miss is redrawn, up to 8 times: a ReLU tie is not an error)."""
    from linr_pcgc_amd import engine, overfit
    for attempt in range(8):
        rng = np.random.default_rng(1000 * n + attempt)
        c = ooct.unique_sorted(rng.integers(0, 7, size=(4 * n, 3)))[:n]
        m = len(c)
        scales = [{'coord': c, 'occ': (rng.random((m, 8)) < 0.5).astype(np.float32), 'offset_tensor': ooct.offset_tensor(c), 'scale_idx': 1},
                  {'coord': np.zeros((0, 3), np.int32), 'occ': np.zeros((0, 8), np.float32), 'offset_tensor': np.zeros((0, 7), np.float32),
                   'scale_idx': 0}]
        model = overfit.gen_model(3, 'cuda', seed=5 + attempt, block_layers=2)
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        sc = dict(scales[0])
        sc['nbr'] = ooct.neighbour_table(c)
        tsc = onet.to_torch_scales([sc])
        sdo = {k: v.clone().requires_grad_() for k, v in sd.items()}
        ref_bits = dref.train_frame_bits(sdo, tsc)
        ref_bits.backward()
        frame = model.make_frame(scales)
        bits = torch.zeros(1, dtype=torch.float64, device='cuda')
        grads = torch.zeros_like(model.flat_parameters())
        engine.net_forward_train_bf16(frame, model.flat_parameters(), None, bits, deep=True)
        engine.net_backward_bf16(frame, model.flat_parameters(), grads, 1.0, deep=True)
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


# ---- 3: several tiles per wave --------------------------------------------------------------------------------------------------------
def _dirty_deep_arena(frame):
    from linr_pcgc_amd import _lib
    nbytes = _lib.lib().linr_net_train_bf16_arena_bytes(frame.rows, frame.block_layers)
    assert nbytes > 0
    frame.arena_train_bf16 = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device='cuda')


def _run_deep(frame, flat, gscale):
    """forward + backward of the deep entries from an arena of 0xFF bytes and poisoned CUs: probs [8, rows], bits, flat gradient"""
    from linr_pcgc_amd import engine
    _dirty_deep_arena(frame)
    probs = torch.full((8, frame.rows), float('nan'), device='cuda')
    bits = torch.zeros(1, dtype=torch.float64, device='cuda')
    grads = torch.zeros_like(flat)
    with tiles._Poison():
        engine.net_forward_train_bf16(frame, flat, probs, bits, deep=True)
        engine.net_backward_bf16(frame, flat, grads, gscale, deep=True)
    assert bool(torch.isfinite(probs).all()), '%d probabilities never written or not finite' % int((~torch.isfinite(probs)).sum())
    assert bool(torch.isfinite(grads).all()), '%d gradient entries not finite' % int((~torch.isfinite(grads)).sum())
    return probs, float(bits), grads


@pytest.fixture(scope='module')
def middle3(pkg):
    """tests/test_gpu_bf16_train_tiles.py's middle frame (its sizes, its pieces) at block_layers 3, the model at initialisation plus
    noise; the deep entries and the fp32 executor on the whole frame and on every piece alone.  Computed once."""
    cus = tiles._cus()
    tiles._schedule(1, cus)                                   # (skips when LINR_WG_BLOCKS is forced)
    total, S = 64 * tiles.BB_WAVES * min(2 * cus, 128) + 132, 3
    sizes = tiles._sizes(total, S)
    scales = []
    for i, n in enumerate(sizes):
        p = tiles._piece(n, 7000 + 100 * S + i)
        p['scale_idx'] = i
        scales.append(p)
    point_num = int(sum(float(s['occ'].sum()) for s in scales))
    model, sd = _model(pkg, S, 3, noise=True)
    frame = model.make_frame(scales)
    assert frame.rows == total and frame.block_layers == 3
    flat = model.flat_parameters()
    gscale = 1.0 / float(point_num)
    c = {'sizes': sizes, 'scales': scales, 'point_num': point_num, 'gscale': gscale, 'model': model, 'frame': frame, 'flat': flat,
         'names': [(k, v.numel(), tuple(v.shape)) for k, v in model.state_dict().items()], 'sd': sd}
    assert sum(n for _, n, _ in c['names']) == flat.numel()
    c['whole'] = _run_deep(frame, flat, gscale)
    c['whole32'] = tiles._run_f32(frame, flat, gscale)
    c['alone'], c['alone32'] = [], []
    for s in scales:
        f = model.make_frame([s])
        c['alone'].append(_run_deep(f, flat, gscale))
        c['alone32'].append(tiles._run_f32(f, flat, gscale))
        del f
    return c


def test_deep_middle_frame_walks_several_tiles_and_is_the_sum_of_its_scales(middle3):
    """32,900 rows (256 CUs) in 3 ragged scales at block_layers 3.  From the CU count as tests/test_gpu_bf16_train_tiles.py derives it: the
    single-group launches (block_in's chain: conv0_0 with the G2 epilogue, the dual launch, conv0_0 with the extra addend) walk
    tiles_per_wave[1] >= 2 tiles per wave, the grouped ones - the conv0_0 launch of the seven outter blocks runs on the grid of eight
    groups, so that its slab rows are the tail launch's - tiles_per_wave[8] >= 2, at 128 slab rows; every piece alone at one tile.
    That file's sum-of-parts criterion, its bound measured on the fp32 executor at the same depth: probabilities of a scale bit-equal
    to the scale alone, every gradient tensor of the whole frame within the re-association bound of the sum of the alone frames'.
    Arena pre-filled with 0xFF, linr_debug_poison on, everything finite."""
    c, cus = middle3, tiles._cus()
    s = tiles._schedule(c['frame'].rows, cus)
    assert s['tiles_per_wave'][1] >= 2 and s['tiles_per_wave'][8] >= 2 and s['nb'] == 128, s
    if cus == 256:
        assert c['frame'].rows == 32900 and s['tiles_per_wave'][1] == 2 and s['tiles_per_wave'][8] == 3, s
    assert all(tiles._one_tile(n, cus) for n in c['sizes']), (c['sizes'], cus)
    tiles._rows_do_not_depend_on_their_place(c, 'middle frame, block_layers 3')
    tiles._sum_of_parts(c, 'middle frame, block_layers 3', kernel_limit=1e-3)


def test_deep_middle_frame_matches_the_emulating_reference(middle3):
    """The same frame against the emulating reference run on the GPU in fp32 with TF32 off, one scale at a time: logits within 2e-2, bits
    1e-3 relative, every gradient tensor within 2e-2 of its own largest entry (whole frame against the sum over the scales)."""
    c = middle3
    leaves = {k: v.cuda().requires_grad_() for k, v in c['sd'].items()}
    names = list(leaves)
    ref_bits, ref_grad, worst_logit = 0.0, None, 0.0
    with tiles._NoTF32():
        for i, sc in enumerate(c['scales']):
            nbr = torch.from_numpy(ooct.neighbour_table(sc['coord'])).long().cuda()
            out = dref.train_forward_scale(leaves, {'offset_tensor': torch.from_numpy(sc['offset_tensor']).cuda(),
                                                    'occ': torch.from_numpy(sc['occ']).cuda(), 'nbr': nbr, 'scale_idx': i})
            sl = c['frame'].scale_slice(i)
            for k in range(8):
                z = out['logits'][k].detach().reshape(-1).double()
                worst_logit = max(worst_logit, float((_logits(c['whole'][0][k, sl]) - z).abs().max()))
            ref_bits += float(out['bits'].detach())
            g = torch.autograd.grad(out['bits'] * c['gscale'], [leaves[k] for k in names], allow_unused=True)
            g = torch.cat([(torch.zeros_like(leaves[k]) if t is None else t).reshape(-1) for k, t in zip(names, g)]).double()
            ref_grad = g if ref_grad is None else ref_grad + g
            del out, g
    rel_bits = abs(c['whole'][1] - ref_bits) / ref_bits
    worst, bad = (0.0, ''), []
    for (name, _, a), (_, _, b) in zip(tiles._tensors(c, c['whole'][2].double()), tiles._tensors(c, ref_grad)):
        gmax, err = float(b.abs().max()), float((a - b).abs().max())
        if err > 2e-2 * gmax:
            bad.append((name, err, gmax))
        if gmax > 0 and err / gmax > worst[0]:
            worst = (err / gmax, name)
    print('middle frame, block_layers 3, against the emulating reference: logits %.3e, bits rel %.2e, worst gradient tensor at %.3e of its '
          'largest entry (%s)' % (worst_logit, rel_bits, worst[0], worst[1]))
    assert worst_logit <= 2e-2, worst_logit
    assert rel_bits <= 1e-3, (c['whole'][1], ref_bits)
    assert not bad, 'gradient tensors off by more than 2e-2 of their own largest entry: %s' % bad[:6]


# ---- 4: the step ----------------------------------------------------------------------------------------------------------------------
def test_bf16_deep_at_block_layers_1_is_bf16_bit_for_bit(pkg, shell):
    """'bf16-deep' at block_layers 1 runs the launches of 'bf16': bits and parameters after three train_steps are torch.equal, and the
    arena has the size it had when 'bf16' had an arena of its own."""
    from linr_pcgc_amd import _lib
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    outs = {}
    for prec in ('bf16', 'bf16-deep'):
        model, _ = _model(pkg, 5, 1)
        model.train_precision = prec
        frame = model.make_frame(shell['scales'])
        opt = FlatAdam(model)
        bits = [train_step(model, opt, frame, shell['point_num']).clone() for _ in range(3)]
        outs[prec] = (torch.cat(bits), model.flat_parameters().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone())
    for a, b in zip(outs['bf16'], outs['bf16-deep']):
        assert torch.equal(a, b)
    assert _lib.lib().linr_net_train_bf16_arena_bytes(6821, 1) == 130606912


def test_bf16_deep_quantisation_aware_steps(pkg, shell):
    """Three steps at block_layers 2 with qat_bitdepth=8 (the step entry with qparams) run: finite, reproducible, and
    different from the plain steps - whose first bits they stay within 5 % of (the 8-bit image of the weights is close to them)."""
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    outs = {}
    for tag, depth in (('plain', 0), ('qat', 8), ('qat2', 8)):
        model, _ = _model(pkg, 5, 2)
        model.train_precision = 'bf16-deep'
        frame = model.make_frame(shell['scales'])
        opt = FlatAdam(model)
        bits = [float(train_step(model, opt, frame, shell['point_num'], qat_bitdepth=depth)) for _ in range(3)]
        outs[tag] = (bits, model.flat_parameters().clone())
    assert all(np.isfinite(outs['qat'][0])) and bool(torch.isfinite(outs['qat'][1]).all())
    assert outs['qat'][0] == outs['qat2'][0] and torch.equal(outs['qat'][1], outs['qat2'][1])
    assert outs['qat'][0] != outs['plain'][0] and not torch.equal(outs['qat'][1], outs['plain'][1])
    assert abs(outs['qat'][0][0] - outs['plain'][0][0]) <= 0.05 * outs['plain'][0][0], 'the 8-bit image of the weights is close to them'


@pytest.mark.parametrize('qat_bitdepth', [0, 8], ids=['plain', 'qat'])
def test_bf16_deep_fused_step_is_its_unfused_entries_bit_for_bit(pkg, shell, qat_bitdepth):
    """block_layers 2 through 'bf16-deep', Adam's arguments pairwise distinct and none at its default, a loss scale that is not
    1 / point_num (gpu_common.ADAM_DISTINCT): three fused steps (one linr_step_args) against the forward entry, the backward entry and
    FlatAdam.step (linr_adam_step, positional scalars) - with qat_bitdepth both at the fake-quantised image of the master.  Bits of
    every step, parameters and both moments torch.equal."""
    from gpu_common import ADAM_DISTINCT, ADAM_DISTINCT_GSCALE_DIV
    from linr_pcgc_amd import engine
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    point_num = ADAM_DISTINCT_GSCALE_DIV * shell['point_num']
    (model, _), (model2, _) = _model(pkg, 5, 2), _model(pkg, 5, 2)
    model.train_precision = 'bf16-deep'
    frame, frame2 = model.make_frame(shell['scales']), model2.make_frame(shell['scales'])
    opt, opt2 = FlatAdam(model, **ADAM_DISTINCT), FlatAdam(model2, **ADAM_DISTINCT)
    for it in range(3):
        bits_fused = train_step(model, opt, frame, point_num, qat_bitdepth=qat_bitdepth)
        at = model2.flat_parameters()
        if qat_bitdepth:
            at, _ = engine.params_fake_quant(at, qat_bitdepth)
        bits = torch.zeros(1, dtype=torch.float64, device='cuda')
        engine.net_forward_train_bf16(frame2, at, None, bits, deep=True)
        assert torch.equal(bits_fused, bits), 'bits of the fused step differ from the forward entry at step %d' % it
        opt2.zero_grad()
        engine.net_backward_bf16(frame2, at, opt2.grad, 1.0 / point_num, deep=True)
        opt2.step(frame2)
    assert opt.t == opt2.t == 3
    assert torch.equal(model.flat_parameters(), model2.flat_parameters()), 'fused step and forward + backward + FlatAdam.step differ'
    assert torch.equal(opt.exp_avg, opt2.exp_avg) and torch.equal(opt.exp_avg_sq, opt2.exp_avg_sq)


def test_bf16_deep_rejects_what_it_does_not_support(pkg, shell):
    from linr_pcgc_amd import _lib, overfit
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    model = overfit.gen_model(5, 'cuda', seed=1, hidden=16)
    model.train_precision = 'bf16-deep'
    frame = model.make_frame(shell['scales'])
    with pytest.raises(_lib.LinrError):
        train_step(model, FlatAdam(model), frame, shell['point_num'])


def test_bf16_deep_train_step_tracks_adam_on_the_emulating_reference(pkg, shell):
    """Four Adam steps at block_layers 2 against torch.optim.Adam on the emulating reference, with the bounds of
    test_bf16_train_step_tracks_adam_on_the_emulating_oracle."""
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    model, sd = _model(pkg, 5, 2)
    model.train_precision = 'bf16-deep'
    frame = model.make_frame(shell['scales'])
    opt = FlatAdam(model)
    sdo = {k: v.clone().requires_grad_() for k, v in sd.items()}
    opt_o = torch.optim.Adam(list(sdo.values()), lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    tsc = onet.to_torch_scales(shell['scales'])
    for it in range(4):
        bits = train_step(model, opt, frame, shell['point_num'])
        lo = dref.train_frame_bits(sdo, tsc)
        (lo / shell['point_num']).backward()
        opt_o.step()
        opt_o.zero_grad()
        assert abs(float(bits) - float(lo)) <= 2e-3 * float(lo), (it, float(bits), float(lo))
    flat_o = torch.cat([v.detach().reshape(-1) for v in sdo.values()])
    d = (model.flat_parameters().cpu() - flat_o).abs()
    assert float(d.max()) <= 4 * 2 * 0.01 + 1e-6
    assert float(d.mean()) <= 2e-3, float(d.mean())


# ---- 5: end to end --------------------------------------------------------------------------------------------------------------------
def test_bf16_deep_overfit_end_to_end():
    """4 frames of sphere8, block_layers 2, constant learning rate 1e-3, 3 epochs, seed 8807, the fp32 executor against 'bf16-deep':
    every epoch's mean loss within +-1 % of the fp32 executor's (the project's bf16 tolerance) and both fall; the
    bf16-trained model then codes the GOP through the bf16 / uint8-weight codec and frame 0 decodes bit-exactly; an fp32 train_step
    continues from its checkpoint with a falling loss."""
    from linr_pcgc_amd import codec, overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    clouds = [synthetic.sequence_frame_device('sphere8', t, 'cuda') for t in range(4)]
    gop = overfit.Gop(None, clouds, None, 64, 'cuda', block_layers=2)
    losses, kept = {}, {}
    for prec in ('f32', 'bf16-deep'):
        model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807, block_layers=2)
        model.train_precision = prec
        opt = FlatAdam(model, lr=1e-3, gamma=1.0)
        losses[prec] = overfit.overfit_gop(model, opt, gop, 3, min_lr=0.0, keep='last')
        kept[prec] = (model, opt)
    ratios = [b / f for b, f in zip(losses['bf16-deep'], losses['f32'])]
    print('sphere8 GOP 4, block_layers 2: fp32 %s  bf16-deep %s  ratios %s' % (['%.4f' % x for x in losses['f32']],
                                                                               ['%.4f' % x for x in losses['bf16-deep']],
                                                                               ['%.4f' % x for x in ratios]))
    assert losses['f32'][-1] < losses['f32'][0] and losses['bf16-deep'][-1] < losses['bf16-deep'][0], 'both executors must be learning'
    for e, q in enumerate(ratios):
        assert abs(q - 1.0) <= 0.01, 'epoch %d: bf16-deep / fp32 = %.4f (%s)' % (e, q, losses)
    model, opt = kept['bf16-deep']
    ck = overfit.checkpoint(model, opt, 2, losses['bf16-deep'][-1])
    enc = codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda', block_layers=2), gop, precision='bf16')
    assert enc['side_info']['train_precision'] == 'bf16-deep' and enc['side_info']['block_layers'] == 2
    dec = codec.decode_gop(overfit.gen_model(gop.scale_num, 'cuda', block_layers=2), enc, frames=[0])
    ref = torch.as_tensor(gop.infos[0]['ori']).cuda() + torch.tensor(gop.coord_mins[0], device='cuda', dtype=torch.int32)
    assert torch.equal(dec[0], ref), 'decode must be bit-exact'
    # hand-over to the fp32 executor: same master parameters, same optimiser state
    m2 = overfit.gen_model(gop.scale_num, 'cuda', seed=1, block_layers=2)
    o2 = FlatAdam(m2, lr=1e-3, gamma=1.0)
    overfit.warm_start(m2, o2, ck)
    assert torch.equal(m2.flat_parameters().cpu(), torch.cat([v.reshape(-1) for v in ck['model'].values()]))
    f0 = gop.frames[0]
    cont = [float(train_step(m2, o2, f0, gop.point_nums[0])) / gop.point_nums[0] for _ in range(6)]
    assert cont[-1] < cont[0], cont
