"""The bf16 training executor (csrc/train_bf16.hip) where its backward kernels walk SEVERAL tiles - the regime of every default overfit
(loot10: 337 k rows, owlii11: 1.25 M), which tests/test_gpu_bf16_train.py (6,821 rows and below) never enters:
  bbwd_k           software-pipelined over the tiles of a wave (index words, own rows and the first 14 gathers of the NEXT tile issued inside
                   the current one, the last tile "prefetches itself"): tiles_per_wave = ceil(t64 / (4 target)), t64 = ceil(R / 64),
                   target = min(max(1, 2 CUs / ng), nb) - one tile up to 16,384 rows (ng = 8) / 32,768 rows (ng = 1) on 256 CUs
  bocc_wgrad7_k    tiles_per_block = ceil(t64 / min(CUs, nb)); two waves per tap set alternate tiles, the tile + 2 prefetch runs from 3 on
  thead_bwd_k      min(2 CUs / 8, nb, ceil(t64 / 4)) blocks of 4 waves: several tiles per wave from 16,385 rows on
  bocc7m_k         min(ceil(t64 / 4), 2 CUs) workgroups: a loop over tile quads (unconditional prefetch of clamped rows) above 2 CUs x 256 rows
  wgrad_reduce_k   nb = 256 slab rows from 100,000 frame rows on: the unrolled branch, which has to stop at each launch's short range
Only the public entries are used (engine.net_forward_train_bf16, engine.net_backward_bf16, model_core.train_step).

Two comparands.
(1) The emulating oracle (oracle/network_bf16.py, autograd, on the GPU in fp32 with TF32 off, one scale at a time) at the project's
    tolerances for this pair: logits 2e-2, bits 1e-3 relative, every gradient tensor within 2e-2 of its own largest entry.  It catches a
    pipeline that mishandles every second tile; one lost 64-row tile in 33,000 rows moves a gradient by ~2e-3 and passes it.
(2) SUM OF PARTS, which does not.  A frame is S scales with distinct scale_idx.  Everything this executor stores is per row and rows of
    different scales never see each other, so a row's probabilities are bit-identical whether its scale is alone in a frame or one of S,
    and every weight gradient of the whole frame is the same set of fp32 terms as the sum of the S alone-frame gradients, associated
    differently.  The pieces stay at or below the one-tile-per-wave bound - the regime tests/test_gpu_bf16_train.py and (1) hold to the
    oracle - so whatever "whole minus sum of parts" shows beyond summation order is the multi-tile code's doing.
    How far pure re-association moves each tensor is measured on a comparand that is not the code under test: the fp32 executor
    (engine.net_forward / net_backward; float64-verified at these sizes by tests/test_gpu_multi_tile.py) on the same frames and model,
    d32_T = max |whole - sum of parts|.  The bf16 executor must satisfy, per tensor T,
        err_T <= max(8 d32_T, 1e-5 max|sum of parts_T|) + 1e-7 max|whole gradient vector|
    (8: up to 9 tiles per wave and 32 products per matrix instruction, where the fp32 kernels fold differently; 1e-5: the measured bound
    of exact-product sums at 39 k rows, test_weight_gradients_of_the_16x16x32_path...).  So that the check is not blind, the bound of
    every 3x3x3 kernel tensor must itself come out below 2e-4 of the tensor's largest entry on the large frame (one 64-row tile weighs
    ~5e-4 there) and below 1e-3 on the middle one (~2e-3).  The measured part, max(8 d32_T, 1e-5 max|T|), does (asserted: it is the
    1e-5 floor everywhere, d32_T / max|T| <= 6.5e-7).  The last term does not for the kernels whose largest gradient entry is below
    5e-4 of the whole vector's (large frame: 7 kernels of the outter blocks' Inception layers, the formula's bound up to 0.19 of the
    tensor's largest entry): such a tensor is held to 2e-4 (1e-3) of its own largest entry instead, never to the looser figure.
    Sensitivity, shown once by hand on a copy of the library (MI355X): bocc_wgrad7_k leaving out ONE full 64-row tile (the last but one of
    the frame, only where tiles_per_block >= 3) moves the first convolutions' kernel gradients by 4.1e-2 (middle) / 1.0e-2 (large) of
    their largest entry - 2,150 x / 369 x the bound; bbwd_k handing a wave's next tile the CURRENT tile's own rows: 2.9 / 2.2 of the
    largest entry, 47,000 x / 25,600 x the bound.  Both fail the three tests of the middle and large frame, the control passes.
Every bf16 run uses an arena pre-filled with 0xFF bytes and linr_debug_poison(0xFFFFFF); probabilities and gradients must be finite.
"""
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import network_bf16 as obf      # noqa: E402
from oracle import octree as ooct           # noqa: E402
from gpu_common import _model_and_oracle    # noqa: E402

BB_WAVES = 4          # csrc/train_bf16.hip
HB_WAVES = 4          # csrc/head_bwd.h


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ceil(a, b):
    return -(-a // b)


def _schedule(R, cus):
    """How the launches of one bf16 training step over a frame of R rows walk it (tb_grid, hb_blocks, linr_wg_blocks_for and the two
    first-convolution launches of csrc/train_bf16.hip restated)."""
    if os.environ.get('LINR_WG_BLOCKS'):
        pytest.skip('LINR_WG_BLOCKS=%s changes the slab rows (nb) these tests derive their schedules from' % os.environ['LINR_WG_BLOCKS'])
    t64 = _ceil(R, 64)
    nb = 256 if R >= 100000 else 128
    tpw = {}
    for ng in (8, 1):
        target = min(max(1, 2 * cus // ng), nb)
        tpw[ng] = max(1, _ceil(t64, BB_WAVES * target))
    head_blocks = max(1, min(2 * cus // 8, nb, _ceil(t64, HB_WAVES)))
    quads = _ceil(t64, 4)
    return {'t64': t64, 'nb': nb, 'tiles_per_wave': tpw, 'tiles_per_block': _ceil(t64, min(cus, nb)),
            'head_tiles_per_wave': _ceil(t64, HB_WAVES * head_blocks), 'quads_per_workgroup': _ceil(quads, min(quads, 2 * cus))}


def _one_tile(R, cus):
    """The regime tests/test_gpu_bf16_train.py covers: one tile per wave of every bbwd_k launch and of the heads, no tile + 2 prefetch
    in bocc_wgrad7_k, no loop in bocc7m_k, 128 slab rows."""
    s = _schedule(R, cus)
    return (s['tiles_per_wave'][8] == 1 and s['tiles_per_wave'][1] == 1 and s['head_tiles_per_wave'] == 1 and s['tiles_per_block'] <= 2
            and s['quads_per_workgroup'] == 1 and s['nb'] == 128)


def _piece(n, seed):
    """n sorted distinct voxels of a box at about half occupancy (about 14.4 of 27 neighbours present per row) and random occupancy:
    the generator of tests/test_gpu_multi_tile.py::occ7_inputs."""
    side = int(np.ceil((2.0 * n) ** (1.0 / 3.0))) + 1
    rng = np.random.default_rng(seed)
    coord = ooct.unique_sorted(rng.integers(0, side, size=(int(0.8 * side ** 3), 3)))[:n]
    assert len(coord) == n
    occ = (rng.random((n, 8)) < 0.5).astype(np.float32)
    return {'coord': coord, 'occ': occ, 'offset_tensor': ooct.offset_tensor(coord)}


def _sizes(total, S):
    """S ragged piece sizes that add up to `total`: total // S + 37 (i - S // 2), the last piece takes the remainder; a piece that is a
    multiple of 64 rows, or a boundary that falls on a tile edge, hands one row to the last piece."""
    sizes = [total // S + 37 * (i - S // 2) for i in range(S - 1)]
    start = 0
    for i in range(S - 1):
        while sizes[i] % 64 == 0 or (start + sizes[i]) % 64 == 0:
            sizes[i] += 1
        start += sizes[i]
    sizes.append(total - start)
    bounds = np.cumsum(sizes)[:-1]
    assert sizes[-1] > 0 and sum(sizes) == total and all(n % 64 for n in sizes) and all(int(b) % 64 for b in bounds), sizes
    return sizes


class _NoTF32:
    """fp32 matmuls of the GPU oracle in fp32 proper."""

    def __enter__(self):
        self.old = torch.backends.cuda.matmul.allow_tf32
        torch.backends.cuda.matmul.allow_tf32 = False

    def __exit__(self, *exc):
        torch.backends.cuda.matmul.allow_tf32 = self.old


def _logits(p):
    p = p.double()
    return torch.log(p) - torch.log1p(-p)


def _dirty_arena(frame):
    """The arena of the bf16 training executor comes uninitialised: here filled with 0xFF bytes (NaN patterns)."""
    from linr_pcgc_amd import _lib
    nbytes = _lib.lib().linr_net_train_bf16_arena_bytes(frame.rows, 1)
    frame.arena_train_bf16 = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device='cuda')


class _Poison:
    """linr_debug_poison in front of every launch (LDS and vector registers of all CUs filled), restored as
    test_bf16_training_does_not_depend_on_leftover_state restores it."""

    def __enter__(self):
        from linr_pcgc_amd import _lib
        self.L = _lib.lib()
        self.L.linr_debug_poison(0xFFFFFF)

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.L.linr_debug_poison(0xFFFFFF if os.environ.get('LINR_DEBUG_POISON') else 0)


def _run_bf16(frame, flat, gscale, backward=True):
    """forward (+ backward) of the bf16 training executor from a dirty arena and dirty CUs: probs [8, rows], bits (float), flat gradient"""
    from linr_pcgc_amd import engine
    _dirty_arena(frame)
    probs = torch.full((8, frame.rows), float('nan'), device='cuda')
    bits = torch.zeros(1, dtype=torch.float64, device='cuda')
    grads = torch.zeros_like(flat)
    with _Poison():
        engine.net_forward_train_bf16(frame, flat, probs, bits)
        if backward:
            engine.net_backward_bf16(frame, flat, grads, gscale)
    assert bool(torch.isfinite(probs).all()), '%d probabilities never written or not finite' % int((~torch.isfinite(probs)).sum())
    assert bool(torch.isfinite(grads).all()), '%d gradient entries not finite' % int((~torch.isfinite(grads)).sum())
    return probs, float(bits), grads


def _run_f32(frame, flat, gscale):
    from linr_pcgc_amd import engine
    grads = torch.zeros_like(flat)
    engine.net_forward(frame, flat, 0, 8, None, None)
    engine.net_backward(frame, flat, grads, gscale)
    assert bool(torch.isfinite(grads).all())
    return grads


def _case(pkg, total, S):
    """A frame of S pieces (scale_idx 0 .. S - 1) with `total` rows, the model (seed 8807, 5 fp32 Adam steps on this frame), and both
    executors on the whole frame and on every piece alone.  Computed once per module and left unchanged."""
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    sizes = _sizes(total, S)
    scales = []
    for i, n in enumerate(sizes):
        p = _piece(n, 7000 + 100 * S + i)
        p['scale_idx'] = i
        scales.append(p)
    point_num = int(sum(float(s['occ'].sum()) for s in scales))
    model, _ = _model_and_oracle(pkg, S, seed=8807)
    frame = model.make_frame(scales)
    assert frame.rows == total
    opt = FlatAdam(model)
    for _ in range(5):
        train_step(model, opt, frame, point_num)
    flat = model.flat_parameters()
    gscale = 1.0 / float(point_num)
    c = {'sizes': sizes, 'scales': scales, 'point_num': point_num, 'gscale': gscale, 'model': model, 'frame': frame, 'flat': flat,
         'names': [(k, v.numel(), tuple(v.shape)) for k, v in model.state_dict().items()],
         'sd': {k: v.detach().clone() for k, v in model.state_dict().items()}}
    assert [k for k, _ in model.named_parameters()] == [k for k, _, _ in c['names']] and sum(n for _, n, _ in c['names']) == flat.numel()
    c['whole'] = _run_bf16(frame, flat, gscale)
    c['whole32'] = _run_f32(frame, flat, gscale)
    c['alone'], c['alone32'] = [], []
    for s in scales:
        f = model.make_frame([s])
        c['alone'].append(_run_bf16(f, flat, gscale))
        c['alone32'].append(_run_f32(f, flat, gscale))
        del f
    return c


def _tensors(c, flat):
    off = 0
    for name, n, shape in c['names']:
        yield name, shape, flat[off:off + n]
        off += n


def _rows_do_not_depend_on_their_place(c, what):
    """(c): the probabilities of every scale of the whole frame bit-equal to those of the scale alone in a frame, the bits equal to the
    sum of the pieces' bits within 1e-9 relative (a float64 sum in another order)."""
    probs, bits, _ = c['whole']
    for i, (p, _, _) in enumerate(c['alone']):
        sl = c['frame'].scale_slice(i)
        if not torch.equal(probs[:, sl], p):
            ne = (probs[:, sl] != p).nonzero()
            k, r = int(ne[0, 0]), int(ne[0, 1])
            pytest.fail('%s: scale %d: %d probabilities differ between the whole frame and the scale alone; first: stage %d, row %d of the '
                        'scale (frame row %d): %.9g against %.9g' % (what, i, len(ne), k, r, sl.start + r, float(probs[k, sl.start + r]),
                                                                       float(p[k, r])))
    parts = sum(b for _, b, _ in c['alone'])
    assert abs(bits - parts) <= 1e-9 * parts, (bits, parts)


def _sum_of_parts(c, what, kernel_limit=None):
    """(d): per tensor, err_T = max |whole - sum of parts| of the bf16 executor against the bound built from the fp32 executor's
    d32_T on the same frames (module docstring).  kernel_limit: what the bound of a 3x3x3 kernel tensor may be at most, as a fraction of
    the tensor's largest entry: the measured part max(8 d32_T, 1e-5 max|T|) must be below it (asserted), and where the formula's last
    term carries the bound above it the tensor is held to kernel_limit x max|T| instead, so that NO 3x3x3 kernel tensor is checked more
    loosely than one tile weighs.  Prints the worst ratios; returns them."""
    whole = c['whole'][2].double()
    parts = sum(g.double() for _, _, g in c['alone'])
    whole32 = c['whole32'].double()
    parts32 = sum(g.double() for g in c['alone32'])
    vec_max = float(whole.abs().max())
    bad, blind, capped = [], [], []
    worst = {'err': (0.0, ''), 'd32': (0.0, ''), 'of_bound': (0.0, ''), 'kernel_bound': (0.0, '')}
    for (name, shape, w), (_, _, p), (_, _, w32), (_, _, p32) in zip(_tensors(c, whole), _tensors(c, parts), _tensors(c, whole32),
                                                                       _tensors(c, parts32)):
        tmax = float(p.abs().max())
        err = float((w - p).abs().max())
        d32 = float((w32 - p32).abs().max())
        noise = max(8.0 * d32, 1e-5 * tmax)
        bound = noise + 1e-7 * vec_max
        rel = lambda v: v / max(tmax, 1e-300)
        strict = False
        kernel3 = len(shape) == 3 and shape[0] == 27
        if kernel3 and kernel_limit is not None:
            if tmax > 0 and not noise < kernel_limit * tmax:          # the fp32 executor's own noise would blind the check
                blind.append((name, rel(noise), rel(d32)))
            if bound >= kernel_limit * tmax:          # the 1e-7 max|gradient vector| term alone is above the limit: a kernel whose largest
                capped.append((name, rel(bound)))     # gradient entry is tiny beside the vector's - held to the limit itself
                bound, strict = kernel_limit * tmax, tmax > 0
        if kernel3 and rel(bound) > worst['kernel_bound'][0]:
            worst['kernel_bound'] = (rel(bound), name)
        for key, v in (('err', rel(err)), ('d32', rel(d32)), ('of_bound', err / max(bound, 1e-300))):
            if v > worst[key][0]:
                worst[key] = (v, name)
        if err > bound or (strict and err >= bound):
            bad.append((name, err, bound, d32, tmax))
    print('%s: %d rows, pieces %s: worst err_T / max|T| %.3e (%s), worst d32_T / max|T| %.3e (%s), worst err_T / bound_T %.3g (%s), '
          'largest bound of a 3x3x3 kernel tensor %.3e of its largest entry (%s)'
          % (what, c['frame'].rows, c['sizes'], worst['err'][0], worst['err'][1], worst['d32'][0], worst['d32'][1], worst['of_bound'][0],
             worst['of_bound'][1], worst['kernel_bound'][0], worst['kernel_bound'][1]))
    if capped:
        print('%s: %d 3x3x3 kernel tensors whose formula bound is above %.0e of their largest entry, held to that limit instead (name, '
              'formula bound / max): %s' % (what, len(capped), kernel_limit, [(n, '%.3e' % b) for n, b in capped]))
    assert not blind, ('%s: the fp32 executor\'s own re-association noise puts the bound of %d 3x3x3 kernel tensors above %.0e of their '
                       'largest entry (name, max(8 d32, 1e-5 max) / max, d32 / max): %s' % (what, len(blind), kernel_limit, blind[:6]))
    assert not bad, ('%s: %d gradient tensors of the whole frame differ from the sum of the alone frames by more than re-association '
                     'explains (name, err, bound, d32, own max): %s' % (what, len(bad), bad[:6]))
    return worst


# ---- the three frames -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def middle(pkg):
    cus = _cus()
    _schedule(1, cus)                                        # (skips when LINR_WG_BLOCKS is forced)
    return _case(pkg, 64 * BB_WAVES * min(2 * cus, 128) + 132, 3)          # three tiles past the one-tile bound of the ng = 1 launches


@pytest.fixture(scope='module')
def large(pkg):
    cus = _cus()
    total = 2 * cus * 256 + 257
    for S in range(9, 17):
        if all(_one_tile(n, cus) for n in _sizes(total, S)):
            return _case(pkg, total, S)
    pytest.skip('%d rows on %d CUs: no 9 .. 16 pieces that each stay in the one-tile regime (16 pieces: %s)' % (total, cus, _sizes(total, 16)))


@pytest.fixture(scope='module')
def control(pkg):
    _schedule(1, _cus())
    return _case(pkg, 6007, 2)


# ---- 1: middle frame ------------------------------------------------------------------------------------------------------------------
def test_middle_frame_matches_the_emulating_oracle(middle):
    """64 x 4 x min(2 CUs, 128) + 132 rows in 3 ragged scales (MI355X: 32,900 = 10,929 + 10,966 + 11,005): tiles_per_wave >= 2 for the
    grouped (ng = 8) and the single (ng = 1) bbwd_k launches, tiles_per_block >= 3 in bocc_wgrad7_k (its tile + 2 prefetch runs), several
    tiles per wave of the heads; every piece alone at one tile per wave.  (a) the whole frame and (b) every piece alone against the
    emulating oracle of its scale: logits per scale and stage within 2e-2, bits 1e-3 relative, every gradient tensor within 2e-2 of its own
    largest entry.
    Measured on the MI355X: logits within 1.60e-3 (whole frame and pieces alone: the same bits), bits rel 3.8e-8, worst gradient
    tensor at 3.07e-3 of its largest entry for the whole frame (outter_blocks.6 conv1_0.kernel) and 1.71e-2 for a piece alone
    (block_in conv1_0.kernel); 7.3 s, 7.2 s of them the oracle's three forward and backward passes."""
    c, cus = middle, _cus()
    s = _schedule(c['frame'].rows, cus)
    assert s['tiles_per_wave'][8] >= 2 and s['tiles_per_wave'][1] >= 2 and s['tiles_per_block'] >= 3 and s['head_tiles_per_wave'] >= 2, s
    assert all(_one_tile(n, cus) for n in c['sizes']), (c['sizes'], cus)
    leaves = {k: v.cuda().requires_grad_() for k, v in c['sd'].items()}
    names = list(leaves)
    ref_bits, ref_grads, worst_logit = [], [], [0.0, 0.0]
    t0 = time.perf_counter()
    with _NoTF32():
        for i, sc in enumerate(c['scales']):
            nbr = torch.from_numpy(ooct.neighbour_table(sc['coord'])).long().cuda()
            out = obf.train_forward_scale(leaves, {'offset_tensor': torch.from_numpy(sc['offset_tensor']).cuda(),
                                                   'occ': torch.from_numpy(sc['occ']).cuda(), 'nbr': nbr, 'scale_idx': i})
            sl = c['frame'].scale_slice(i)
            for k in range(8):
                z = out['logits'][k].detach().reshape(-1).double()
                for j, p in enumerate((c['whole'][0][k, sl], c['alone'][i][0][k])):
                    worst_logit[j] = max(worst_logit[j], float((_logits(p) - z).abs().max()))
            ref_bits.append(float(out['bits'].detach()))
            g = torch.autograd.grad(out['bits'] * c['gscale'], [leaves[k] for k in names], allow_unused=True)
            ref_grads.append(torch.cat([(torch.zeros_like(leaves[k]) if t is None else t).reshape(-1) for k, t in zip(names, g)]).double())
            del out, g
    torch.cuda.synchronize()
    t_oracle = time.perf_counter() - t0
    assert max(worst_logit) <= 2e-2, 'logits %.3e (whole frame) / %.3e (pieces alone) from the emulating oracle' % tuple(worst_logit)

    def grads_close(got, ref, what):
        worst, bad = (0.0, ''), []
        for (name, _, a), (_, _, b) in zip(_tensors(c, got.double()), _tensors(c, ref)):
            gmax, err = float(b.abs().max()), float((a - b).abs().max())
            if err > 2e-2 * gmax:
                bad.append((name, err, gmax))
            if gmax > 0 and err / gmax > worst[0]:
                worst = (err / gmax, name)
        assert not bad, '%s: gradient tensors off by more than 2e-2 of their own largest entry: %s' % (what, bad[:6])
        return worst
    w_alone = (0.0, '')
    for i in range(len(c['scales'])):                                     # (b) the anchor
        assert abs(c['alone'][i][1] - ref_bits[i]) <= 1e-3 * ref_bits[i], (i, c['alone'][i][1], ref_bits[i])
        w_alone = max(w_alone, grads_close(c['alone'][i][2], ref_grads[i], 'piece %d alone' % i))
    total = sum(ref_bits)
    assert abs(c['whole'][1] - total) <= 1e-3 * total, (c['whole'][1], total)
    w_whole = grads_close(c['whole'][2], sum(ref_grads), 'whole frame')          # (a)
    print('middle frame against the emulating oracle: %d rows, pieces %s; logits %.3e (whole) / %.3e (alone), bits rel %.2e, worst gradient '
          'tensor at %.3e of its largest entry (whole: %s) / %.3e (alone: %s); the oracle took %.1f s'
          % (c['frame'].rows, c['sizes'], worst_logit[0], worst_logit[1], abs(c['whole'][1] - total) / total, w_whole[0], w_whole[1],
             w_alone[0], w_alone[1], t_oracle))


def test_middle_frame_is_the_sum_of_its_scales(middle):
    """(c) probabilities of every scale bit-equal to the scale alone, bits the sum of the pieces' bits; (d) every gradient tensor of
    the whole frame within the measured re-association bound of the sum of the alone frames' gradients; the bound of every 3x3x3 kernel
    tensor below 1e-3 of the tensor's largest entry (one 64-row tile of 32,900 rows weighs ~2e-3).
    Measured on the MI355X: worst err_T / max|T| 6.5e-7, worst d32_T / max|T| 6.5e-7 (both outter_blocks.0 conv1_2.kernel), worst err_T at
    0.017 of its bound (inner_mlps.1.0.0.bias); largest bound of a 3x3x3 kernel tensor 8.96e-4 of its largest entry (outter_blocks.3
    conv1_1.kernel), none held to the limit; 0.02 s."""
    _rows_do_not_depend_on_their_place(middle, 'middle frame')
    _sum_of_parts(middle, 'middle frame', kernel_limit=1e-3)


# ---- 2: large frame -------------------------------------------------------------------------------------------------------------------
def test_large_frame_is_the_sum_of_its_scales(large):
    """2 CUs x 256 + 257 rows in 9 ragged scales (MI355X: 131,329 rows, pieces of 14,444 to 14,740): above bocc7m_k's loop point (every
    workgroup walks two tile quads, the last one ragged) and at least 100,000 rows (256 slab rows: wgrad_reduce_k's unrolled branch
    over the short ranges of the launches), up to 9 tiles per wave of bbwd_k; every piece alone in the one-tile regime.  No oracle at this
    size: (c) and (d), the bound of every 3x3x3 kernel tensor below 2e-4 of the tensor's largest entry (one 64-row tile weighs ~5e-4).
    Measured on the MI355X: worst err_T / max|T| 1.5e-7 (outter_blocks.5 conv1_1.kernel), worst d32_T / max|T| 2.6e-7 (prune_blocks.4
    kernel), worst err_T at 0.0115 of its bound (inner_mlps.6.0.0.weight); 7 kernels (conv0_0 / conv0_1 / conv1_1 of outter_blocks 1 .. 5,
    largest gradient entry 5e-7 .. 5e-4 of the vector's) have a formula bound of 2.9e-4 .. 0.19 of their largest entry and are held to
    2e-4 of it; 0.2 s with the nine alone frames."""
    c, cus = large, _cus()
    s = _schedule(c['frame'].rows, cus)
    assert s['quads_per_workgroup'] >= 2 and s['nb'] == 256 and c['frame'].rows >= 100000 and s['tiles_per_wave'][8] >= 2, s
    assert all(_one_tile(n, cus) for n in c['sizes']), (c['sizes'], cus)
    _rows_do_not_depend_on_their_place(c, 'large frame')
    _sum_of_parts(c, 'large frame', kernel_limit=2e-4)


def test_large_frame_first_convolutions_match_the_4x4x4_kernel(large, monkeypatch):
    """The forward of the large frame once more with LINR_BOCC7_MFMA16=0: bocc7_k has one row per lane and no loop, bocc7m_k walks two
    tile quads per workgroup here.  The criteria of test_first_convolutions_as_one_matrix_product_match_the_4x4x4_kernel: logits
    within 1e-2, at most 5 % of them moved by more than 1e-4, bits within 1e-4 relative, stage 0 bit-equal.
    Measured on the MI355X: logits within 1.05e-3, 0.005 % of them moved by more than 1e-4, bits rel 3.3e-10; 0.01 s."""
    c = large
    monkeypatch.setenv('LINR_BOCC7_MFMA16', '0')
    probs, bits, _ = _run_bf16(c['frame'], c['flat'], c['gscale'], backward=False)
    monkeypatch.delenv('LINR_BOCC7_MFMA16')
    d = (_logits(probs) - _logits(c['whole'][0])).abs()
    moved = float((d > 1e-4).double().mean())
    print('large frame, bocc7m_k against bocc7_k: logits within %.3e, %.3f %% of them moved by more than 1e-4, bits rel %.2e'
          % (float(d.max()), 100.0 * moved, abs(bits - c['whole'][1]) / c['whole'][1]))
    assert float(d.max()) <= 1e-2, float(d.max())
    assert moved <= 0.05, moved
    assert abs(bits - c['whole'][1]) <= 1e-4 * c['whole'][1], (bits, c['whole'][1])
    assert torch.equal(probs[0], c['whole'][0][0]), 'stage 0 does not read the occupancy convolutions'


# ---- 3: control -----------------------------------------------------------------------------------------------------------------------
def test_control_frame_is_the_sum_of_its_scales(control):
    """The noise floor of the identity: 2 pieces of about 3,000 rows (6,007 = 2,966 + 3,041), the whole frame itself in the one-tile
    regime - nothing new runs, and (c) pins the premise that a row does not depend on its place in the frame.
    Measured on the MI355X: worst err_T / max|T| 3.9e-7 (inner_mlps.0.0.2.bias), worst d32_T / max|T| 2.4e-7, worst err_T at 0.033 of
    its bound; largest bound of a 3x3x3 kernel tensor 4.2e-5 of its largest entry; 0.03 s."""
    c, cus = control, _cus()
    assert _one_tile(c['frame'].rows, cus) and _schedule(c['frame'].rows, cus)['tiles_per_block'] == 1, _schedule(c['frame'].rows, cus)
    _rows_do_not_depend_on_their_place(c, 'control frame')
    _sum_of_parts(c, 'control frame')


# ---- 4: the fused step ----------------------------------------------------------------------------------------------------------------
def test_fused_step_sees_the_gradient_of_the_large_frame(large):
    """One train_step with train_precision 'bf16' from zero moments on the large frame: the returned bits bit-equal to
    net_forward_train_bf16's, exp_avg = (1 - beta1) (g + weight_decay p) with g from net_backward_bf16 at the same gscale and the
    hyperparameters of the FlatAdam object as the C entry hands them to the kernel (rounded to float), rtol 1e-6 and atol 1e-12: the
    kernel's two fp32 roundings (fmaf, then the product).
    Measured on the MI355X: bits 1,051,954.056 both ways, worst exp_avg entry at 0.097 of the tolerance."""
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    c = large
    model, flat = c['model'], c['flat']
    p0 = flat.clone()
    opt = FlatAdam(model)
    _dirty_arena(c['frame'])
    model.train_precision = 'bf16'
    try:
        with _Poison():
            bits = float(train_step(model, opt, c['frame'], c['point_num']))
    finally:
        model.train_precision = 'f32'
        flat.copy_(p0)
    assert bits == c['whole'][1], (bits, c['whole'][1])
    omb1, wd = float(np.float32(1.0 - opt.betas[0])), float(np.float32(opt.weight_decay))
    ref = omb1 * (c['whole'][2].double() + wd * p0.double())
    err = (opt.exp_avg.double() - ref).abs()
    ratio = float((err / (1e-12 + 1e-6 * ref.abs())).max())
    print('fused bf16 step on %d rows: bits %.3f, exp_avg at %.3g of rtol 1e-6 + atol 1e-12' % (c['frame'].rows, bits, ratio))
    assert bool(torch.isfinite(opt.exp_avg).all()) and ratio <= 1.0, ratio
