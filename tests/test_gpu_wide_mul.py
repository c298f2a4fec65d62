"""train_precision 'bf16-mul' (hidden_channel_conv 16 / 32): the fp32 wide step with the PRODUCTS of its 3x3x3 convolutions on bf16 matrix
instructions (csrc/wide_mul.hip; LINR_MUL_BF16).  The contract: operands rounded to bf16 at the multiply, fp32 sums, everything that is
not a product of a convolution computed in fp32 on the unrounded values.  rb(t) = t.to(bfloat16).to(float32).

Measured on the MI355X (profiles/wide_bf16_mul.txt): every entry of the three entries at <= 0.056 of gpu_common's rounding bound against
the float64 convolution of the rounded operands (C_ROUND stays 64), mul='f32' at 454 - 670 x; network against the emulating oracle: logits
<= 2.2e-3, bits <= 2.1e-7, gradients <= 1.26e-2 of a tensor's largest entry, cosine with the fp32 oracle >= 0.999974 overall, >= 0.996219 per
tensor; per-epoch loss within 0.01 % of fp32."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import network as onet          # noqa: E402
from oracle import octree as ooct           # noqa: E402
from gpu_common import C_ROUND, _U, _within_rounding          # noqa: E402,F401
import wide_bf16_mul_ref as mref            # noqa: E402

pytestmark = pytest.mark.gpu


def rb(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _maps(coord):
    """coord: int32 [n, 3] on the GPU, sorted -> the oracle's [n, 27] map and the library's maps."""
    from linr_pcgc_amd import ops
    n = coord.shape[0]
    ld = (n + 63) // 64 * 64
    nbr = torch.full((27, ld), -1, dtype=torch.int32, device='cuda')
    nbr[:, :n] = ops.kmap_build(coord.to(torch.int32).contiguous())
    lo, mask = ops.kmap_compress(nbr, n)
    return {'n': n, 'nbr_o': torch.from_numpy(ooct.neighbour_table(coord.cpu().numpy().astype(np.int32))).long().cuda(), 'nbr': nbr,
            'lo': lo, 'mask': mask, 'tile8t': ops.kmap_tile8t(nbr, n)}


_SMALL = {}


def _small(pkg, n):
    """A random sparse cloud of n voxels in a 24^3 box (made once per n)."""
    if n not in _SMALL:
        rng = np.random.default_rng(1000 + n)
        lin = rng.choice(24 ** 3, size=n, replace=False)
        c = ooct.unique_sorted(np.stack([lin // 576, (lin // 24) % 24, lin % 24], axis=1).astype(np.int32))
        assert len(c) == n
        _SMALL[n] = _maps(torch.from_numpy(c).cuda())
    return _SMALL[n]


@pytest.fixture(scope='module')
def finest9(pkg):
    """The finest scale of the 9-bit shell of tests/test_gpu_wide.py (156,985 rows): the convolutions' workgroups walk several tiles."""
    from linr_pcgc_amd import synthetic
    from linr_pcgc_amd.module_utils import prepare_frame
    fr = prepare_frame(synthetic.sequence_frame({'bitdepth': 9, 'radius': 200, 'thickness': 0.5}, 0), None, 64, device='cuda')
    m = _maps(fr['all_input_info'][0]['coord'])
    assert m['n'] > 2 * _cus() * 256, (m['n'], _cus())
    return m


def _nan_blocks(n, nb):
    return [torch.full((n, 8), float('nan'), device='cuda') for _ in range(nb)]


def _padded_blocks(t, nb, fill=0.0):
    """[n, c <= 8 nb] -> nb blocks (views buf[i, 1:] of [n + 1, 8] buffers whose row 0 is zero; channels past c = fill)."""
    n = t.shape[0]
    buf = torch.full((nb, n + 1, 8), fill, device=t.device)
    buf[:, 0] = 0.0
    for i in range(nb):
        w = min(8, t.shape[1] - 8 * i)
        buf[i, 1:, :w] = t[:, 8 * i:8 * i + w]
    return [buf[i, 1:] for i in range(nb)]


def _inputs(n, cin, cout, seed):
    torch.manual_seed(seed)
    return {'W': torch.randn(27, cin, cout, device='cuda') * 0.1, 'b': torch.randn(cout, device='cuda'), 'x': torch.randn(n, cin, device='cuda'),
            'res': torch.randn(n, cout, device='cuda'), 'g': torch.randn(n, cout, device='cuda'), 'act': torch.randn(n, cin, device='cuda'),
            'old': torch.randn(n, cin, device='cuda')}


def _run_entries(m, cin, cout, t, mul):
    """Forward with bias / residual / ReLU, the weight and bias gradients, backward-data with the ReLU mask and LINR_ACCUM (cin % 8 == 0).
    Outputs start as NaN (the accumulated one holds `old`)."""
    from linr_pcgc_amd import ops
    n, nbi, nbo = m['n'], (cin + 7) // 8, cout // 8
    xs = _padded_blocks(t['x'], nbi, fill=7.0 if cin % 8 else 0.0)          # channels past cin must be ignored
    gs = _padded_blocks(t['g'], nbo)
    out = {'fwd': torch.cat(ops.spconv_wide(xs, m['lo'], m['mask'], n, t['W'], t['b'], res=_padded_blocks(t['res'], nbo), relu=True,
                                            outs=_nan_blocks(n, nbo), mul=mul), dim=1)}
    gw, gb = torch.full((27, cin, cout), float('nan'), device='cuda'), torch.full((cout,), float('nan'), device='cuda')
    ops.spconv_wgrad_wide(xs, gs, m['nbr'], m['tile8t'], n, cin, cout, gw=gw, gb=gb, mul=mul)
    out['gw'], out['gb'] = gw, gb
    if cin % 8 == 0:
        outs = _padded_blocks(t['old'], nbi)
        ops.spconv_wide(gs, m['lo'], m['mask'], n, t['W'], None, bwd=True, act=_padded_blocks(t['act'], nbi), outs=outs, accumulate=True,
                        mul=mul)
        out['bwd'] = torch.cat(outs, dim=1)
    return out


def _reference(m, cin, cout, t):
    """float64 oracle.conv3 on rb(x), rb(W), rb(g); bias, residual, the accumulated content and the bias gradient unrounded.  Per output
    (exact, sum of |terms|)."""
    nbr_o = m['nbr_o']
    x64, W64 = rb(t['x']).double().requires_grad_(), rb(t['W']).double().requires_grad_()
    b64, g64 = t['b'].double().reshape(1, -1), rb(t['g']).double()
    y = onet.conv3(x64, nbr_o, W64, b64)
    ref = {}
    with torch.no_grad():
        ref['fwd'] = (torch.relu(y + t['res'].double()),
                      onet.conv3(x64.abs(), nbr_o, W64.abs(), b64.abs()) + t['res'].double().abs())
    gx, gw = torch.autograd.grad(y, [x64, W64], g64)
    xabs, wabs = x64.detach().abs().requires_grad_(), W64.detach().abs().requires_grad_()
    gx_abs, gw_abs = torch.autograd.grad(onet.conv3(xabs, nbr_o, wabs, torch.zeros_like(b64)), [xabs, wabs], g64.abs())
    ref['gw'] = (gw, gw_abs)
    ref['gb'] = (t['g'].double().sum(0), t['g'].double().abs().sum(0))
    if cin % 8 == 0:
        ref['bwd'] = ((gx + t['old'].double()) * (t['act'] > 0), gx_abs + t['old'].double().abs())
    return ref


def _worst_ratio(got, exact, absum):
    return float(((got.double() - exact).abs() / (C_ROUND * _U * absum).clamp(min=1e-300)).max())


SHAPES = [(8, 8), (16, 16), (8, 16), (16, 8), (32, 32), (32, 16), (16, 32), (3, 16), (7, 32)]


def _check_entries(m, cin, cout):
    t = _inputs(m['n'], cin, cout, cin * 100 + cout)
    got, ref = _run_entries(m, cin, cout, t, 'bf16'), _reference(m, cin, cout, t)
    worst = {k: _worst_ratio(got[k], *ref[k]) for k in ref}
    print('bf16-mul conv %d -> %d at %d rows: worst entry at %s of its bound' % (cin, cout, m['n'], {k: '%.3g' % v for k, v in worst.items()}))
    for k in ref:
        _within_rounding(got[k], ref[k][0], ref[k][1], '%s %d -> %d' % (k, cin, cout))


# ---- 1. each entry is the float64 convolution of the rounded operands -----------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 63, 257, 1000])
@pytest.mark.parametrize('cin,cout', SHAPES)
def test_entries_are_the_float64_convolution_of_the_rounded_operands(pkg, cin, cout, n):
    """Every entry of every output within gpu_common's rounding bound (C_ROUND 2^-24 sum |terms|, terms from the rounded operands) of the
    float64 convolution of rb(x), rb(W), rb(g): the products are exact, so only the fp32 sums err."""
    _check_entries(_small(pkg, n), cin, cout)


@pytest.mark.parametrize('cin,cout', [(16, 16), (32, 32), (3, 16)])
def test_entries_multi_tile(pkg, finest9, cin, cout):
    _check_entries(finest9, cin, cout)


def _paired(pkg, m, h):
    from linr_pcgc_amd import ops
    n, nbr_o = m['n'], m['nbr_o']
    torch.manual_seed(h)
    sets = []
    for _ in range(2):
        sets.append((torch.randn(n, h, device='cuda'), torch.randn(n, h, device='cuda'), torch.full((27, h, h), float('nan'), device='cuda'),
                     torch.full((h,), float('nan'), device='cuda')))
    (xa, ga, gwa, gba), (xb, gb_, gwb, gbb) = sets
    deferred = []
    nb = h // 8
    ops.spconv_wgrad_wide2(_padded_blocks(xa, nb), _padded_blocks(ga, nb), gwa, gba, _padded_blocks(xb, nb), _padded_blocks(gb_, nb), gwb, gbb,
                           m['tile8t'], n, deferred, mul='bf16')
    assert len(deferred) == 2
    ops.wide_reduce_many(deferred)
    worst = []
    for which, (x, g, gw, gb) in zip('AB', sets):
        W64 = torch.zeros(27, h, h, dtype=torch.float64, device='cuda', requires_grad=True)
        b64 = torch.zeros(1, h, dtype=torch.float64, device='cuda')
        gw64 = torch.autograd.grad(onet.conv3(rb(x).double(), nbr_o, W64, b64), [W64], rb(g).double())[0]
        gw_abs = torch.autograd.grad(onet.conv3(rb(x).double().abs(), nbr_o, W64, b64), [W64], rb(g).double().abs())[0]
        worst += [_worst_ratio(gw, gw64, gw_abs), _worst_ratio(gb, g.double().sum(0), g.double().abs().sum(0))]
        print('bf16-mul paired weight gradients h = %d at %d rows: worst entry at %s of its bound' % (h, n, ['%.3g' % w for w in worst]))
        _within_rounding(gw, gw64, gw_abs, 'kernel gradient ' + which)
        _within_rounding(gb, g.double().sum(0), g.double().abs().sum(0), 'bias gradient ' + which)


@pytest.mark.parametrize('h', [8, 16])
def test_paired_entry_small(pkg, h):
    """linr_spconv_wgrad_wide2 with the flag through the deferred reductions, 257 rows (most of the 256 slab rows empty)."""
    _paired(pkg, _small(pkg, 257), h)


@pytest.mark.parametrize('h', [8, 16])
def test_paired_entry_multi_tile(pkg, finest9, h):
    _paired(pkg, finest9, h)


# ---- 2. the rounding is really applied, and only to the products ------------------------------------------------------------------------
@pytest.mark.parametrize('cin,cout', [(16, 16), (32, 32)])
def test_rounding_is_applied_to_the_products_and_only_to_them(pkg, cin, cout):
    m = _small(pkg, 1000)
    t = _inputs(m['n'], cin, cout, 7 * cin + cout)
    ref = _reference(m, cin, cout, t)
    f32 = _run_entries(m, cin, cout, t, 'f32')
    for k in ('fwd', 'gw', 'bwd'):          # the unrounded product differs from the rounded one by ~2^-9 relative per operand
        r = _worst_ratio(f32[k], *ref[k])
        print("mul='f32' against the rounded-operand reference, %s %d -> %d: worst entry at %.3g of the bound" % (k, cin, cout, r))
        assert r > 1.0, (k, r)
    # pre-rounded operands: both multiplications compute the same exact products
    tr = dict(t, x=rb(t['x']), W=rb(t['W']), g=rb(t['g']))
    ref_r = _reference(m, cin, cout, tr)
    for mul in ('bf16', 'f32'):
        got = _run_entries(m, cin, cout, tr, mul)
        for k in ref_r:
            _within_rounding(got[k], ref_r[k][0], ref_r[k][1], '%s, pre-rounded operands, mul=%s' % (k, mul))


def test_bias_and_residual_come_through_unrounded(pkg):
    """A bias, and a residual, of 1 + 2^-20 (bf16 would make it 1) on an all-zero input: exactly that, in every entry."""
    from linr_pcgc_amd import ops
    m = _small(pkg, 257)
    n, v = m['n'], 1.0 + 2.0 ** -20
    W = torch.randn(27, 16, 16, device='cuda')
    xs = _padded_blocks(torch.zeros(n, 16, device='cuda'), 2)
    full = torch.full((n, 16), v, device='cuda')
    out = ops.spconv_wide(xs, m['lo'], m['mask'], n, W, torch.full((16,), v, device='cuda'), outs=_nan_blocks(n, 2), mul='bf16')
    assert torch.equal(torch.cat(out, dim=1), full)
    out = ops.spconv_wide(xs, m['lo'], m['mask'], n, W, torch.zeros(16, device='cuda'), res=_padded_blocks(full, 2), outs=_nan_blocks(n, 2),
                          mul='bf16')
    assert torch.equal(torch.cat(out, dim=1), full)
    gi = ops.spconv_wide(xs, m['lo'], m['mask'], n, W, None, bwd=True, res=_padded_blocks(full, 2), outs=_nan_blocks(n, 2), mul='bf16')
    assert torch.equal(torch.cat(gi, dim=1), full)


# ---- 3. fused epilogues -----------------------------------------------------------------------------------------------------------------
def _model(hidden, scale_num=5, block_layers=1, seed=8807, tp='bf16-mul'):
    from linr_pcgc_amd.model_core import LINR_PCGC_Model
    torch.manual_seed(seed)
    model = LINR_PCGC_Model({'scale_num': scale_num, 'in_channel': 7, 'hidden_channel_conv': hidden, 'block_layers': block_layers,
                             'outstage': 8, 'instage': 1})
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.cuda()
    model.train_precision = tp
    return model, sd


def _train_pass(model, frame, gscale, probs=None):
    """The training forward (keep) and backward through the executor's own tape: tape, bits, the flat gradient."""
    model._ensure_grad_views()
    bits = torch.zeros(1, dtype=torch.float64, device='cuda')
    with torch.no_grad():
        model._flat_grad.zero_()
        tape = model._wide.forward(frame, 0, 8, probs, bits, keep=True)
        model._wide.backward(frame, tape, gscale)
    return tape, bits, model._flat_grad.clone()


@pytest.mark.parametrize('hidden,block_layers', [(16, 1), (32, 1), (16, 2), (32, 2)])
def test_fused_epilogues_are_bitwise_the_two_launch_form(pkg, shell, hidden, block_layers):
    """EPI 1 .. 4 with the flag: the side outputs computed in the convolutions' epilogues (h1 = conv1_0, the layer output's upper half =
    conv1_2 + residual; gM and conv1_0's backward-data, which every upstream gradient depends on) are bitwise those of linr_linear_wide
    on the fp32 rows (LINR_WIDE_FUSE_PW=0's schedule): the side paths read unrounded values and keep their fmaf chains."""
    def run(fuse):
        model, _ = _model(hidden, block_layers=block_layers)
        model._wide.fuse_pw = fuse
        frame = model.make_frame(shell['scales'])
        tape, bits, grads = _train_pass(model, frame, 1.0 / shell['point_num'])
        side = []
        for bt in [tape['bin']] + [st['blk'] for st in tape['stages'] if st['blk'] is not None]:
            for lt in bt['layers']:
                side += [b.clone() for b in lt['h1']]
            side += [b.clone() for b in bt['il']]
        return side, bits, grads
    (sa, ba, ga), (sb, bb, gb) = run(True), run(False)
    assert len(sa) == len(sb) and len(sa) > 0 and bool(torch.isfinite(ga).all())
    for x, y in zip(sa, sb):
        assert torch.equal(x, y)
    assert torch.equal(ba, bb) and torch.equal(ga, gb)


# ---- 4. the network against an oracle that rounds where the kernels round ------------------------------------------------------------------
def _emulated_grads(sd, scales, gscale, emulate):
    leaves = {k: v.clone().requires_grad_() for k, v in sd.items()}
    outs = []
    ctx = mref.emulated() if emulate else _Null()
    with ctx:
        total = 0
        for s in onet.to_torch_scales(scales):
            if s['occ'].shape[0] == 0:          # an empty scale costs nothing and reaches no parameter
                outs.append(None)
                continue
            o = onet.forward_scale(leaves, s)
            outs.append(o)
            total = total + o['bits']
        (total * gscale).backward()
    return leaves, outs, float(total)


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _network_against_the_emulating_oracle(model, sd, scales, point_num, what):
    """Bounds: those the project holds its bf16-storage executor to (an fp32 activation that differs in its last bits between kernel and
    oracle can round to the neighbouring bf16, so fp32-order bounds do not apply): logits 2e-2, bits 1e-3 relative, every gradient
    tensor within 2e-2 of its own largest entry, cosine with the fp32 oracle's gradient >= 0.999 overall and >= 0.99 per tensor."""
    frame = model.make_frame([{k: v for k, v in s.items() if k != 'nbr'} for s in scales])
    gscale = 1.0 / point_num
    probs = torch.full((8, frame.rows), float('nan'), device='cuda')
    _, bits, grads = _train_pass(model, frame, gscale, probs)
    leaves, outs, ref_bits = _emulated_grads(sd, scales, gscale, True)
    plain, _, _ = _emulated_grads(sd, scales, gscale, False)
    worst_z = 0.0
    for i, o in enumerate(outs):
        sl = frame.scale_slice(i)
        for k in range(8):
            if o is None:
                continue
            p = probs[k, sl].double().cpu()
            z = torch.log(p) - torch.log1p(-p)
            if p.numel():
                worst_z = max(worst_z, float((z - o['logits'][k].reshape(-1).double()).abs().max()))
    rel_bits = abs(float(bits) - ref_bits) / ref_bits
    worst_g, worst_cos, own_cos, off = (0.0, ''), (1.0, ''), (1.0, ''), 0
    dots = [0.0, 0.0, 0.0]
    for name, v in leaves.items():
        n = v.numel()
        mine = grads[off:off + n].view(v.shape).double().cpu()
        off += n
        ref = torch.zeros_like(mine) if v.grad is None else v.grad.double()
        f32 = torch.zeros_like(mine) if plain[name].grad is None else plain[name].grad.double()
        gmax = float(ref.abs().max())
        if gmax == 0.0:
            assert float(mine.abs().max()) == 0.0, name          # a scale the frame does not hold: exactly zero
            continue
        err = float((mine - ref).abs().max()) / gmax
        if err > worst_g[0]:
            worst_g = (err, name)
        cos = float((mine * f32).sum() / (mine.norm() * f32.norm()))
        if cos < worst_cos[0]:
            worst_cos = (cos, name)
        cos = float((ref * f32).sum() / (ref.norm() * f32.norm()))          # what the contract itself costs: no kernel in it
        if cos < own_cos[0]:
            own_cos = (cos, name)
        dots = [dots[0] + float((mine * f32).sum()), dots[1] + float((mine * mine).sum()), dots[2] + float((f32 * f32).sum())]
    cos_all = dots[0] / (dots[1] * dots[2]) ** 0.5
    print('%s: logits %.3e, bits rel %.3e, worst gradient tensor %.3e of its largest entry (%s), cosine with the fp32 oracle %.6f overall, '
          'worst tensor %.6f (%s); the emulating oracle itself: worst tensor %.6f (%s)'
          % (what, worst_z, rel_bits, worst_g[0], worst_g[1], cos_all, worst_cos[0], worst_cos[1], own_cos[0], own_cos[1]))
    assert worst_z <= 2e-2 and rel_bits <= 1e-3
    assert worst_g[0] <= 2e-2, worst_g
    assert cos_all >= 0.999 and worst_cos[0] >= 0.99, (cos_all, worst_cos)


@pytest.mark.parametrize('hidden,block_layers', [(16, 1), (16, 3), (32, 1), (32, 3)])
def test_network_matches_the_emulating_oracle(pkg, shell, hidden, block_layers):
    model, sd = _model(hidden, block_layers=block_layers)
    _network_against_the_emulating_oracle(model, sd, shell['scales'], shell['point_num'], 'width %d, block_layers %d' % (hidden, block_layers))


def test_network_on_a_ragged_frame_with_an_empty_scale(pkg, shell):
    """Scales 0 and 2 of the shell fixture around an EMPTY scale: 4983 + 0 + 361 rows, no multiple of any tile.

    The frame is chosen by the oracle alone.  Two evaluations of the contract that differ only at fp32 order - the emulating oracle in
    fp32 and in float64 arithmetic, no kernel involved - must agree well inside the gradient bound, or the bound measures the contract's
    own rounding flips (an activation next to a bf16 rounding boundary or a ReLU input next to zero lands on the other side) instead of
    the kernels.  Here they agree within 1.8e-3 of a tensor's largest entry and their worst per-tensor cosine with the fp32 oracle is
    0.99958.  Random-occupancy clouds as in tests/test_gpu_wide.py's ragged tests do not qualify: the two ORACLES differ by 1.6e-2
    (2049 + 0 + 513 rows), 2.4e-2 / 7.9e-3 (8193 + 0 + 2049 rows, two draws) of a head tensor's largest entry, and at 257 + 0 + 65 rows
    their 8-entry gradient of block_in's conv1_0.bias has cosine 0.96886 with the fp32 oracle's (the kernels measured 0.968862 there, at
    1.4e-4 from the emulating oracle; on the 2049 + 0 + 513 cloud 2.8e-2 from it in inner_mlps.0.0.0.weight, cosines equal to 5
    digits)."""
    model, sd = _model(16, scale_num=3)
    empty = {'coord': np.zeros((0, 3), np.int32), 'occ': np.zeros((0, 8), np.float32), 'offset_tensor': np.zeros((0, 7), np.float32),
             'nbr': np.zeros((0, 27), np.int64)}
    scales = [dict(shell['scales'][0], scale_idx=0), dict(empty, scale_idx=1), dict(shell['scales'][2], scale_idx=2)]
    assert [len(s['coord']) for s in scales] == [4983, 0, 361]
    _network_against_the_emulating_oracle(model, sd, scales, shell['point_num'], 'ragged frame (4983 + 0 + 361 rows), width 16')


# ---- 5. the fused step ---------------------------------------------------------------------------------------------------------------------
def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize('hidden', [16, 32])
def test_train_step_equals_the_tape_path_and_repeats_bitwise(pkg, shell, hidden):
    from linr_pcgc_amd.model_core import FlatAdam, train_step

    def fused(tp='bf16-mul'):
        model, _ = _model(hidden, tp=tp)
        opt = FlatAdam(model)
        bits = train_step(model, opt, model.make_frame(shell['scales']), shell['point_num'])
        torch.cuda.synchronize()
        return model.flat_parameters().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), bits.clone()

    def by_hand():
        model, _ = _model(hidden)
        opt = FlatAdam(model)
        frame = model.make_frame(shell['scales'])
        _, bits, grads = _train_pass(model, frame, 1.0 / float(shell['point_num']))
        with torch.no_grad():
            opt.grad.copy_(grads)
            opt.step(frame)
        return model.flat_parameters().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), bits
    a, b, c = fused(), fused(), by_hand()
    assert bool(torch.isfinite(a[0]).all())
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y), 'two steps from the same state must give the same bits'
        assert torch.equal(x, z), 'train_step must be forward + backward + FlatAdam.step'
    assert not torch.equal(a[3], fused('f32')[3]), "the step must multiply in bf16 (its bits are not the fp32 step's)"


# ---- 6. on-chip state ----------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_leftover_onchip_state(pkg):
    """tests/test_gpu_wide.py::test_wide_results_do_not_depend_on_leftover_onchip_state with the flag set: the new launches sit in the
    wide poison class (linr_debug_poison bit 16)."""
    from linr_pcgc_amd import _lib, overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    gop = overfit.Gop(None, [synthetic.sequence_frame_device('sphere8', 0, 'cuda')], None, 64, 'cuda')
    L = _lib.lib()

    def run(mask, hidden):
        m = overfit.gen_model(gop.scale_num, 'cuda', seed=8807, hidden=hidden)
        m.train_precision = 'bf16-mul'
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
    for hidden in (16, 32):
        clean, dirty = run(0, hidden), run(0x1FFFF, hidden)
        assert bool(torch.isfinite(dirty[0]).all())
        for a, b in zip(clean, dirty):
            assert torch.equal(a, b)


# ---- 7. tracking and losslessness ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gop4(pkg):
    from linr_pcgc_amd import overfit, synthetic
    return overfit.Gop(None, [synthetic.sequence_frame_device('sphere8', t, 'cuda') for t in range(4)], None, 64, 'cuda')


def test_bf16_mul_tracks_fp32(gop4):
    """SURVEY section 8c's criterion (tests/test_gpu_bf16_train.py::test_bf16_tracks_fp32_outside_the_chaotic_regime) at width 16:
    constant lr 1e-3, 3 epochs over a GOP of 4, seeds 8807 / 1 / 2 - every epoch's mean loss within +-1 % of fp32's."""
    from linr_pcgc_amd import overfit
    from linr_pcgc_amd.model_core import FlatAdam
    worst = 0.0
    for seed in (8807, 1, 2):
        losses = {}
        for prec in ('f32', 'bf16-mul'):
            model = overfit.gen_model(gop4.scale_num, 'cuda', seed=seed, hidden=16)
            model.train_precision = prec
            losses[prec] = overfit.overfit_gop(model, FlatAdam(model, lr=1e-3, gamma=1.0), gop4, 3, min_lr=0.0, keep='last')
        ratios = [b / f for b, f in zip(losses['bf16-mul'], losses['f32'])]
        print('seed %d: fp32 %s  bf16-mul %s  ratios %s' % (seed, ['%.4f' % x for x in losses['f32']], ['%.4f' % x for x in losses['bf16-mul']],
                                                             ['%.4f' % x for x in ratios]))
        assert losses['f32'][-1] < losses['f32'][0] and losses['bf16-mul'][-1] < losses['bf16-mul'][0], 'both must be learning'
        assert losses['bf16-mul'] != losses['f32']
        for e, q in enumerate(ratios):
            worst = max(worst, abs(q - 1.0))
            assert abs(q - 1.0) <= 0.01, 'seed %d epoch %d: bf16-mul / fp32 = %.4f (%s)' % (seed, e, q, losses)
    print('worst |bf16-mul / fp32 - 1| over 3 seeds x 3 epochs = %.4f' % worst)


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_gop_codec_files_roundtrip_is_lossless(gop4, tmp_path, precision):
    """The default recipe at 2 epochs with bf16 products, then the codec as ever (its forward never multiplies in bf16)."""
    from linr_pcgc_amd import codec, overfit
    from linr_pcgc_amd.model_core import FlatAdam

    def gen(seed=None):
        return overfit.gen_model(gop4.scale_num, 'cuda', seed=seed, hidden=16)
    model = gen(8807)
    model.train_precision = 'bf16-mul'
    overfit.overfit_gop(model, FlatAdam(model), gop4, 2)
    enc = codec.encode_gop(model, gen(), gop4, 8, precision=precision)
    codec.write_gop(enc, str(tmp_path / 'g'))
    back = codec.read_gop(str(tmp_path / 'g'))
    assert back['side_info']['train_precision'] == 'bf16-mul' and back['side_info'].get('precision', 'f32') == precision
    dec = codec.decode_gop(gen(), back, 'cuda', workers=1)
    for d, info, mn in zip(dec, gop4.infos, gop4.coord_mins):
        assert torch.equal(d, torch.as_tensor(info['ori']).cuda() + torch.tensor(mn, device='cuda', dtype=torch.int32))


def test_cli_end_to_end(tmp_path):
    out = tmp_path / 'run'
    cmd = [sys.executable, '-m', 'linr_pcgc_amd.run', '--config', 'sphere8', '--frames', '4', '--gop', '4', '--first-epoch', '2',
           '--others-epoch', '2', '--hidden-channel-conv', '16', '--train-precision', 'bf16-mul', '--decode', '--out', str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    summary = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert summary['lossless'] is True, summary
    from linr_pcgc_amd import codec
    back = codec.read_gop(str(out / 'result_enc' / sorted(os.listdir(str(out / 'result_enc')))[0]))
    assert back['side_info']['train_precision'] == 'bf16-mul'


# ---- 8. off means off ----------------------------------------------------------------------------------------------------------------------
def test_off_means_off(pkg, monkeypatch):
    """train_precision 'f32': three steps give the parameters and moments of the same steps made with `mul` never passed to the ops."""
    from linr_pcgc_amd import ops, overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    gop = overfit.Gop(None, [synthetic.sequence_frame_device('sphere8', 0, 'cuda')], None, 64, 'cuda')

    def run():
        m = overfit.gen_model(gop.scale_num, 'cuda', seed=8807, hidden=16)
        assert m.train_precision == 'f32'
        o = FlatAdam(m)
        bits = torch.zeros(3, dtype=torch.float64, device='cuda')
        for s in range(3):
            train_step(m, o, gop.frames[0], gop.point_nums[0], out=bits[s:s + 1])
        torch.cuda.synchronize()
        return _sha(m.flat_parameters(), o.exp_avg, o.exp_avg_sq, bits)
    with_option = run()
    seen = []
    for name in ('spconv_wide', 'spconv_wgrad_wide', 'spconv_wgrad_wide2'):
        def strip(*a, _f=getattr(ops, name), **kw):
            seen.append(kw.pop('mul', 'f32'))
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, strip)
    assert run() == with_option
    assert seen and set(seen) == {'f32'}
