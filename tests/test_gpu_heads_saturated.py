"""Every fp32 head and loss kernel on SATURATED logits against the float64 reference of tests/head_ref.py (torch's BCELoss on an fp32
sigmoid, piece by piece: logs clamped at -100 nats, the backward's quotient clamped at 1e-12, p == 1.0f from z ~ 17 on).  An overfitted
network codes at ~0.28 bits / point: most logits of its heads are far from zero, and every kernel below works where those pieces meet.

  op level, through the C-ABI entries (as tests/test_gpu_fused_ops.py::test_head_forward_backward and
  tests/test_gpu_wide.py::test_wide_head_entries_match_torch call them):
    backward on SUPPLIED probabilities   linr_head_bwd, linr_head_wide_bwd (C = 16, 32), linr_bce_bits_bwd
    forward on logits of deviation ~40   linr_head_fwd, linr_head_wide_fwd (C = 16, 32), linr_bce_bits_fwd
  executor level: the width-8 fp32 executor, the wide fp32 executor at 16, the bf16 inference executor and the bf16 training executor on a
  model whose eight output layers are multiplied by 40 and - this file's own factor, because times 40 a fresh model only reaches logits
  of deviation 3.4 - by 400.

Criterion (tests/gpu_common.py): the kernel must be as close to the float64 reference as the fp32 oracle is,
    err_hip(f64) <= max(3 err_oracle32(f64), 1e-4 max|g_tensor|)         bits: |bits - ref64| <= max(3 |oracle32 - ref64|, 1e-5 ref64)
Each test prints its figures (HEADSAT lines) before it asserts.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_ref as hr                                                        # noqa: E402
from gpu_common import _grads_close_per_tensor, _model_and_oracle, _smallest_relu_input          # noqa: E402
from oracle import network as onet                                           # noqa: E402
from oracle import octree as ooct                                            # noqa: E402
from test_gpu_wide import _empty_scale                                       # noqa: E402

pytestmark = pytest.mark.gpu

GSCALE = 0.37
K = 3                            # the occupancy column the op-level tests read (target_ld = 8), the other columns hold 1 - t
ENTRIES = ['head8', 'wide16', 'wide32', 'bce']


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _occ(t):
    """[n, 8] occupancy on the device whose column K is t and whose other columns are its complement (a wrong column or stride shows)"""
    occ = (1.0 - t).view(-1, 1).repeat(1, 8)
    occ[:, K] = t
    return occ.cuda().contiguous()


def _blocks(t):
    """[n, 8 nb] host tensor -> nb device blocks [n, 8] (rows 1.. of [n + 1, 8] buffers whose row 0 is zero)"""
    n, nb = t.shape[0], t.shape[1] // 8
    buf = torch.zeros((nb, n + 1, 8), device='cuda')
    for i in range(nb):
        buf[i, 1:] = t[:, 8 * i:8 * i + 8].cuda()
    return [buf[i, 1:] for i in range(nb)]


def _as_accurate(got, ref64, o32, what):
    """the criterion on one tensor"""
    got, o32 = got.detach().double().cpu().reshape(ref64.shape), o32.double().reshape(ref64.shape)
    gmax = float(ref64.abs().max())
    e_hip, e_o32 = float((got - ref64).abs().max()), float((o32 - ref64).abs().max())
    print('HEADSAT %s: err_hip %.3e err_oracle32 %.3e own max %.3e' % (what, e_hip, e_o32, gmax))
    assert e_hip <= max(3.0 * e_o32, 1e-4 * gmax), '%s vs float64: HIP %.3e, fp32 oracle %.3e (own max %.3e)' % (what, e_hip, e_o32, gmax)


def _rows_as_accurate(got, ref64, o32, what):
    """the criterion row by row: every row of gc against ITS OWN largest entry (the rows' gz span 33 orders of magnitude).  No floor: where
    a row underflows in fp32 (p = 1.18e-38 or the denormal against t = 0: gz ~ 1e-64) the fp32 oracle underflows too and its error is the
    bound."""
    got, o32 = got.detach().double().cpu(), o32.double()
    e_hip, e_o32 = (got - ref64).abs().amax(1), (o32 - ref64).abs().amax(1)
    bound = torch.maximum(3.0 * e_o32, 1e-4 * ref64.abs().amax(1))
    rel = e_hip / ref64.abs().amax(1).clamp(min=1e-300)
    live = ref64.abs().amax(1) > 1e-30
    print('HEADSAT %s: worst row err_hip / own max %.3e (fp32 oracle %.3e)' %
          (what, float(rel[live].max()) if bool(live.any()) else 0.0,
           float((e_o32 / ref64.abs().amax(1).clamp(min=1e-300))[live].max()) if bool(live.any()) else 0.0))
    bad = torch.nonzero(e_hip > bound).reshape(-1)
    assert bad.numel() == 0, '%s: %d rows off, first %d: HIP %.3e, fp32 oracle %.3e, own max %.3e' % (
        what, bad.numel(), int(bad[0]), float(e_hip[bad[0]]), float(e_o32[bad[0]]), float(ref64[bad[0]].abs().max()))


# ---- op level: backward on supplied probabilities -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', hr.NS)
@pytest.mark.parametrize('entry', ENTRIES)
def test_backward_entries_on_supplied_probabilities(pkg, entry, n):
    """linr_head_bwd / linr_head_wide_bwd / linr_bce_bits_bwd on probabilities GIVEN to them: 0, 1, the smallest denormal, 1.18e-38, both
    sides of the 1e-12 switch of (1 - p) p, ordinary values, 1 - 2^-24 and 1 - 1e-3, each against t = 0 and t = 1, at n around the 64-row
    wave tiles and the 256-row blocks.  gc row by row and the 241 (24 C + 49) head gradients tensor by tensor against the float64
    reference, the fp32 oracle being the same formulas in torch float32; rows with p in {0, 1} must give gc == 0 exactly.
    Row n - 1 holds p = 1e-6 against t = 1, |gz| = gscale: the kernels let rows beyond n read row n - 1 and force their gz to 0, and the
    bias gradient gb2 is the plain sum of gz (about -0.6 gscale per 22 rows here, 28 gscale at n = 1025), so a last row counted twice moves
    gb2 by gscale - hundreds of times the bound 1e-4 |gb2| - and gw2 / gb1 / gW1 with it."""
    from linr_pcgc_amd import _lib, ops
    L = _lib.lib()
    p, t = hr.supplied_rows(n)
    occ = _occ(t)
    pd = p.cuda()
    sat = (p == 0) | (p == 1)
    if entry == 'bce':
        gz = ops.bce_bits_bwd(pd, occ[:, K], GSCALE)
        ref, o32 = hr.gz_of(p, t, GSCALE), hr.gz_of(p, t, GSCALE, torch.float32)
        _rows_as_accurate(gz.view(-1, 1), ref.view(-1, 1), o32.view(-1, 1), 'bce n=%d gz' % n)
        assert bool((gz.cpu()[sat] == 0).all())
        return
    C = 8 if entry == 'head8' else int(entry[4:])
    k = hr.raw_case(n, C)                                # the layers and rows of the forward tests, output layer not scaled
    w1, b1, w2, c = k['w1'], k['b1'], k['w2'], (k['c64'].float() if C == 8 else k['c'])
    g = GSCALE / hr.LN2 if C == 8 else GSCALE          # linr_head_bwd's gscale multiplies BITS, the wide entry's (and the loss's) nats
    ref = hr.head_backward(c, p, t, w1, b1, w2, g)
    o32 = hr.head_backward(c, p, t, w1, b1, w2, g, torch.float32)
    d = lambda x: x.cuda().contiguous()
    w1d, b1d, w2d = d(w1), d(b1), d(w2)
    if C == 8:
        cd = d(c)
        gc = torch.full((n, 8), float('nan'), device='cuda')
        gh = torch.full((241,), float('nan'), device='cuda')
        ws = torch.empty(max(L.linr_head_workspace_bytes(n), 16), dtype=torch.uint8, device='cuda')
        _lib.check(L.linr_head_bwd(cd.data_ptr(), pd.data_ptr(), occ.data_ptr() + 4 * K, 8, w1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(),
                                   GSCALE, gc.data_ptr(), n, gh.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), 'linr_head_bwd')
    else:
        cs, gcs = _blocks(c), _blocks(torch.full((n, C), float('nan')))
        gh = torch.full((24 * C + 49,), float('nan'), device='cuda')
        ops.head_wide_bwd([cs], [pd], [occ[:, K]], [w1d], [b1d], [w2d], GSCALE, [gcs], gh)
        gc = torch.cat(gcs, dim=1)
    torch.cuda.synchronize()
    gh = gh.cpu()
    assert bool(torch.isfinite(gc).all()) and bool(torch.isfinite(gh).all())
    _rows_as_accurate(gc, ref['gc'], o32['gc'], '%s n=%d gc' % (entry, n))
    assert bool((gc.cpu()[sat] == 0).all()), 'rows with p in {0, 1} have no gradient at all'
    o = 24 * C
    for name, lo, hi in (('gw1', 0, o), ('gb1', o, o + 24), ('gw2', o + 24, o + 48), ('gb2', o + 48, o + 49)):
        _as_accurate(gh[lo:hi], ref[name], o32[name], '%s n=%d %s' % (entry, n, name))


# ---- op level: forward on logits of standard deviation ~40 -------------------------------------------------------------------------------------
def _check_p(p, k, what, one_from=20.0, atol=1e-4, rtol=1e-4):
    """p == 1.0f where z64 >= 20, p == 0 where z64 <= -110; elsewhere, over p in [1e-35, 1 - 1e-4], the logit recovered from p within the
    project's 1e-4 + 1e-4 |z| of the float64 one (the bf16 executors: from 24 on, within 2e-2 of their emulating oracle's).  No row is
    skipped for being saturated."""
    p, z = p.detach().cpu(), k['z64'].double()
    assert bool((p[z >= one_from] == 1.0).all()) and bool((p[z <= -110] == 0.0).all()), what
    assert bool(((p >= 0) & (p <= 1)).all())
    m = (p >= 1e-35) & (p <= 1.0 - 1e-4)
    pm = p[m].double()
    err = (torch.log(pm) - torch.log1p(-pm) - z[m]).abs()
    tol = atol + rtol * z[m].abs()
    print('HEADSAT %s: %d rows with a recoverable logit, worst |dz| / tol %.3f' % (what, int(m.sum()), float((err / tol).max()) if bool(m.any()) else 0.0))
    assert bool((err <= tol).all()), '%s: recovered logits off by %.3e' % (what, float(err.max()))


def _check_bits(bits, k, what):
    o32 = hr.oracle32_bits(k)
    got, ref = float(bits), k['bits64']
    print('HEADSAT %s: bits %.9g ref64 %.9g err_hip %.3e err_oracle32 %.3e counts %s' % (what, got, ref, abs(got - ref), abs(o32 - ref), k['counts']))
    assert abs(got - ref) <= max(3.0 * abs(o32 - ref), 1e-5 * ref), (what, got, ref, o32)


@pytest.mark.parametrize('n', hr.NS)
@pytest.mark.parametrize('entry', ENTRIES)
def test_forward_entries_on_saturated_logits(pkg, entry, n):
    """linr_head_fwd (with its prune convolution) / linr_head_wide_fwd / linr_bce_bits_fwd on head_ref.saturated_case: the layers of the
    existing head tests with w2 and b2 scaled to logits of deviation ~40, targets by choose_targets (every class drawn at n >= 257: rows
    of exactly 100 nats, contradicted rows on both sides of the backward's switch, agreeing saturated rows of exactly 0 nats).  The
    probabilities, the bits against the float64 reference, and the decoder form (no target) bit for bit."""
    from linr_pcgc_amd import _lib, ops
    L = _lib.lib()
    C = 8 if entry in ('head8', 'bce') else int(entry[4:])
    k = hr.saturated_case(n, C)
    if n >= 257:
        assert all(k['counts'][c] >= 8 for c in hr.CLASSES), k['counts']
    occ = _occ(k['t'])
    d = lambda x: x.cuda().contiguous()
    bits = torch.zeros(1, dtype=torch.float64, device='cuda')
    what = '%s n=%d' % (entry, n)
    if entry == 'bce':
        p, bits = ops.bce_bits_fwd(d(k['z64'].float()), occ[:, K])
        # (the stand-alone loss has no decoder form; its p is a pure function of the fp32 logit)
        _check_p(p, k, what)
        _check_bits(bits, k, what)
        return
    p = torch.full((n,), float('nan'), device='cuda')
    p2 = torch.full((n,), float('nan'), device='cuda')
    w1d, b1d, w2d, b2d = d(k['w1']), d(k['b1']), d(k['w2']), d(k['b2'])
    if C == 8:
        nbr = ops.kmap_build(torch.from_numpy(k['coord']).cuda())
        lo, mask = ops.kmap_compress(nbr)
        buf = torch.zeros((n + 1, 8), device='cuda')
        buf[1:] = k['prior'].cuda()
        prior = buf[1:]
        c_out = torch.empty((n, 8), device='cuda')
        ws = torch.empty(max(L.linr_head_workspace_bytes(n), 16), dtype=torch.uint8, device='cuda')
        Wd, bd = d(k['Wp']), d(k['bp'])
        _lib.check(L.linr_head_fwd(prior.data_ptr(), lo.data_ptr(), mask.data_ptr(), nbr.shape[1], n, Wd.data_ptr(), bd.data_ptr(),
                                   w1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), occ.data_ptr() + 4 * K, 8,
                                   c_out.data_ptr(), p.data_ptr(), bits.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), 'linr_head_fwd')
        _lib.check(L.linr_head_fwd(prior.data_ptr(), lo.data_ptr(), mask.data_ptr(), nbr.shape[1], n, Wd.data_ptr(), bd.data_ptr(),
                                   w1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), None, 0, c_out.data_ptr(), p2.data_ptr(),
                                   None, None, 0, _stream()), 'linr_head_fwd (decoder)')
    else:
        cs = _blocks(k['c'])
        ops.head_wide_fwd(cs, w1d, b1d, w2d, b2d, occ[:, K], p, bits)
        ops.head_wide_fwd(cs, w1d, b1d, w2d, b2d, None, p2)
    torch.cuda.synchronize()
    _check_p(p, k, what)
    assert torch.equal(p, p2), 'the decoder form must give the same probabilities bit for bit'
    _check_bits(bits, k, what)


# ---- executor level -----------------------------------------------------------------------------------------------------------------------------
FACTORS = [40.0, 400.0]


def _saturate(sd, factor):
    """The last layer (weight and bias) of all eight heads times `factor`.  A freshly initialised model has logits of deviation ~0.09:
    times 40 they reach 3.4 - rows in the forbidden band (8, 20), where 1 - p has a few bits left, and none beyond it (asserted: >= 8 band
    rows); times 400, this file's own factor, they reach ~34 and every class of choose_targets is drawn (asserted: >= 8 rows each)."""
    out = {k: v.clone() for k, v in sd.items()}
    for h in range(8):
        for leaf in ('weight', 'bias'):
            out['upsampler.inner_mlps.%d.0.2.%s' % (h, leaf)] *= factor
    return out


def _f64_stage_logits(sd):
    sd64 = {k: v.double() for k, v in sd.items()}

    def logits(sc, k):
        ts = onet.to_torch_scales([sc], torch.float64)[0]
        return onet.cnp_forward(sd64, onet.scale_context(sd64, ts['offset_tensor'], 1), ts['occ'], ts['nbr'], stages=k + 1)[0][k]
    return logits


def _column_by_column(c, rng, band, stage_logits):
    """The occupancy of a cloud for a saturated model: stage k sees only occ[:, :k], so column k is chosen (head_ref.choose_targets) from
    stage k's logits - stage_logits(scale, k): the float64 oracle's, or a bf16 executor's emulating oracle's - once the columns before
    it are fixed.  Eight small CPU passes.  Returns (scale, summed class counts)."""
    n = len(c)
    occ = np.zeros((n, 8), np.float32)
    sc = {'coord': c, 'occ': occ, 'offset_tensor': ooct.offset_tensor(c), 'scale_idx': 1, 'nbr': ooct.neighbour_table(c)}
    total = {}
    with torch.no_grad():
        for k in range(8):
            z = stage_logits(sc, k).reshape(-1).double()
            occ[:, k], counts = hr.choose_targets(z.numpy(), rng, band)
            for name, v in counts.items():
                total[name] = total.get(name, 0) + v
    return sc, total


def _reference_grads(sd, sc, gscale):
    """The float64 oracle UNDER THE REFERENCE'S SEMANTICS: float64 network up to the logits, then head_ref's fp32 p, nats and gz (plain
    float64 autograd would take the true sigmoid loss: 20 nats and gz = 1 where the reference has 100 nats and gz = 0).  Returns (leaves
    with .grad, bits, the float64 logits)."""
    leaves = {k: v.double().clone().requires_grad_() for k, v in sd.items()}
    ts = onet.to_torch_scales([sc], torch.float64)[0]
    logits = onet.forward_scale(leaves, ts)['logits']
    bits, gz = 0.0, []
    for k, z in enumerate(logits):
        p32, t = hr.sigmoid32(z.detach().reshape(-1)), ts['occ'][:, k].float()
        bits += float(hr.bits(p32, t))
        gz.append((hr.gz_of(p32, t, gscale) / hr.LN2).reshape(z.shape))
    torch.autograd.backward(logits, gz)
    return leaves, bits, [z.detach().reshape(-1) for z in logits]


def _saturated_frame(sd, seed, band=hr.BAND, stage_logits=None):
    """one random cloud of 257 rows (redrawn on a ReLU tie at fp32 resolution) with its column-by-column occupancy"""
    stage_logits = stage_logits or _f64_stage_logits(sd)
    for attempt in range(6):
        rng = np.random.default_rng(seed + 1000 * attempt)
        c = ooct.unique_sorted(rng.integers(0, 11, size=(4 * 257, 3)))[:257]
        assert len(c) == 257
        sc, counts = _column_by_column(c, rng, band, stage_logits)
        if _smallest_relu_input(sd, sc) >= 3e-7:
            return sc, counts
    pytest.fail('six clouds in a row with a ReLU tie')


def _check_executor(what, probs, bits, grads, sd, sc, counts, gscale, saturated):
    sd64, bits64, z64 = _reference_grads(sd, sc, gscale)
    sdo = {k: v.clone().requires_grad_() for k, v in sd.items()}
    out32 = onet.forward_scale(sdo, onet.to_torch_scales([sc])[0])
    (out32['bits'] * gscale).backward()
    o32 = float(out32['bits'])
    print('HEADSAT %s: bits %.9g ref64 %.9g err_hip %.3e err_oracle32 %.3e counts %s' % (what, float(bits), bits64, abs(float(bits) - bits64),
                                                                                      abs(o32 - bits64), counts))
    assert counts['band'] >= 8 and (not saturated or all(counts[c] >= 8 for c in hr.CLASSES)), counts
    for k in range(8):
        _check_p(probs[k], {'z64': z64[k]}, '%s stage %d' % (what, k))
    assert abs(float(bits) - bits64) <= max(3.0 * abs(o32 - bits64), 1e-5 * bits64), (float(bits), bits64, o32)
    assert sdo['scale_mlp.0.0.weight'].grad is None          # the zero-row scale
    report = []
    try:
        _grads_close_per_tensor(grads, sdo, sd64=sd64, report=report)
    finally:
        name, e_hip, e_o32, gmax = max(report, key=lambda r: r[1] / r[3] if r[3] > 0 else 0.0)
        print('HEADSAT %s: worst gradient tensor %s err_hip / own max %.3e err_oracle32 / own max %.3e' % (what, name, e_hip / gmax, e_o32 / gmax))


@pytest.mark.parametrize('factor', FACTORS)
def test_fp32_executor_on_a_saturated_model(pkg, factor):
    """The width-8 fp32 executor (linr_head_fwd's kernel inside linr_net_forward, head_bwd.h inside linr_net_backward) on a model whose
    eight output layers are multiplied by 40 and by 400: 257 rows beside a zero-row scale, bits, probabilities and every gradient."""
    from linr_pcgc_amd import engine
    model, sd = _model_and_oracle(pkg, 3)
    sd = _saturate(sd, factor)
    model.load_state_dict(sd)
    sc, counts = _saturated_frame(sd, 257)
    frame = model.make_frame([{k: v for k, v in sc.items() if k != 'nbr'}, _empty_scale(0)])
    assert frame.rows == 257
    flat = model.flat_parameters()
    probs = torch.empty((8, frame.rows), device='cuda')
    bits = torch.zeros(1, dtype=torch.float64, device='cuda')
    engine.net_forward(frame, flat, 0, 8, probs, bits)
    grads = torch.zeros_like(flat)
    gscale = 1.0 / 257
    engine.net_backward(frame, flat, grads, gscale)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grads).all())
    _check_executor('fp32 executor x%d' % factor, probs, bits, grads, sd, sc, counts, gscale, factor >= 400)


@pytest.mark.parametrize('factor', FACTORS)
def test_wide_fp32_executor_on_a_saturated_model(pkg, factor):
    """The same for the channel-blocked fp32 executor at hidden_channel_conv 16 (linr_head_wide_fwd / _bwd through the tape)."""
    from linr_pcgc_amd.model_core import LINR_PCGC_Model
    torch.manual_seed(8807)
    model = LINR_PCGC_Model({'scale_num': 3, 'in_channel': 7, 'hidden_channel_conv': 16, 'block_layers': 1, 'outstage': 8, 'instage': 1})
    sd = _saturate({k: v.detach().clone() for k, v in model.state_dict().items()}, factor)
    model.load_state_dict(sd)
    model = model.cuda()
    sc, counts = _saturated_frame(sd, 258)
    frame = model.make_frame([{k: v for k, v in sc.items() if k != 'nbr'}, _empty_scale(0)])
    assert frame.rows == 257
    probs, bits = model.frame_probs(frame)
    gscale = 1.0 / 257
    model._ensure_grad_views()
    b = torch.zeros(1, dtype=torch.float64, device='cuda')
    with torch.no_grad():
        model._flat_grad.zero_()
        tape = model._wide.forward(frame, 0, 8, None, b, keep=True)
        model._wide.backward(frame, tape, gscale)
    torch.cuda.synchronize()
    assert torch.equal(b, bits)
    _check_executor('wide fp32 executor (16) x%d' % factor, probs, bits, model._flat_grad.clone(), sd, sc, counts, gscale, factor >= 400)


# ---- the bf16 executors against their emulating oracles (oracle/network_bf16.py) ---------------------------------------------------------------------
# Tolerances: those of tests/test_gpu_bf16.py (logits 2e-2, bits 2e-3) and tests/test_gpu_bf16_train.py (logits 2e-2, bits 1e-3, every
# gradient tensor within 2e-2 of its own largest entry); forbidden band (6, 24).  The output layers are multiplied by 40 only: a bf16
# rounding that the summation order flips moves a logit by the output layer's gain, and times 400 that is beyond what 2e-2 can ask of two
# correct evaluations.  The training case reaches the saturated classes through the output BIASES instead (+30 on heads 0-2, -30 on heads
# 3-5: p == 1.0f rows of 100 nats, contradicted rows beyond the 1e-12 switch), which no rounding multiplies.  The inference case needs
# none: the 8-bit weight code spans the whole parameter range (+-27 with the output layers times 40: steps of 0.21), and the de-quantised
# network's logits have a deviation of ~75 by themselves.
def _bf16_checks(what, probs, bits, ref, counts, bits_rtol):
    print('HEADSAT %s: bits %.9g emulating oracle %.9g rel %.3e counts %s' % (what, float(bits), float(ref['bits']),
                                                                            abs(float(bits) - float(ref['bits'])) / float(ref['bits']), counts))
    for k in range(8):
        _check_p(probs[k], {'z64': ref['logits'][k].detach().reshape(-1)}, '%s stage %d' % (what, k), one_from=24.0, atol=2e-2, rtol=0.0)
    assert abs(float(bits) - float(ref['bits'])) <= bits_rtol * float(ref['bits']), (float(bits), float(ref['bits']))


def test_bf16_training_executor_on_a_saturated_model(pkg):
    """csrc/train_bf16.hip (the heads of bf16_common.h going forward, head_bwd.h on bf16 rows going back) against obf.train_forward_scale
    and its autograd: probabilities with no saturated row skipped, bits, every gradient tensor."""
    from linr_pcgc_amd import engine
    from oracle import network_bf16 as obf
    model, sd = _model_and_oracle(pkg, 3)
    sd = _saturate(sd, 40.0)
    for h in range(6):
        sd['upsampler.inner_mlps.%d.0.2.bias' % h] += 30.0 if h < 3 else -30.0
    model.load_state_dict(sd)

    def logits(sc, k):
        return obf.train_forward_scale(sd, onet.to_torch_scales([sc])[0])['logits'][k]
    sc, counts = _saturated_frame(sd, 259, hr.BAND_BF16, logits)
    assert all(counts[c] >= 8 for c in hr.CLASSES) and counts['band'] >= 8, counts
    frame = model.make_frame([{k: v for k, v in sc.items() if k != 'nbr'}, _empty_scale(0)])
    flat = model.flat_parameters()
    probs = torch.empty((8, frame.rows), device='cuda')
    bits = torch.zeros(1, dtype=torch.float64, device='cuda')
    engine.net_forward_train_bf16(frame, flat, probs, bits)
    grads = torch.zeros_like(flat)
    gscale = 1.0 / 257
    engine.net_backward_bf16(frame, flat, grads, gscale)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grads).all())
    sdo = {k: v.clone().requires_grad_() for k, v in sd.items()}
    ref = obf.train_forward_scale(sdo, onet.to_torch_scales([sc])[0])
    (ref['bits'] * gscale).backward()
    _bf16_checks('bf16 training executor', probs, bits, ref, counts, 1e-3)
    off, bad, worst = 0, [], (0.0, '')
    g = grads.cpu().double()
    for name, v in sdo.items():
        m = v.numel()
        want = (v.grad if v.grad is not None else torch.zeros_like(v)).double()
        err, gmax = float((g[off:off + m].view(v.shape) - want).abs().max()), float(want.abs().max())
        if err > 2e-2 * gmax + 1e-9:
            bad.append((name, err, gmax))
        if gmax > 0 and err / gmax > worst[0]:
            worst = (err / gmax, name)
        off += m
    print('HEADSAT bf16 training executor: worst gradient tensor %s err / own max %.3e' % (worst[1], worst[0]))
    assert not bad, 'gradient tensors off by more than 2e-2 of their own max: %s' % bad[:8]


def test_bf16_inference_executor_on_a_saturated_model(pkg):
    """csrc/net_bf16.hip (bf16_common.h's heads on the de-quantised 8-bit weights) against obf.forward_scale: probabilities with no
    saturated row skipped - the rows tests/test_gpu_bf16.py leaves out at |z| >= 12 are compared here - and the bits."""
    from linr_pcgc_amd import overfit
    from linr_pcgc_amd.model_codec import Model_Estimate
    from oracle import network_bf16 as obf
    model, sd0 = _model_and_oracle(pkg, 3)
    model.load_state_dict(_saturate(sd0, 40.0))
    coded = Model_Estimate().compress_model(model, 8, True, overfit.gen_model(3, 'cuda'))['new_model']
    sd = {k: v.detach().cpu().clone() for k, v in coded.state_dict().items()}

    def logits(sc, k):
        return obf.forward_scale(sd, onet.to_torch_scales([sc])[0])['logits'][k]
    sc, counts = _saturated_frame(sd, 260, hr.BAND_BF16, logits)
    assert all(counts[c] >= 8 for c in hr.CLASSES) and counts['band'] >= 8, counts
    frame = coded.make_frame([{k: v for k, v in sc.items() if k != 'nbr'}, _empty_scale(0)])
    probs, bits = coded.frame_probs(frame, precision='bf16')
    with torch.no_grad():
        ref = obf.forward_scale(sd, onet.to_torch_scales([sc])[0])
    z = torch.cat([x.reshape(-1) for x in ref['logits']])
    assert int((z.abs() >= 12).sum()) >= 8, 'rows beyond the |z| < 12 filter of tests/test_gpu_bf16.py must be among those compared'
    _bf16_checks('bf16 inference executor', probs, bits, ref, counts, 2e-3)
