"""The training step of hidden_channel_conv 16 / 32 as one C call (csrc/wide_train.hip: linr_net_train_step_wide and its split entries)
against the Python schedule of the same commit (WideNet.forward(keep=True) / backward / FlatAdam.step, which tests/test_gpu_wide*.py
hold to the oracle and to float64).  The C schedule issues the same launches with the same arguments, so every comparison here is
torch.equal: parameters, Adam's moments, bits, gradients.  The loss scale crosses the C-ABI as a float; where a test hands a scale to
the Python schedule itself it hands it the same float."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from oracle import octree as ooct                                       # noqa: E402
from gpu_common import ADAM_DEFAULT, ADAM_DISTINCT, ADAM_DISTINCT_GSCALE_DIV, _close       # noqa: E402
from test_fake_quant_host import fake_quant_host                        # noqa: E402

pytestmark = pytest.mark.gpu

CONFIGS = [(16, 1), (16, 2), (32, 1), (32, 3)]
PRECISIONS = ['f32', 'bf16-mul']


def _model(hidden, scale_num=5, block_layers=1, seed=8807, precision='f32', c_step=True):
    from linr_pcgc_amd.model_core import LINR_PCGC_Model
    torch.manual_seed(seed)
    model = LINR_PCGC_Model({'scale_num': scale_num, 'in_channel': 7, 'hidden_channel_conv': hidden, 'block_layers': block_layers,
                             'outstage': 8, 'instage': 1}).cuda()
    model.train_precision = precision
    model._wide.c_step = c_step
    return model


def _f32(x):
    return float(np.float32(x))


def _steps(model, opt, frame, point_num, n, **kw):
    from linr_pcgc_amd.model_core import train_step
    bits = torch.zeros(n, dtype=torch.float64, device='cuda')
    for s in range(n):
        train_step(model, opt, frame, point_num, out=bits[s:s + 1], **kw)
    torch.cuda.synchronize()
    return bits


def _same_state(a, oa, b, ob, what=''):
    assert bool(torch.isfinite(a.flat_parameters()).all()), what
    assert torch.equal(a.flat_parameters(), b.flat_parameters()), 'parameters ' + what
    assert torch.equal(oa.exp_avg, ob.exp_avg), 'exp_avg ' + what
    assert torch.equal(oa.exp_avg_sq, ob.exp_avg_sq), 'exp_avg_sq ' + what
    assert oa.t == ob.t and np.array_equal(oa.t_scale, ob.t_scale) and oa.lr == ob.lr, what


def _mul(model):
    return 'bf16' if model.train_precision == 'bf16-mul' else 'f32'


def _tape_grads(model, frame, gscale):
    """d (gscale * bits) / d params and the bits through the Python executor's own tape."""
    model._ensure_grad_views()
    b = torch.zeros(1, dtype=torch.float64, device='cuda')
    with torch.no_grad():
        model._flat_grad.zero_()
        tape = model._wide.forward(frame, 0, 8, None, b, keep=True)
        model._wide.backward(frame, tape, gscale)
    return model._flat_grad.clone(), b


def _arena(frame, hidden, block_layers, fill=None):
    from linr_pcgc_amd import _lib
    need = int(_lib.lib().linr_net_wide_train_arena_bytes(frame.rows, hidden, block_layers))
    assert need > 0
    a = torch.empty(need + 64, dtype=torch.uint8, device='cuda')
    if fill is not None:
        a.fill_(fill)
    return a


def _c_grads(frame, params, hidden, block_layers, mul, gscale, arena=None):
    """linr_net_forward_train_wide, then linr_net_backward_wide into a NaN-filled gradient."""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    arena = _arena(frame, hidden, block_layers) if arena is None else arena
    base = (arena.data_ptr() + 63) & ~63
    nbytes = arena.numel() - (base - arena.data_ptr())
    flags = _lib.LINR_MUL_BF16 if mul == 'bf16' else 0
    bits = torch.zeros(1, dtype=torch.float64, device='cuda')
    g = torch.full_like(params, float('nan'))
    s = _lib.current_stream_handle()
    _lib.check(L.linr_net_forward_train_wide(frame.cref(), params.data_ptr(), hidden, base, nbytes, flags, bits.data_ptr(), s), 'forward')
    _lib.check(L.linr_net_backward_wide(frame.cref(), params.data_ptr(), hidden, base, nbytes, flags, gscale, g.data_ptr(), s), 'backward')
    return g, bits


# ---- 1. step equals step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('hidden,block_layers', CONFIGS)
def test_c_step_equals_the_python_schedule(pkg, shell, hidden, block_layers, precision):
    from linr_pcgc_amd.model_core import FlatAdam
    out = []
    for c_step in (False, True):
        m = _model(hidden, block_layers=block_layers, precision=precision, c_step=c_step)
        o = FlatAdam(m)
        start = m.flat_parameters().clone()
        bits = _steps(m, o, m.make_frame(shell['scales']), shell['point_num'], 3)
        assert not torch.equal(start, m.flat_parameters())
        out.append((m, o, bits))
    (a, oa, ba), (b, ob, bb) = out
    assert float(ba[0]) > 0 and torch.equal(ba, bb), (ba, bb)
    _same_state(a, oa, b, ob)
    assert ob.t == 3 and ob.sched_steps == 3 and oa.sched_steps == 3


# ---- 2. the split entries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hidden,block_layers,precision', [(16, 2, 'f32'), (32, 1, 'bf16-mul'), (32, 3, 'f32'), (16, 1, 'bf16-mul')])
def test_split_entries_equal_the_python_tape(pkg, shell, hidden, block_layers, precision):
    m = _model(hidden, block_layers=block_layers, precision=precision)
    frame = m.make_frame(shell['scales'])
    gscale = _f32(1.0 / shell['point_num'])
    want, want_bits = _tape_grads(m, frame, gscale)
    arena = _arena(frame, hidden, block_layers)
    g1, b1 = _c_grads(frame, m.flat_parameters(), hidden, block_layers, _mul(m), gscale, arena)
    g2, b2 = _c_grads(frame, m.flat_parameters(), hidden, block_layers, _mul(m), gscale, arena)          # the same arena again
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0          # every element of the NaN-filled gradient was written
    assert torch.equal(g1, want) and torch.equal(b1, want_bits)
    assert torch.equal(g2, g1) and torch.equal(b2, b1)


# ---- 3. ragged and tiny frames, scales that come and go ------------------------------------------------------------------------------
def _empty_scale(idx):
    return {'coord': np.zeros((0, 3), np.int32), 'occ': np.zeros((0, 8), np.float32), 'offset_tensor': np.zeros((0, 7), np.float32),
            'scale_idx': idx}


def _cloud(n, idx, seed, side=None):
    """n distinct voxels of a box at ~1/3 occupancy, cut as tests/test_gpu_wide.py::test_wide_tiny_and_ragged_frames cuts them."""
    side = max(6, int(round((3 * n) ** (1 / 3))) + 2) if side is None else side
    rng = np.random.default_rng(seed)
    c = ooct.unique_sorted(rng.integers(0, side, size=(4 * n, 3)))[:n]
    assert len(c) == n
    return {'coord': c, 'occ': (rng.random((n, 8)) < 0.5).astype(np.float32), 'offset_tensor': ooct.offset_tensor(c), 'scale_idx': idx}


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 1025])
@pytest.mark.parametrize('hidden,block_layers', [(16, 2), (32, 1)])
def test_c_step_on_tiny_and_ragged_frames(pkg, hidden, block_layers, n):
    from linr_pcgc_amd.model_core import FlatAdam
    scales = [_cloud(n, 1, n + hidden), _empty_scale(0)]
    out = []
    for c_step in (False, True):
        m = _model(hidden, scale_num=3, block_layers=block_layers, c_step=c_step)
        o = FlatAdam(m)
        frame = m.make_frame(scales)
        assert frame.rows == n
        out.append((m, o, _steps(m, o, frame, 8 * n, 2)))
    (a, oa, ba), (b, ob, bb) = out
    assert torch.equal(ba, bb) and float(bb[0]) > 0
    _same_state(a, oa, b, ob)
    assert list(ob.t_scale) == [0, 2, 0]


@pytest.mark.parametrize('hidden,block_layers', [(16, 2), (32, 1)])
def test_c_step_skips_then_starts_the_mlp_of_an_empty_scale(pkg, hidden, block_layers):
    """A three-scale frame whose middle scale has no rows for 2 steps, then a frame that contains it: scale 1's context MLP is left
    alone (no weight decay, no moments), then starts with its own step count - exactly as on the Python schedule."""
    from linr_pcgc_amd.model_core import FlatAdam
    s0, s1, s2 = _cloud(257, 0, 70, side=9), _cloud(33, 1, 71, side=9), _cloud(65, 2, 72, side=9)
    out = []
    for c_step in (False, True):
        m = _model(hidden, scale_num=3, block_layers=block_layers, c_step=c_step)
        o = FlatAdam(m)
        mlp1 = [p for name, p in m.named_parameters() if name.startswith('scale_mlp.1.')]
        before = [p.detach().clone() for p in mlp1]
        gap = m.make_frame([s0, _empty_scale(1), s2])
        assert gap.rows == 322 and gap.n_scales == 3
        bits = [_steps(m, o, gap, 2000, 2)]
        assert list(o.t_scale) == [2, 0, 2]
        assert all(torch.equal(p, q) for p, q in zip(mlp1, before)), 'the MLP of a scale that never had a gradient was touched'
        mid = [(m.flat_parameters().clone(), o.exp_avg.clone(), o.exp_avg_sq.clone())]
        bits.append(_steps(m, o, m.make_frame([s0, s1, s2]), 2200, 2))
        assert list(o.t_scale) == [4, 2, 4] and o.t == 4
        assert not any(torch.equal(p, q) for p, q in zip(mlp1, before))
        bits.append(_steps(m, o, gap, 2000, 1))          # a started scale goes on with a zero gradient
        assert list(o.t_scale) == [5, 3, 5]
        out.append((m, o, torch.cat(bits), mid))
    (a, oa, ba, ma), (b, ob, bb, mb) = out
    assert torch.equal(ba, bb)
    assert all(torch.equal(x, y) for x, y in zip(ma[0], mb[0]))
    _same_state(a, oa, b, ob)


# ---- 4. Adam's arguments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hidden,block_layers,precision', [(16, 1, 'f32'), (32, 3, 'bf16-mul')])
def test_c_step_passes_distinct_adam_arguments(pkg, shell, hidden, block_layers, precision):
    """Pairwise distinct, non-default lr, betas, eps, weight_decay, gscale, step 7 and unequal per-scale counts: a field of
    linr_step_args that is dropped or swapped with a neighbour changes the C step alone."""
    from linr_pcgc_amd import engine
    from linr_pcgc_amd.model_core import FlatAdam
    adam = ADAM_DISTINCT
    m = _model(hidden, block_layers=block_layers, precision=precision, c_step=False)
    frame = m.make_frame(shell['scales'])
    opt = FlatAdam(m, **adam)
    _steps(m, opt, frame, shell['point_num'], 2)          # moments to start from
    M, m0, v0 = m.flat_parameters().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    gscale = _f32(1.0 / (ADAM_DISTINCT_GSCALE_DIV * shell['point_num']))
    counts = np.asarray([7, 5, 3, 6, 2], dtype=np.int64)
    # the C step from (M, m0, v0)
    p, ea, es = M.clone(), m0.clone(), v0.clone()
    bits_c = torch.zeros(1, dtype=torch.float64, device='cuda')
    engine.net_train_step_wide(frame, p, hidden, _arena(frame, hidden, block_layers), ea, es, gscale, 7, adam['lr'], adam['betas'][0],
                               adam['betas'][1], adam['eps'], adam['weight_decay'], bits_c, mul=_mul(m), scale_steps=counts)
    # the Python schedule from the same state, its counters one short of those
    opt.t, opt.t_scale = 6, counts - 1
    g, bits_p = _tape_grads(m, frame, gscale)
    opt.grad.copy_(g)
    opt.step(frame)
    assert opt.t == 7 and np.array_equal(opt.t_scale, counts)
    assert torch.equal(bits_c, bits_p)
    assert torch.equal(p, m.flat_parameters()) and torch.equal(ea, opt.exp_avg) and torch.equal(es, opt.exp_avg_sq)
    assert not torch.equal(p, M)
    # ... and each argument matters: the default in its place gives another result
    for name, value in (('lr', 0.01), ('b1', 0.9), ('b2', 0.999), ('eps', 1e-8), ('wd', 1e-4), ('gscale', _f32(1.0 / shell['point_num'])),
                        ('step', 3), ('counts', None)):
        kw = dict(lr=adam['lr'], b1=adam['betas'][0], b2=adam['betas'][1], eps=adam['eps'], wd=adam['weight_decay'], gscale=gscale, step=7,
                  counts=counts)
        kw[name] = value
        q, qa, qs = M.clone(), m0.clone(), v0.clone()
        engine.net_train_step_wide(frame, q, hidden, _arena(frame, hidden, block_layers), qa, qs, kw['gscale'], kw['step'], kw['lr'], kw['b1'],
                                   kw['b2'], kw['eps'], kw['wd'], torch.zeros_like(bits_c), mul=_mul(m), scale_steps=kw['counts'])
        assert not torch.equal(q, p), name


# ---- 5. the quantisation-aware step -------------------------------------------------------------------------------------------------------
def _adam64(M, g, m, v, t, wd, adam):
    """torch.optim.Adam's update in float64."""
    LR, (B1, B2), EPS = adam['lr'], adam['betas'], adam['eps']
    M, g, m, v = M.double(), g.double(), m.double(), v.double()
    g = g + wd * M
    m = B1 * m + (1 - B1) * g
    v = B2 * v + (1 - B2) * g * g
    denom = v.sqrt() / (1 - B2 ** t) ** 0.5 + EPS
    return M - LR / (1 - B1 ** t) * m / denom


@pytest.mark.parametrize('bitdepth', [8, 4])
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('hidden,block_layers', [(16, 1), (32, 2)])
def test_qat_step_is_the_plain_step_at_the_quantised_weights(pkg, shell, hidden, block_layers, precision, bitdepth):
    """tests/test_gpu_qat.py's identities of the width-8 steps for linr_net_train_step_wide: with weight_decay 0 a step with qparams on the
    master M is the plain step started at Q = fake_quant(M) in bits and moments, bit for bit; qparams is the host quantiser's image of
    M; with weight decay M lands where forward + backward at Q followed by FlatAdam.step on M puts it, bit for bit."""
    from linr_pcgc_amd import _lib, engine
    from linr_pcgc_amd.model_core import FlatAdam
    adam = ADAM_DEFAULT
    model = _model(hidden, block_layers=block_layers, precision=precision)
    frame = model.make_frame(shell['scales'])
    opt = FlatAdam(model, **adam)
    _steps(model, opt, frame, shell['point_num'], 2)          # plain steps: moments and counters to start from
    M, m0, v0 = model.flat_parameters().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    t, ts = opt.advance(frame)
    assert t == 3
    gscale = _f32(1.0 / shell['point_num'])
    arena = _arena(frame, hidden, block_layers)

    def run(start, wd, **qat):
        p, m, v = start.clone(), m0.clone(), v0.clone()
        bits = torch.zeros(1, dtype=torch.float64, device='cuda')
        engine.net_train_step_wide(frame, p, hidden, arena, m, v, gscale, t, adam['lr'], *adam['betas'], adam['eps'], wd, bits,
                                   mul=_mul(model), scale_steps=ts, **qat)
        return p, m, v, bits

    qbuf = torch.full_like(M, float('nan'))
    pa, ma, va, bits_a = run(M, 0.0, qparams=qbuf, bitdepth=bitdepth)
    hq, _, _ = fake_quant_host(_lib.lib(), M.cpu().numpy(), bitdepth)
    Q = torch.from_numpy(hq).cuda()
    assert torch.equal(qbuf, Q) and not torch.equal(Q, M)          # far above 65,536 parameters: the kernel's re-reading path
    assert M.numel() > 65536
    pb, mb, vb, bits_b = run(Q, 0.0)
    assert torch.equal(bits_a, bits_b) and float(bits_a) > 0
    assert torch.equal(ma, mb) and torch.equal(va, vb)
    assert not torch.equal(pa, pb)                          # ... while the update lands on the master, not on Q
    # the optimiser's weight decay acts on the master
    WD = adam['weight_decay']
    g, bits_g = _c_grads(frame, Q, hidden, block_layers, _mul(model), gscale, arena)
    pw, mw, vw, bits_w = run(M, WD, qparams=qbuf, bitdepth=bitdepth)
    assert torch.equal(bits_w, bits_a) and torch.equal(bits_g, bits_a)
    _close(pw, _adam64(M, g, m0, v0, t, WD, adam), 2e-6, 2e-7, 'master after a quantisation-aware step')
    # bit for bit the unfused path: FlatAdam.step on the master with the gradient at Q - the model and opt still hold M, m0, v0
    assert torch.equal(model.flat_parameters(), M)
    opt.grad.copy_(g)
    opt.step(frame)
    assert torch.equal(model.flat_parameters(), pw), 'fused quantisation-aware step and forward + backward at Q + FlatAdam.step differ'
    assert torch.equal(opt.exp_avg, mw) and torch.equal(opt.exp_avg_sq, vw)


def test_qat_train_step_surface(pkg, shell):
    """train_step(qat_bitdepth=) on a wide model: the one-call step (opt-in) takes it, the Python schedule refuses it before anything runs."""
    from linr_pcgc_amd import _lib
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    m = _model(16)
    frame = m.make_frame(shell['scales'])
    o = FlatAdam(m)
    plain = _steps(m, o, frame, shell['point_num'], 1)
    aware = _steps(m, o, frame, shell['point_num'], 1, qat_bitdepth=8)
    assert o.t == 2 and float(aware[0]) > 0 and float(aware[0]) != float(plain[0])
    m._wide.c_step = False
    before = m.flat_parameters().clone()
    with pytest.raises(_lib.LinrError, match='quantisation-aware training exists for hidden_channel_conv=8 only'):
        train_step(m, o, frame, shell['point_num'], qat_bitdepth=8)
    assert o.t == 2 and torch.equal(before, m.flat_parameters())


# ---- 6. nothing read that was not written ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
def test_c_step_does_not_depend_on_what_the_arena_held(pkg, shell, precision):
    from linr_pcgc_amd import engine
    hidden, block_layers = 32, 3
    model = _model(hidden, block_layers=block_layers, precision=precision)
    frame = model.make_frame(shell['scales'])
    M = model.flat_parameters().clone()
    gscale = _f32(1.0 / shell['point_num'])
    out = []
    for fill in (0xFF, 0x00):
        arena = _arena(frame, hidden, block_layers, fill)
        p, m, v = M.clone(), torch.zeros_like(M), torch.zeros_like(M)
        bits = torch.zeros(2, dtype=torch.float64, device='cuda')
        for s in range(2):
            engine.net_train_step_wide(frame, p, hidden, arena, m, v, gscale, s + 1, 0.01, 0.9, 0.999, 1e-8, 1e-4, bits[s:s + 1], mul=_mul(model))
        g, b = _c_grads(frame, p, hidden, block_layers, _mul(model), gscale, _arena(frame, hidden, block_layers, fill))
        out.append((p, m, v, bits, g, b))
    assert bool(torch.isfinite(out[0][0]).all()) and bool(torch.isfinite(out[0][4]).all())
    for x, y in zip(*out):
        assert torch.equal(x, y)


# ---- 7. no shared state ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def two_frames(pkg):
    from linr_pcgc_amd import overfit, synthetic
    gop = overfit.Gop(None, [synthetic.sequence_frame_device('sphere8', t, 'cuda') for t in (0, 1)], None, 64, 'cuda')
    assert gop.frames[0].rows != gop.frames[1].rows
    return gop


def _pair(gop):
    from linr_pcgc_amd import overfit
    from linr_pcgc_amd.model_core import FlatAdam
    A = overfit.gen_model(gop.scale_num, 'cuda', seed=8807, hidden=16)
    A.train_precision = 'bf16-mul'
    B = overfit.gen_model(gop.scale_num, 'cuda', seed=4242, hidden=32)
    A._wide.c_step = B._wide.c_step = True
    return (A, FlatAdam(A)), (B, FlatAdam(B))


def _snapshot(m, o, bits):
    return m.flat_parameters().clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), bits.clone()


def test_c_steps_of_two_models_interleave(pkg, two_frames):
    from linr_pcgc_amd.model_core import train_step
    gop = two_frames
    (A, oa), (B, ob) = _pair(gop)
    apart = [_snapshot(m, o, _steps(m, o, gop.frames[i], gop.point_nums[i], 2)) for i, (m, o) in enumerate(((A, oa), (B, ob)))]
    (A, oa), (B, ob) = _pair(gop)
    bits = torch.zeros((2, 2), dtype=torch.float64, device='cuda')
    for s in range(2):
        for i, (m, o) in enumerate(((A, oa), (B, ob))):
            train_step(m, o, gop.frames[i], gop.point_nums[i], out=bits[i, s:s + 1])
    torch.cuda.synchronize()
    for i, (m, o) in enumerate(((A, oa), (B, ob))):
        for x, y in zip(apart[i], _snapshot(m, o, bits[i])):
            assert torch.equal(x, y), i


def test_c_steps_from_two_threads_on_two_streams(pkg, two_frames):
    """One process, two Python threads, a HIP stream each, 3 steps each: the library keeps no state, the arena is the model's."""
    gop = two_frames
    (A, oa), (B, ob) = _pair(gop)
    apart = [_snapshot(m, o, _steps(m, o, gop.frames[i], gop.point_nums[i], 3)) for i, (m, o) in enumerate(((A, oa), (B, ob)))]
    pairs = _pair(gop)
    bits = [torch.zeros(3, dtype=torch.float64, device='cuda') for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    errors = []
    torch.cuda.synchronize()

    def work(i):
        from linr_pcgc_amd.model_core import train_step
        try:
            m, o = pairs[i]
            with torch.cuda.stream(streams[i]):
                for s in range(3):
                    train_step(m, o, gop.frames[i], gop.point_nums[i], out=bits[i][s:s + 1])
            streams[i].synchronize()
        except Exception as e:          # noqa: BLE001 - reported on the main thread
            errors.append((i, repr(e)))
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for i, (m, o) in enumerate(pairs):
        for x, y in zip(apart[i], _snapshot(m, o, bits[i])):
            assert torch.equal(x, y), i


# ---- 8. end to end ------------------------------------------------------------------------------------------------------------------------------
def _files(d):
    out = {}
    for root, _, names in os.walk(d):
        for n in names:
            out[os.path.relpath(os.path.join(root, n), d)] = open(os.path.join(root, n), 'rb').read()
    return out


def test_overfit_encode_decode_with_the_c_step(pkg, two_frames, tmp_path):
    from linr_pcgc_amd import codec, overfit
    from linr_pcgc_amd.model_core import FlatAdam
    gop = two_frames

    def run(c_step, name, **kw):
        model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807, hidden=16)
        model._wide.c_step = c_step
        info = {}
        losses = overfit.overfit_gop(model, FlatAdam(model), gop, 2, info=info, **kw)
        enc = codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda', hidden=16), gop, 8)
        codec.write_gop(enc, str(tmp_path / name))
        return losses, info

    # quantisation-aware: the last of 2 epochs, then the codec round trip through files
    losses, info = run(True, 'qat', qat_epochs=1)
    assert info['qat_from'] == 1 and all(np.isfinite(losses))
    dec = codec.decode_gop(overfit.gen_model(gop.scale_num, 'cuda', hidden=16), codec.read_gop(str(tmp_path / 'qat')), 'cuda', workers=1)
    for i in range(2):
        ref = torch.as_tensor(gop.infos[i]['ori']).cuda() + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32)
        assert torch.equal(dec[i], ref), i
    # the plain overfit writes the same files on either schedule
    l_c, _ = run(True, 'c', qat_epochs=0)
    l_py, _ = run(False, 'py', qat_epochs=0)
    assert l_c == l_py and l_c[:1] == losses[:1] and l_c[1:] != losses[1:]
    fc, fp = _files(str(tmp_path / 'c')), _files(str(tmp_path / 'py'))
    assert fc and sorted(fc) == sorted(fp)
    for name in fc:
        assert fc[name] == fp[name], name


def test_run_with_qat_epochs_at_width_16_in_a_child_process(pkg, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env['LINR_WIDE_C_STEP'] = '1'          # the one-call step is opt-in; quantisation-aware epochs at this width need it
    done = subprocess.run([sys.executable, '-m', 'linr_pcgc_amd.run', '--config', 'sphere8', '--hidden-channel-conv', '16', '--qat-epochs', '1',
                           '--frames', '2', '--gop', '2', '--first-epoch', '2', '--others-epoch', '2', '--decode', '--out', str(tmp_path / 'seq')],
                          cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    summary = json.loads(done.stdout.strip().splitlines()[-1])
    assert summary['lossless'] is True
    side = json.load(open(str(tmp_path / 'seq' / 'result_enc' / 'gop_0_1' / 'side_info.json')))
    assert side['qat_epochs'] == 1
