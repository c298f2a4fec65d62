"""GPU tests of the opt-in quantisation-aware overfit: the device quantiser (linr_params_fake_quant) against its host twin, the two
train steps with linr_step_args.qparams (linr_net_train_step, linr_net_train_step_bf16) against the plain steps they are built from, one oracle
anchor, and the drivers (overfit_gop qat_epochs=, run.py --qat-epochs, the stand-alone decoder).

What is exact here and why: the quantiser is six individually rounded fp32 operations behind an exact min / max, so host and device
agree bit for bit; a quantisation-aware step runs the kernels of the plain step on the weights Q = fake_quant(M), so its bits and -
with weight_decay 0, where the moments see the gradient alone - its Adam moments are those of a plain step started at Q.  No rate
threshold is asserted: on shells of this size the rate is noise (profiles/qat_ab.txt holds the measurement)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import network as onet                                      # noqa: E402
from gpu_common import _dev, _close, _model_and_oracle                  # noqa: E402
from gpu_common import ADAM_DEFAULT, ADAM_DISTINCT, ADAM_DISTINCT_GSCALE_DIV       # noqa: E402
from test_fake_quant_host import SCALES, fake_quant_host, planted      # noqa: E402

pytestmark = pytest.mark.gpu

# 65,536 floats is what the kernel's one workgroup holds in registers: at and below it params is read once, above it twice
NS = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4097, 65535, 65536, 65537, 70001)
B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 0.01


def _device_quant(p, bitdepth):
    from linr_pcgc_amd import engine
    q, c, mm = engine.params_fake_quant(torch.from_numpy(p).to(_dev()), bitdepth, codes=True)
    return q.cpu().numpy(), c.cpu().numpy(), mm.cpu().numpy()


def _same_as_host(lib, p, bitdepth):
    p = np.ascontiguousarray(p, dtype=np.float32)
    hq, hc, hmm = fake_quant_host(lib, p, bitdepth)
    dq, dc, dmm = _device_quant(p, bitdepth)
    assert np.array_equal(dq.view(np.uint32), hq.view(np.uint32))
    assert np.array_equal(dc, hc)
    assert np.array_equal(dmm.view(np.uint32), hmm.view(np.uint32))
    return dq, dc, dmm


@pytest.mark.parametrize('bitdepth', [4, 8, 12])
def test_device_quantiser_equals_host_bitwise(pkg, golden_dir, bitdepth):
    from linr_pcgc_amd import _lib
    lib = _lib.lib()
    flat = np.load(os.path.join(golden_dir, 'loot_model_kat.npz'))['flat'].astype(np.float32)
    first = _same_as_host(lib, flat, bitdepth)
    again = _device_quant(flat, bitdepth)                       # called twice: identical output
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(first, again))
    for i, n in enumerate(NS):
        _same_as_host(lib, planted(n, SCALES[i % len(SCALES)], bitdepth, 31 * n + bitdepth), bitdepth)
    # the defined edge cases: a constant vector (codes 0, the parameters themselves), NaN (stays NaN, code 0, no part in min / max)
    q, c, mm = _same_as_host(lib, np.full(1025, 0.25, dtype=np.float32), bitdepth)
    assert np.all(q == 0.25) and not c.any() and mm.tolist() == [0.25, 0.25]
    p = planted(5000, 1.0, bitdepth, 5)
    p[[7, 4099]] = np.nan
    q, c, mm = _same_as_host(lib, p, bitdepth)
    assert np.isnan(q[[7, 4099]]).all() and not c[[7, 4099]].any() and not np.isnan(mm).any() and int(c.max()) == 2 ** bitdepth - 1


def test_device_quantiser_without_optional_outputs(pkg):
    from linr_pcgc_amd import _lib, engine
    p = torch.from_numpy(planted(3001, 0.05, 8, 1)).to(_dev())
    q0, c0, _ = engine.params_fake_quant(p, 8, codes=True)
    q1 = torch.full_like(p, 7.0)
    _lib.check(_lib.lib().linr_params_fake_quant(p.data_ptr(), p.numel(), 8, q1.data_ptr(), None, None, _lib.current_stream_handle()), 'quant')
    assert torch.equal(q0, q1) and int(c0.cpu().numpy().max()) == 255


def _adam64(M, g, m, v, t, wd, adam):
    """torch.optim.Adam's update in float64."""
    LR, (B1, B2), EPS = adam['lr'], adam['betas'], adam['eps']
    M, g, m, v = M.double(), g.double(), m.double(), v.double()
    g = g + wd * M
    m = B1 * m + (1 - B1) * g
    v = B2 * v + (1 - B2) * g * g
    denom = v.sqrt() / (1 - B2 ** t) ** 0.5 + EPS
    return M - LR / (1 - B1 ** t) * m / denom


def _step_identity(model, frame, point_num, step_fn, fwd_bwd, adam=ADAM_DEFAULT):
    """step_fn(params, exp_avg, exp_avg_sq, t, t_scale, weight_decay, bits, **qat): one train step of the executor under test with
    Adam's other arguments from `adam`; fwd_bwd(params, grads): its forward and backward at `params`, the gradient of
    bits / point_num added into grads."""
    from linr_pcgc_amd import engine
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    opt = FlatAdam(model, **adam)
    WD = adam['weight_decay']
    for _ in range(2):
        train_step(model, opt, frame, point_num)          # plain steps: moments and counters to start from
    M, m0, v0 = model.flat_parameters().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    t, ts = opt.advance(frame)
    assert t == 3
    Q, _ = engine.params_fake_quant(M, 8)
    assert not torch.equal(Q, M)

    def run(start, wd, **qat):
        p, m, v = start.clone(), m0.clone(), v0.clone()
        bits = torch.zeros(1, dtype=torch.float64, device=p.device)
        step_fn(p, m, v, t, ts, wd, bits, **qat)
        return p, m, v, bits

    # weight_decay 0: the moments depend on the gradient alone, and that is the gradient at Q
    qbuf = torch.full_like(M, float('nan'))
    pa, ma, va, bits_a = run(M, 0.0, qparams=qbuf, bitdepth=8)
    pb, mb, vb, bits_b = run(Q, 0.0)
    assert torch.equal(qbuf, Q)
    assert torch.equal(bits_a, bits_b) and float(bits_a) > 0
    assert torch.equal(ma, mb) and torch.equal(va, vb)
    assert not torch.equal(pa, pb)                          # ... while the update lands on the master, not on Q
    # the optimiser's weight decay acts on the master: Adam's formula in float64 on (M, g at Q)
    g = torch.zeros_like(M)
    fwd_bwd(Q, g)
    pw, mw, vw, bits_w = run(M, WD, qparams=qbuf, bitdepth=8)
    assert torch.equal(bits_w, bits_a)
    _close(pw, _adam64(M, g, m0, v0, t, WD, adam), 2e-6, 2e-7, 'master after a quantisation-aware step')
    _close(pa, _adam64(M, g, m0, v0, t, 0.0, adam), 2e-6, 2e-7, 'master after a quantisation-aware step, no weight decay')
    # and bit for bit the unfused path: the forward and backward entries at Q, then FlatAdam.step (linr_adam_step, positional
    # scalars) on the master with that gradient - the model and opt still hold M, m0, v0
    opt.grad.copy_(g)
    opt.step(frame)
    assert torch.equal(model.flat_parameters(), pw), 'fused quantisation-aware step and forward + backward at Q + FlatAdam.step differ'
    assert torch.equal(opt.exp_avg, mw) and torch.equal(opt.exp_avg_sq, vw)
    return Q, float(bits_a)


@pytest.mark.parametrize('block_layers', [1, 3])
def test_fp32_qat_step_is_the_plain_step_at_the_quantised_weights(pkg, shell, block_layers):
    _fp32_qat_step(pkg, shell, block_layers, ADAM_DEFAULT, 1.0)


def test_fp32_qat_step_passes_distinct_adam_arguments(pkg, shell):
    _fp32_qat_step(pkg, shell, 1, ADAM_DISTINCT, ADAM_DISTINCT_GSCALE_DIV)


def _fp32_qat_step(pkg, shell, block_layers, adam, gscale_div):
    from linr_pcgc_amd import engine
    model, sd = _model_and_oracle(pkg, 5, block_layers=block_layers)
    frame = model.make_frame(shell['scales'])
    point_num = gscale_div * shell['point_num']
    gscale = 1.0 / point_num

    def step_fn(p, m, v, t, ts, wd, bits, **qat):
        engine.net_train_step(frame, p, m, v, gscale, t, adam['lr'], *adam['betas'], adam['eps'], wd, bits, scale_steps=ts, **qat)

    def fwd_bwd(p, g):
        engine.net_forward(frame, p, 0, 8, None, None)
        engine.net_backward(frame, p, g, gscale)

    Q, bits = _step_identity(model, frame, point_num, step_fn, fwd_bwd, adam)
    if block_layers == 1:
        # the oracle anchor: the bits of the step are those of the network with the state dict filled with Q
        sdq, off, qc = {}, 0, Q.cpu()
        for k, v in sd.items():
            sdq[k] = qc[off:off + v.numel()].view(v.shape).clone()
            off += v.numel()
        assert off == qc.numel()
        with torch.no_grad():
            ref = float(onet.frame_bits(sdq, onet.to_torch_scales(shell['scales'])))
        assert abs(bits - ref) <= 3e-4 * ref, (bits, ref)


def test_bf16_qat_step_is_the_plain_step_at_the_quantised_weights(pkg, shell):
    _bf16_qat_step(pkg, shell, ADAM_DEFAULT, 1.0)


def test_bf16_qat_step_passes_distinct_adam_arguments(pkg, shell):
    _bf16_qat_step(pkg, shell, ADAM_DISTINCT, ADAM_DISTINCT_GSCALE_DIV)


def _bf16_qat_step(pkg, shell, adam, gscale_div):
    from linr_pcgc_amd import engine
    model, _ = _model_and_oracle(pkg, 5)
    model.train_precision = 'bf16'
    frame = model.make_frame(shell['scales'])
    point_num = gscale_div * shell['point_num']
    gscale = 1.0 / point_num

    def step_fn(p, m, v, t, ts, wd, bits, **qat):
        engine.net_train_step_bf16(frame, p, m, v, gscale, t, adam['lr'], *adam['betas'], adam['eps'], wd, bits, scale_steps=ts, **qat)

    def fwd_bwd(p, g):
        engine.net_forward_train_bf16(frame, p, None, None)
        engine.net_backward_bf16(frame, p, g, gscale)

    _step_identity(model, frame, point_num, step_fn, fwd_bwd, adam)


def test_qat_step_refuses_bad_arguments(pkg, shell):
    from linr_pcgc_amd import _lib, engine
    model, _ = _model_and_oracle(pkg, 5)
    frame = model.make_frame(shell['scales'])
    p = model.flat_parameters()
    m, v, bits = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(1, dtype=torch.float64, device=p.device)
    before = p.clone()
    for qparams, depth in ((p, 8), (torch.empty_like(p), 1), (torch.empty_like(p), 17), (torch.empty(p.numel() + 1, device=p.device)[1:], 8)):
        with pytest.raises(_lib.LinrError):
            engine.net_train_step(frame, p, m, v, 1.0, 1, LR, B1, B2, EPS, 0.0, bits, qparams=qparams, bitdepth=depth)
        with pytest.raises(_lib.LinrError):
            engine.net_train_step_bf16(frame, p, m, v, 1.0, 1, LR, B1, B2, EPS, 0.0, bits, qparams=qparams, bitdepth=depth)
    assert torch.equal(p, before) and float(bits) == 0.0 and not m.any()          # refused before any launch


def test_wide_models_are_refused(pkg, shell):
    from linr_pcgc_amd import _lib
    from linr_pcgc_amd.model_core import FlatAdam, LINR_PCGC_Model, train_step
    model = LINR_PCGC_Model({'scale_num': 5, 'in_channel': 7, 'hidden_channel_conv': 16, 'block_layers': 1, 'outstage': 8,
                             'instage': 1}).cuda()
    frame = model.make_frame(shell['scales'])
    with pytest.raises(_lib.LinrError, match='quantisation-aware training exists for hidden_channel_conv=8 only'):
        train_step(model, FlatAdam(model), frame, shell['point_num'], qat_bitdepth=8)


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_overfit_gop_with_quantisation_aware_epochs(pkg, tmp_path, precision):
    from linr_pcgc_amd import codec, overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam
    clouds = [synthetic.sphere_shell(7, 40), synthetic.sphere_shell(7, 41)]

    def run(**kw):
        gop = overfit.Gop(None, clouds, None, 64, 'cuda')
        model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807)
        model.train_precision = precision
        info = {}
        losses = overfit.overfit_gop(model, FlatAdam(model), gop, 4, keep='best', info=info, **kw)
        return gop, model, losses, info

    def streams(gop, model):
        enc = codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda'), gop, 8, precision=precision)
        return enc, ([bytes(b) for f in enc['frames'] for b in f], enc['model_bin'], enc['low_enc_bytes'], enc['side_info'])

    gop0, plain, l_plain, i_plain = run()
    gop1, zero, l_zero, i_zero = run(qat_epochs=0)
    assert l_zero == l_plain and i_zero == i_plain and 'qat_from' not in i_plain
    assert torch.equal(zero.flat_parameters(), plain.flat_parameters())
    assert streams(gop1, zero)[1] == streams(gop0, plain)[1]

    gop, model, losses, info = run(qat_epochs=2)
    assert losses[:2] == l_plain[:2] and losses[2:] != l_plain[2:]
    assert info['qat_from'] == 2 and info['coded_epoch'] in (2, 3) and info['coded_loss'] == losses[info['coded_epoch']]
    model.qat_epochs = 2                                    # what run.py sets for side_info.json
    enc, _ = streams(gop, model)
    codec.write_gop(enc, str(tmp_path / 'enc'))
    side = json.load(open(str(tmp_path / 'enc' / 'side_info.json')))
    assert side['qat_epochs'] == 2 and side['train_precision'] == precision
    dec = codec.decode_gop(overfit.gen_model(gop.scale_num, 'cuda'), codec.read_gop(str(tmp_path / 'enc')), 'cuda')
    for i, d in enumerate(dec):
        ref = torch.as_tensor(gop.infos[i]['ori']).cuda() + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32)
        assert torch.equal(d, ref), i
    # more quantisation-aware epochs than epochs: all of them are
    _, _, l_all, i_all = run(qat_epochs=9)
    assert i_all['qat_from'] == 0 and l_all[0] != l_plain[0]


def test_run_with_qat_epochs_is_lossless_and_decodes_in_another_process(pkg, tmp_path):
    from linr_pcgc_amd import run
    out = str(tmp_path / 'seq')
    args = run.parse(['--config', 'sphere8', '--frames', '4', '--gop', '2', '--first-epoch', '3', '--others-epoch', '2', '--qat-epochs', '1',
                      '--decode', '--out', out])
    summary, results = run.run_sequence_job(args, 0, 1, None)
    assert summary['lossless'] is True
    assert results[0]['qat_from'] == 2 and results[1]['qat_from'] == 1 and results[0]['coded_epoch'] == 2 and results[1]['coded_epoch'] == 1
    side = json.load(open(os.path.join(out, 'result_enc', 'gop_0_1', 'side_info.json')))
    assert side['qat_epochs'] == 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
    done = subprocess.run([sys.executable, '-m', 'linr_pcgc_amd.decoder', '--enc-dir', os.path.join(out, 'result_enc'), '--dec-dir',
                           str(tmp_path / 'dec')], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    assert 'decoded 4 frames of 2 GOPs' in done.stdout
