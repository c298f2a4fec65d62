"""The bf16 / uint8-weight inference executor of the wide models (hidden_channel_conv 16 / 32, csrc/wide_bf16.hip,
WideNet.forward_bf16): against the width-generic emulation of its numerics (tests/wide_bf16_ref.py), against the fp32 wide path on the
same de-quantised model, staged = one-shot, lossless through model.encode / decode, the codec files and the CLI, independent of leftover
state, on tiny and ragged frames; and the emulation itself against the shipped width-8 executor."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wide_bf16_ref as wref                 # noqa: E402
from oracle import network as onet           # noqa: E402
from oracle import octree as ooct            # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(16, 1), (16, 2), (32, 1), (32, 3)]


def _trained_quantised(shell, hidden, block_layers, steps=6):
    """a wide model a few Adam steps away from its initialisation, pushed through the model codec at bitdepth 8: (coded model with
    its codes, its de-quantised fp32 state dict on the CPU)"""
    from linr_pcgc_amd import overfit
    from linr_pcgc_amd.model_codec import Model_Estimate
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    model = overfit.gen_model(5, 'cuda', seed=8807, block_layers=block_layers, hidden=hidden)
    frame = model.make_frame(shell['scales'])
    opt = FlatAdam(model)
    for _ in range(steps):
        train_step(model, opt, frame, shell['point_num'])
    coded = Model_Estimate().compress_model(model, 8, True, overfit.gen_model(5, 'cuda', block_layers=block_layers,
                                                                               hidden=hidden))['new_model']
    sd = {k: v.detach().cpu().clone() for k, v in coded.state_dict().items()}
    return coded, sd


def _logits(p):
    p = p.double()
    return torch.log(p) - torch.log1p(-p)


def _emu(sd, s):
    return wref.forward_scale(sd, onet.to_torch_scales([s])[0])


@pytest.fixture(scope='module')
def models(shell):
    from linr_pcgc_amd import _lib
    _lib.lib()
    return {c: _trained_quantised(shell, *c) for c in CASES}


@pytest.mark.parametrize('hidden,block_layers', CASES)
def test_wide_bf16_against_emulation_and_fp32(shell, models, hidden, block_layers):
    coded, sd = models[(hidden, block_layers)]
    worst_e, worst_f, worst_be, worst_bf = 0.0, 0.0, 0.0, 0.0
    # the width-8 bounds at width 16; at width 32 the bf16 roundings of 32-term sums and stored rows widen the gap to
    # fp32 (measured 0.109 at block_layers 1, while the same run stays within 1e-3 of the emulation): 1.5e-1 / 2e-1
    tol_f = {16: (5e-2, 1e-1), 32: (1.5e-1, 2e-1)}[hidden][0 if block_layers == 1 else 1]
    for s in shell['scales']:
        frame = coded.make_frame([s])
        p, bits = coded.frame_probs(frame, precision='bf16')
        p32, bits32 = coded.frame_probs(frame, precision='f32')
        with torch.no_grad():
            ref = _emu(sd, s)
        for k in range(8):
            z = _logits(p[k]).cpu()
            ze = ref['logits'][k].view(-1).double()
            keep = ze.abs() < 12
            worst_e = max(worst_e, float((z - ze).abs()[keep].max()) if bool(keep.any()) else 0.0)
            z32 = _logits(p32[k]).cpu()
            keep = z32.abs() < 12
            worst_f = max(worst_f, float((z - z32).abs()[keep].max()) if bool(keep.any()) else 0.0)
        worst_be = max(worst_be, abs(float(bits) - float(ref['bits'])) / float(ref['bits']))
        worst_bf = max(worst_bf, abs(float(bits) - float(bits32)) / float(bits32))
    print('hidden %d block_layers %d: logits |d| vs emulation %.3g, vs fp32 %.3g; bits rel. vs emulation %.3g, vs fp32 %.3g'
          % (hidden, block_layers, worst_e, worst_f, worst_be, worst_bf))
    assert worst_e <= 2e-2 and worst_be <= 2e-3
    assert worst_f <= tol_f and worst_bf <= 1e-2


@pytest.mark.parametrize('hidden,block_layers', CASES)
def test_wide_bf16_deterministic_staged_and_lossless(shell, models, hidden, block_layers):
    coded, _ = models[(hidden, block_layers)]
    frame = coded.make_frame(shell['scales'])
    one, bits = coded.frame_probs(frame, precision='bf16')
    two, bits2 = coded.frame_probs(frame, precision='bf16')
    assert torch.equal(one, two) and torch.equal(bits, bits2)
    staged = torch.empty_like(one)
    for k in range(8):
        coded._stage_forward(frame, k, k + 1, staged, None, 'bf16')
    assert torch.equal(one, staged), 'the stage-serial decoder must reproduce the encoder bit for bit'
    coded.inference_precision = 'bf16'
    try:
        for s in shell['scales'][:2]:
            d = {'coord': torch.tensor(s['coord'], device='cuda'), 'offset_tensor': torch.tensor(s['offset_tensor'], device='cuda'),
                 'occ_lst': [torch.tensor(s['occ'][:, i:i + 1], device='cuda') for i in range(8)], 'scale_idx': s['scale_idx']}
            enc = coded.encode(d)
            dec = coded.decode({'enc_bytes': enc['enc_bytes'], 'coord': d['coord'], 'offset_tensor': None, 'scale_idx': s['scale_idx']})
            assert torch.equal(torch.cat(dec, dim=1).cpu(), torch.tensor(s['occ']))
    finally:
        coded.inference_precision = 'f32'


@pytest.mark.parametrize('hidden', [16, 32])
def test_wide_bf16_gop_codec_files_roundtrip(tmp_path, hidden):
    from linr_pcgc_amd import codec, overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam
    clouds = [synthetic.sequence_frame_device('sphere8', t, 'cuda') for t in range(2)]
    gop = overfit.Gop(None, clouds, None, 64, 'cuda')

    def gen(seed=None):
        return overfit.gen_model(gop.scale_num, 'cuda', seed=seed, hidden=hidden)
    model = gen(8807)
    overfit.overfit_gop(model, FlatAdam(model), gop, 2)
    enc = codec.encode_gop(model, gen(), gop, 8, precision='bf16')
    assert enc['side_info']['precision'] == 'bf16'
    codec.write_gop(enc, str(tmp_path / 'g'))
    back = codec.read_gop(str(tmp_path / 'g'))
    assert back['side_info']['precision'] == 'bf16' and back['side_info']['hidden_channel_conv'] == hidden
    dec = codec.decode_gop(gen(), back, 'cuda', workers=1)
    for d, info, mn in zip(dec, gop.infos, gop.coord_mins):
        assert torch.equal(d, torch.as_tensor(info['ori']).cuda() + torch.tensor(mn, device='cuda', dtype=torch.int32))


def test_wide_bf16_cli_end_to_end(tmp_path):
    """The command that used to throw its training away: --precision bf16 --hidden-channel-conv 16 trains in fp32, codes with the
    bf16 executor and decodes losslessly."""
    out = tmp_path / 'run'
    cmd = [sys.executable, '-m', 'linr_pcgc_amd.run', '--config', 'sphere8', '--frames', '2', '--gop', '2', '--first-epoch', '2',
           '--others-epoch', '2', '--precision', 'bf16', '--hidden-channel-conv', '16', '--decode', '--out', str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert (out / 'result_enc').is_dir()
    import json
    summary = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert summary['lossless'] is True, summary


def test_wide_bf16_ignores_leftover_state(shell, models):
    """Under linr_debug_poison and with the executor's parameter copy, weight images and activation pool filled with 0xFF bytes,
    probabilities and bits are those of a clean run."""
    from linr_pcgc_amd import _lib
    for key in ((16, 2), (32, 1)):
        coded, _ = models[key]
        frame = coded.make_frame(shell['scales'])
        p0, b0 = coded.frame_probs(frame, precision='bf16')
        st = coded._wide._bf
        st['pf'].view(torch.int32).fill_(-1)
        st['img'].fill_(0xFF)
        for b in st['pool'].bufs.values():
            b[:, 1:].fill_(-1)
        L = _lib.lib()
        L.linr_debug_poison(0xFFFFFF)
        try:
            import ctypes
            L.linr_debug_poison_now(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            p1, b1 = coded.frame_probs(frame, precision='bf16')
            torch.cuda.synchronize()
        finally:
            L.linr_debug_poison(0)
        assert torch.equal(p0, p1) and torch.equal(b0, b1)


# the model (16, 2) keeps the ids it had when it was the only one ('1', '2', ...); (32, 1) and (32, 3) are named in theirs
RAGGED_NS = [1, 2, 63, 64, 65, 255, 256, 257, 1025]
RAGGED = [pytest.param(m, n, id=str(n) if m == (16, 2) else '%dx%d-%d' % (m[0], m[1], n)) for m in [(16, 2), (32, 1), (32, 3)] for n in RAGGED_NS]


@pytest.mark.parametrize('model,n', RAGGED)
def test_wide_bf16_tiny_and_ragged_frames(models, model, n):
    coded, sd = models[model]
    rng = np.random.default_rng(n)
    side = 8 if n <= 257 else 16                 # 512 cells hold the sizes up to 257; 1025 rows need the 16-cube
    c = ooct.unique_sorted(rng.integers(0, side, size=(4 * n, 3)))[:n]
    assert len(c) == n
    sc = {'coord': c, 'occ': (rng.random((n, 8)) < 0.5).astype(np.float32), 'offset_tensor': ooct.offset_tensor(c), 'scale_idx': 1}
    frame = coded.make_frame([sc, {'coord': np.zeros((0, 3), np.int32), 'occ': np.zeros((0, 8), np.float32),
                                   'offset_tensor': np.zeros((0, 7), np.float32), 'scale_idx': 0}])
    one, bits = coded.frame_probs(frame, precision='bf16')
    staged = torch.empty_like(one)
    for k in range(8):
        coded._stage_forward(frame, k, k + 1, staged, None, 'bf16')
    assert torch.equal(one, staged)
    sc = dict(sc, nbr=ooct.neighbour_table(c))
    with torch.no_grad():
        ref = _emu(sd, sc)
    assert abs(float(bits) - float(ref['bits'])) <= 2e-3 * float(ref['bits']) + 1e-3
    for k in range(8):
        ze = ref['logits'][k].view(-1).double()
        d = (_logits(one[k]).cpu() - ze).abs()[ze.abs() < 12]
        assert d.numel() == 0 or float(d.max()) <= 2e-2, (k, float(d.max()))
    coded.inference_precision = 'bf16'
    try:
        d = {'coord': torch.tensor(c, device='cuda'), 'offset_tensor': torch.tensor(sc['offset_tensor'], device='cuda'),
             'occ_lst': [torch.tensor(sc['occ'][:, i:i + 1], device='cuda') for i in range(8)], 'scale_idx': 1}
        enc = coded.encode(d)
        dec = coded.decode({'enc_bytes': enc['enc_bytes'], 'coord': d['coord'], 'offset_tensor': None, 'scale_idx': 1})
        assert torch.equal(torch.cat(dec, dim=1).cpu(), torch.tensor(sc['occ']))
    finally:
        coded.inference_precision = 'f32'


def test_emulation_tracks_the_shipped_width8_executor(shell):
    """The generic emulation at width 8 against engine.net_forward_bf16 (the width-8 executor, unchanged) on a trained, quantised
    model: logits within the same 2e-2."""
    coded, sd = _trained_quantised(shell, 8, 1)
    worst = 0.0
    for s in shell['scales']:
        frame = coded.make_frame([s])
        p, _ = coded.frame_probs(frame, precision='bf16')
        with torch.no_grad():
            ref = _emu(sd, s)
        for k in range(8):
            ze = ref['logits'][k].view(-1).double()
            d = (_logits(p[k]).cpu() - ze).abs()[ze.abs() < 12]
            if d.numel():
                worst = max(worst, float(d.max()))
    print('width 8: logits |d| of the shipped executor vs the generic emulation %.3g' % worst)
    assert worst <= 2e-2
