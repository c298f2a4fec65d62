"""GPU tests of the opt-in averaged weights: the kernel (linr_params_average) against its host twin, the overfit that keeps the averages
(overfit.overfit_gop avg_decays=, the Python loop and linr_overfit_gop_avg) against the overfit without them and against a replay,
the rate-checked choice (codec.search_average, codec.encode_gop avg=) against its own objective recomputed through the public API,
round trips through the unchanged decoders, and the drivers.

Everything here is exact.  The update is two individually rounded fp32 operations per element, so kernel and host twin agree bit for
bit; the averaging launch reads the parameters and writes a buffer of its own, so training is what it was; a candidate's bits come from
the codec's deterministic forward on bit-identical weights, so a recomputed objective is the recorded one; streams are bytes.  No rate
gain is asserted on real averages (profiles/avg_ab.txt holds that measurement): the two rate assertions are on planted candidates -
the same model trained twice as long, which must win, and the model under noise of a whole quantiser step, which must lose."""
import filecmp
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_common import _dev                                                            # noqa: E402
from test_params_avg_host import DECAYS, SENTINEL, UPDATES, NS, chain_host, values, weights    # noqa: E402

pytestmark = pytest.mark.gpu

# 2048 workgroups of 256 lanes, a float4 each: above it the grid strides
N_STRIDED = 2048 * 256 * 4 + 1029
CASES = [(n, K, pad) for n in NS for K in (1, 4) for pad in (0, 8)] + [(N_STRIDED, 1, 0), (N_STRIDED, 4, 8)]


def chain_device(n, K, stride, seed=None):
    """test_params_avg_host.chain_host on the kernel: the buffer (padding included) after every update, as host arrays."""
    from linr_pcgc_amd import _lib
    w = weights(K)
    seed = 31 * n + K if seed is None else seed
    avg = torch.full((K, stride), float(SENTINEL), dtype=torch.float32, device=_dev())
    avg[:, :n] = 0.0
    states = []
    for t in range(UPDATES):
        p = torch.from_numpy(values(n, seed + t)).to(_dev())
        _lib.check(_lib.lib().linr_params_average(p.data_ptr(), n, w.ctypes.data, K, stride, avg.data_ptr(), _lib.current_stream_handle()),
                   'linr_params_average')
        states.append(avg.cpu().numpy())
    return states


def _same(a, b):
    """Bit for bit, signed zeros and infinities included; where both hold a NaN it is a NaN in both - the sign and payload of a NaN
    that an operation creates (inf - inf) are the processor's choice, not the arithmetic's (x86 sets the sign bit, gfx950 does not)."""
    if a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return np.array_equal(np.where(both_nan, np.uint32(0), a.view(np.uint32)), np.where(both_nan, np.uint32(0), b.view(np.uint32)))


def test_kernel_equals_host_twin_bitwise(pkg):
    lib = pkg._lib.lib()
    for n, K, pad in CASES:
        stride = ((n + 3) & ~3) + pad
        _, want = chain_host(lib, n, K, stride, 31 * n + K)
        got = chain_device(n, K, stride)
        for t, (g, h) in enumerate(zip(got, want)):
            assert _same(g, h), (n, K, pad, t)                                 # padding included: still the sentinel
        assert np.all(got[-1][:, n:] == SENTINEL)
        if n >= 1023:
            assert np.isnan(got[-1][:, :n]).any(axis=1).all()                  # NaN and inf went into every row


def test_engine_wrapper_and_its_refusals(pkg):
    from linr_pcgc_amd import engine
    lib = pkg._lib.lib()
    n, K = 1025, 3
    w = weights(K)
    p = values(n, 9)
    avg = torch.zeros((K, 1028), dtype=torch.float32, device=_dev())
    engine.params_average(torch.from_numpy(p).to(_dev()), w, avg)
    host = np.zeros((K, 1028), dtype=np.float32)
    engine.params_average_host(p, w, host)
    assert _same(avg.cpu().numpy(), host)
    with pytest.raises(ValueError):
        engine.params_average(torch.from_numpy(p).to(_dev()), w[:2], avg)
    with pytest.raises(pkg._lib.LinrError):
        engine.params_average(torch.from_numpy(p).to(_dev()), w, torch.zeros((K, 1026), dtype=torch.float32, device=_dev()))   # stride % 4
    with pytest.raises(pkg._lib.LinrError):
        engine.params_average(torch.from_numpy(p), w, avg)
    assert lib.linr_params_average(avg.data_ptr(), 0, w.ctypes.data, K, 0, avg.data_ptr(), None) == 0


def test_kernel_under_poison_in_a_child_process(pkg, tmp_path):
    """The same chains with the LDS and the vector registers of every CU filled with a NaN pattern in front of every launch (class 12
    included), in a process of its own: the last state of every case, bit for bit the host twin's."""
    lib = pkg._lib.lib()
    out = str(tmp_path / 'poison.npz')
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), '_params_avg_child.py')
    clean = {k: v for k, v in os.environ.items() if not k.startswith('LINR_')}
    subprocess.run([sys.executable, script, out], check=True, env=dict(clean, LINR_DEBUG_POISON='1'), timeout=600)
    got = np.load(out)
    for n, K, pad in CASES:
        stride = ((n + 3) & ~3) + pad
        assert _same(got['n%d_K%d_p%d' % (n, K, pad)], chain_host(lib, n, K, stride, 31 * n + K)[1][-1]), (n, K, pad)


# ---- the overfit ------------------------------------------------------------------------------------------------------------------
EPOCHS = 4
AVG = (0.5, 0.9)
_gop_cache = {}


def _gop():
    from linr_pcgc_amd import overfit, synthetic
    if 'gop' not in _gop_cache:
        clouds = [synthetic.sphere_shell(7, 40), synthetic.sphere_shell(7, 41)]
        _gop_cache['gop'] = overfit.Gop(None, clouds, None, 64, 'cuda')
    return _gop_cache['gop']


def _fresh(tp, hidden):
    from linr_pcgc_amd import overfit
    from linr_pcgc_amd.model_core import FlatAdam
    model = overfit.gen_model(_gop().scale_num, 'cuda', seed=8807, hidden=hidden)
    model.train_precision = tp
    return model, FlatAdam(model)


def _overfit(tp, hidden, avg_decays, c_loop=False, epochs=EPOCHS):
    from linr_pcgc_amd import overfit
    model, opt = _fresh(tp, hidden)
    info = {}
    losses = overfit.overfit_gop(model, opt, _gop(), epochs, info=info, avg_decays=avg_decays, c_loop=c_loop)
    torch.cuda.synchronize()
    return {'model': model, 'opt': opt, 'info': info, 'losses': losses}


def _same_training(a, b):
    assert a['losses'] == b['losses']
    assert torch.equal(a['model'].flat_parameters().view(torch.int32), b['model'].flat_parameters().view(torch.int32))
    assert torch.equal(a['opt'].exp_avg.view(torch.int32), b['opt'].exp_avg.view(torch.int32))
    assert torch.equal(a['opt'].exp_avg_sq.view(torch.int32), b['opt'].exp_avg_sq.view(torch.int32))
    assert (a['opt'].t, a['opt'].t_scale.tolist(), a['opt'].lr, a['opt'].sched_steps) == (b['opt'].t, b['opt'].t_scale.tolist(), b['opt'].lr, b['opt'].sched_steps)
    assert a['info']['coded_epoch'] == b['info']['coded_epoch'] and a['info']['coded_loss'] == b['info']['coded_loss']


def _replay(tp, hidden):
    """The averages by hand: a train_step loop like overfit_gop's that clones the parameters behind every step, the host twin on the
    clones, the debias scale as one fp32 multiply."""
    from linr_pcgc_amd import overfit
    from linr_pcgc_amd.model_core import train_step
    gop = _gop()
    model, opt = _fresh(tp, hidden)
    if tp == 'bf16':
        gop.share_train_bf16_arena()
    bits = torch.zeros(len(gop), dtype=torch.float64, device='cuda')
    snaps = []
    for _ in range(EPOCHS):
        bits.zero_()
        for j, (f, pn) in enumerate(zip(gop.frames, gop.point_nums)):
            train_step(model, opt, f, pn, out=bits[j:j + 1])
            snaps.append(model.flat_parameters().clone())
        opt.clamp_lr(4e-4)
    n = snaps[0].numel()
    w = overfit.avg_weights(AVG)
    avg = np.zeros((len(AVG), (n + 3) & ~3), dtype=np.float32)
    from linr_pcgc_amd import _lib
    lib = _lib.lib()
    for s in snaps:
        p = s.cpu().numpy()
        assert lib.linr_params_average_host(p.ctypes.data, n, w.ctypes.data, len(AVG), avg.shape[1], avg.ctypes.data) == 0
    return avg[:, :n] * overfit.avg_debias_scales(w, len(snaps))[:, None], len(snaps)


@pytest.mark.parametrize('tp,hidden', [('f32', 8), ('bf16', 8), ('f32', 16)])
def test_training_is_untouched_and_the_averages_match_a_replay(pkg, tp, hidden):
    plain = _overfit(tp, hidden, None)
    with_avg = _overfit(tp, hidden, AVG)
    assert 'averages' not in plain['info'] and 'averages' not in _overfit(tp, hidden, ())['info']
    _same_training(plain, with_avg)
    got = with_avg['info']['averages']
    want, steps = _replay(tp, hidden)
    assert got['decays'] == list(AVG) and got['steps'] == steps == EPOCHS * len(_gop())
    assert got['params'].is_cuda and got['params'].dtype == torch.float32 and tuple(got['params'].shape) == want.shape
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    assert _same(got['params'].cpu().numpy(), np.ascontiguousarray(want))
    # the averages are no copy of the kept parameters
    assert not torch.equal(got['params'][0], with_avg['model'].flat_parameters())


@pytest.mark.parametrize('tp,hidden', [('f32', 8), ('bf16', 8), ('f32', 16)])
def test_c_loop_returns_the_same_averages(pkg, tp, hidden):
    loop = _overfit(tp, hidden, AVG)
    plain_c = _overfit(tp, hidden, None, c_loop=True)
    call = _overfit(tp, hidden, AVG, c_loop=True)
    _same_training(plain_c, call)                                              # the call with averages trains as the call without
    a, b = loop['info']['averages'], call['info']['averages']
    assert a['decays'] == b['decays'] and a['steps'] == b['steps']
    assert torch.equal(a['params'].view(torch.int32), b['params'].view(torch.int32))
    assert torch.equal(loop['model'].flat_parameters().view(torch.int32), call['model'].flat_parameters().view(torch.int32))


def test_overfit_gop_avg_with_null_is_overfit_gop(pkg, monkeypatch):
    """linr_overfit_gop_avg(avg = NULL) in the place of linr_overfit_gop: the same losses, state and counters."""
    L = pkg._lib.lib()
    want = _overfit('f32', 8, None, c_loop=True)
    real, calls = L.linr_overfit_gop_avg, []

    def through_avg(frames, args, result, stream):
        calls.append(1)
        return real(frames, args, None, result, stream)
    monkeypatch.setattr(L, 'linr_overfit_gop', through_avg, raising=False)
    try:
        got = _overfit('f32', 8, None, c_loop=True)
    finally:
        monkeypatch.undo()
    assert calls == [1]
    _same_training(want, got)


def test_gop_avg_refuses_bad_averages_before_any_launch(pkg):
    from linr_pcgc_amd import engine, overfit
    gop = _gop()
    model, opt = _fresh('f32', 8)
    before = model.flat_parameters().clone()
    n = before.numel()
    big = max(gop.frames, key=lambda f: f.rows)
    base = dict(frames=gop.frames, point_nums=gop.point_nums, executor=pkg._lib.LINR_OVERFIT_F32, flat_params=model.flat_parameters(),
                exp_avg=opt.exp_avg, exp_avg_sq=opt.exp_avg_sq, arena=big.arena.data_ptr(), arena_bytes=big.arena.numel(), epochs=1, lr=opt.lr,
                min_lr=4e-4, gamma=opt.gamma, step_size=opt.step_size, step=0, sched_steps=0, scale_steps=opt.t_scale, beta1=0.9, beta2=0.999,
                eps=1e-8, weight_decay=1e-4)
    rows = torch.full((2, (n + 3) & ~3), 7.0, dtype=torch.float32, device='cuda')
    for w, r in (([0.5, 0.0], rows), ([0.5, 1.5], rows), ([0.5, float('nan')], rows), ([0.5, 0.1], rows[:, :n - 4].contiguous()),
                 ([0.5, 0.1], rows.view(-1)[1:1 + 2 * (rows.shape[1] - 4)].view(2, -1))):
        with pytest.raises((pkg._lib.LinrError, ValueError)):
            engine.overfit_gop(avg=(np.asarray(w, np.float32), r), **base)
    torch.cuda.synchronize()
    assert torch.equal(model.flat_parameters(), before) and bool((rows == 7.0).all())          # refused: nothing ran
    assert overfit.AVG_MAX_DECAYS == pkg._lib.LINR_AVG_MAX == 4


# ---- the choice ---------------------------------------------------------------------------------------------------------------------
def _shell(hidden=8):
    from linr_pcgc_amd import overfit
    return overfit.gen_model(_gop().scale_num, 'cuda', hidden=hidden)


@pytest.fixture(scope='module')
def trained(pkg):
    """The GOP's model after 4 epochs (with its real averages), the same model after 8 - the planted better candidate - and the model
    under Gaussian noise of one quantiser step."""
    short = _overfit('f32', 8, AVG)
    longer = _overfit('f32', 8, None, epochs=2 * EPOCHS)
    print('coded loss after %d epochs %.4f, after %d epochs %.4f' % (EPOCHS, short['info']['coded_loss'], 2 * EPOCHS, longer['info']['coded_loss']))
    assert longer['info']['coded_loss'] < 0.97 * short['info']['coded_loss']             # the precondition of "better"
    flat = short['model'].flat_parameters().detach()
    step = float(flat.max() - flat.min()) / 255.0
    gen = torch.Generator().manual_seed(11)
    noisy = flat + (step * torch.randn(flat.numel(), generator=gen)).to(flat.device)
    return {'model': short['model'], 'opt': short['opt'], 'info': short['info'], 'better': longer['model'].flat_parameters().detach().clone(),
            'noisy': noisy}


def _avg(rows, decays):
    return {'decays': list(decays), 'steps': 8, 'params': torch.stack(rows)}


def test_equal_candidates_make_plain_win_and_the_files_are_the_plain_files(trained):
    from linr_pcgc_amd import codec
    gop, model = _gop(), trained['model']
    flat = model.flat_parameters().detach()
    plain = codec.encode_gop(model, _shell(), gop, 8)
    same = codec.encode_gop(model, _shell(), gop, 8, avg=_avg([flat.clone(), flat.clone()], AVG))
    assert 'average' not in plain and 'avg_decay' not in plain['side_info']
    got = same['average']
    assert got['chosen'] == 0 and got['objective_bits'][0] == got['objective_bits'][1] == got['objective_bits'][2]
    assert same['frames'] == plain['frames'] and same['model_bin'] == plain['model_bin'] and same['low_enc_bytes'] == plain['low_enc_bytes']
    assert same['bpp'] == plain['bpp']                                         # the two fields are not counted
    assert same['side_info'] == {**plain['side_info'], 'avg_decay': None, 'avg_candidates': 3}
    # no decay at all: today's call and today's dictionary
    none = codec.encode_gop(model, _shell(), gop, 8, avg={'decays': [], 'steps': 0, 'params': flat.new_zeros((0, flat.numel()))})
    assert 'average' not in none and none['side_info'] == plain['side_info'] and none['frames'] == plain['frames']


def test_noise_loses_the_planted_candidate_wins_and_the_choice_is_honest(trained):
    """Candidates: the model under noise of one quantiser step (must lose to the plain model), the same GOP trained 4 more epochs
    (must win).  The recorded objective of every candidate, recomputed through the public API: compress_params, _fill into a fresh
    shell, frame_probs on the evaluated frames, laplace_bits_est from the codes.  The training model and its checkpoint are only read."""
    from linr_pcgc_amd import codec, overfit
    from linr_pcgc_amd.model_codec import Model_Estimate, compress_params, laplace_bits_est
    gop, model, opt = _gop(), trained['model'], trained['opt']
    flat0 = model.flat_parameters().detach().clone()
    ck0 = overfit.checkpoint(model, opt, trained['info']['coded_epoch'], trained['info']['coded_loss'])
    enc = codec.encode_gop(model, _shell(), gop, 8, avg=_avg([trained['noisy'], trained['better']], AVG), avg_frames=0)
    got = enc['average']
    print('objective bits: plain %.1f, noisy %.1f, trained longer %.1f; chosen %d' % (*got['objective_bits'], got['chosen']))
    assert got['decays'] == list(AVG) and got['frames'] == [0, 1] and got['search_s'] > 0
    assert got['objective_bits'][1] > got['objective_bits'][0]                 # noise of a quantiser step loses
    assert got['chosen'] == 2 and got['objective_bits'][2] < got['objective_bits'][0]
    assert enc['side_info']['avg_decay'] == AVG[1] and enc['side_info']['avg_candidates'] == 3
    only_noise = codec.search_average(model, _shell(), gop, torch.stack([trained['noisy']]), AVG[:1], 8, 'f32', 0)
    assert only_noise['chosen'] == 0
    n = flat0.numel()
    want = []
    for v in (flat0, trained['noisy'], trained['better']):
        out = compress_params(v, 8)
        cand = Model_Estimate._fill(_shell(), out['recon_ret'], out['symbols'], out['min_param'], out['max_param'], 8)
        bits = float(torch.stack([cand.frame_probs(f)[1] for f in gop.frames]).sum())
        dev = int(np.abs(out['symbols'].astype(np.int64) - int(out['mu'])).sum())
        want.append(laplace_bits_est(n, dev, 8) + 1.0 * bits)
    assert got['objective_bits'] == want
    # what was coded is the winner through the model codec
    best = compress_params(trained['better'], 8)
    assert enc['model_bin'] == best['final_bytes']
    assert (enc['side_info']['min_param'], enc['side_info']['max_param']) == (best['min_param'], best['max_param'])
    # the training model, its optimiser and hence the checkpoint: as before
    assert torch.equal(model.flat_parameters().view(torch.int32), flat0.view(torch.int32))
    ck1 = overfit.checkpoint(model, opt, trained['info']['coded_epoch'], trained['info']['coded_loss'])
    assert list(ck0['model']) == list(ck1['model']) and all(torch.equal(ck0['model'][k], ck1['model'][k]) for k in ck0['model'])
    s0, s1 = ck0['optimizer_state_dict'], ck1['optimizer_state_dict']
    assert s0['param_groups'] == s1['param_groups'] and list(s0['state']) == list(s1['state'])
    for k in s0['state']:
        for key, v in s0['state'][k].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(s1['state'][k][key])), (k, key)


def test_a_non_finite_average_never_wins(trained):
    from linr_pcgc_amd import codec
    model = trained['model']
    bad = trained['better'].clone()
    bad[17] = float('nan')
    inf = trained['better'].clone()
    inf[5] = float('-inf')
    got = codec.search_average(model, _shell(), _gop(), torch.stack([bad, inf]), AVG, 8, 'f32', 0)
    assert got['chosen'] == 0 and got['objective_bits'][1:] == [None, None] and got['objective_bits'][0] > 0


def _lossless(codec, gop, enc, **kw):
    dec = codec.decode_gop(_shell(), enc, 'cuda', **kw)
    assert len(dec) == len(gop.frames)
    for i, d in enumerate(dec):
        ref = torch.as_tensor(gop.infos[i]['ori']).cuda() + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32)
        assert torch.equal(d, ref), i


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_round_trip_through_the_unchanged_decoders(trained, tmp_path, precision):
    from linr_pcgc_amd import codec
    gop, model = _gop(), trained['model']
    enc = codec.encode_gop(model, _shell(), gop, 8, precision=precision, avg=_avg([trained['better']], AVG[:1]))
    assert enc['average']['chosen'] == 1                                       # an average, chosen on purpose
    codec.write_gop(enc, str(tmp_path / 'enc'))
    side = json.load(open(str(tmp_path / 'enc' / 'side_info.json')))
    assert side['avg_decay'] == AVG[0] and side['avg_candidates'] == 2 and side.get('precision', 'f32') == precision
    back = codec.read_gop(str(tmp_path / 'enc'))
    _lossless(codec, gop, back)
    _lossless(codec, gop, back, lockstep=2)


def test_the_range_search_runs_on_the_winner(trained):
    from linr_pcgc_amd import codec
    from linr_pcgc_amd.model_codec import candidate_ranges
    gop, model = _gop(), trained['model']
    enc = codec.encode_gop(model, _shell(), gop, 8, avg=_avg([trained['better']], AVG[:1]), qrange_search=True, qrange_trims=(0, 1, 2))
    assert enc['average']['chosen'] == 1
    kept, ranges = candidate_ranges(trained['better'].cpu(), (0, 1, 2))
    assert enc['qrange']['trims'] == kept
    assert (enc['side_info']['min_param'], enc['side_info']['max_param']) == ranges[kept.index(enc['qrange']['chosen'])]
    _lossless(codec, gop, enc)
    # ... and everything behind the choice is the unchanged encoder, whichever way the streams are coded
    ref = codec.encode_gop(model, _shell(), gop, 8, avg=_avg([trained['better']], AVG[:1]))
    for kw in ({'device_codes': True}, {'device_coder': True, 'coder_group': 2}, {'digests': True}, {'stream_chunk': 64}):
        other = codec.encode_gop(model, _shell(), gop, 8, avg=_avg([trained['better']], AVG[:1]), **kw)
        assert other['average']['chosen'] == 1 and other['model_bin'] == ref['model_bin']
        assert other['average']['objective_bits'] == ref['average']['objective_bits']
        if 'stream_chunk' not in kw:
            assert other['frames'] == ref['frames']
        _lossless(codec, gop, other)


# ---- the drivers --------------------------------------------------------------------------------------------------------------------
def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_run_with_averages_serial_pipelined_and_one_call(pkg, tmp_path):
    """run.py --avg-decays 0.5,0.9 --decode on a 2-GOP sequence: lossless, 'average' in every result, the two fields in every
    side_info.json, the same files with --pipeline and with --c-overfit, and the decoder program rebuilds the frames in another
    process from the files alone."""
    from linr_pcgc_amd import run
    outs = []
    for name, flag in (('serial', []), ('pipe', ['--pipeline']), ('call', ['--c-overfit'])):
        out = str(tmp_path / name)
        args = run.parse(['--config', 'sphere8', '--frames', '4', '--gop', '2', '--first-epoch', '3', '--others-epoch', '2', '--avg-decays', '0.5,0.9',
                          '--decode', '--out', out] + flag)
        summary, results = run.run_sequence_job(args, 0, 1, None)
        assert summary['lossless'] is True and summary['gops'] == 2 and sorted(results) == [0, 1]
        for g, r in results.items():
            a = r['average']
            assert a['decays'] == [0.5, 0.9] and a['chosen'] in (0, 1, 2) and len(a['objective_bits']) == 3 and a['frames'] == [0, 1]
            assert a['objective_bits'][a['chosen']] == min(a['objective_bits'])
            side = json.load(open(os.path.join(out, 'result_enc', r['gop'], 'side_info.json')))
            assert side['avg_candidates'] == 3 and side['avg_decay'] == ([None, 0.5, 0.9][a['chosen']])
            json.dumps(r)                                                      # what results_rank0.json is written from
        outs.append(os.path.join(out, 'result_enc'))
    names = _tree(outs[0])
    assert len(names) > 6
    for other in outs[1:]:
        assert names == _tree(other)
        for n in names:
            assert filecmp.cmp(os.path.join(outs[0], n), os.path.join(other, n), shallow=False), (other, n)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
    done = subprocess.run([sys.executable, '-m', 'linr_pcgc_amd.decoder', '--enc-dir', outs[0], '--dec-dir', str(tmp_path / 'dec')],
                          cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    assert 'decoded 4 frames of 2 GOPs' in done.stdout
