"""The overfit of a whole GOP as one C call (csrc/overfit.hip: linr_overfit_gop; overfit.overfit_gop(c_loop=True); run.py --c-overfit)
against the Python loop on the same inputs.  The call makes the loop's launches with the loop's host doubles, so parameters, both
moments, every counter, the learning rate and the kept epoch are compared with torch.equal / ==.  The epoch losses are the same
n_frames non-negative doubles summed in frame order instead of torch's reduction order: each sum is within n u of the exact sum
(u = 2^-53), so two orders differ by at most 2 n u relative, and the one division by n_frames that follows adds half an ulp on either
side, 2^-52 together - the bound LOSS_REL below.  Every case first asserts, from the Python loop's own losses, that the two smallest
competing losses are further apart than that, so the kept epoch is unambiguous.

The GOP is ragged on purpose: a 6-bit shell that fixes scale_num at 4, a sphere8 frame (the largest: the shared arena is sized by a
frame that is not the first) and a 450-point cloud that lacks the two coarsest scales (per-scale Adam counters); step_size 2 and gamma
0.5 bring the learning rate under min_lr in epoch 1 (the clamp)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 8807
EPOCHS = 4
ADAM = dict(lr=0.01, step_size=2, gamma=0.5)
MIN_LR = 4e-3
N_FRAMES = 3
LOSS_REL = 2 * N_FRAMES * 2.0 ** -53 + 2.0 ** -52

CASES = {
    'f32-bl1': dict(),
    'f32-bl3': dict(bl=3),
    'bf16': dict(tp='bf16'),
    'bf16-deep2': dict(tp='bf16-deep', bl=2),
    'w16': dict(hidden=16),
    'w32-mul': dict(hidden=32, tp='bf16-mul', c_step=True),
    'qat-f32': dict(qat=2),
    'qat-w16': dict(hidden=16, qat=2, c_step=True),          # the Python loop has aware steps at this width on the one-call step only
    'last': dict(keep='last'),
}
_gops, _refs = {}, {}


def _gop(bl):
    """One GOP per block_layers for the whole module: training never writes to a frame."""
    from linr_pcgc_amd import overfit, synthetic
    if bl not in _gops:
        clouds = [synthetic.sphere_shell(6, 20), synthetic.sequence_frame('sphere8', 0), synthetic.sphere_shell(5, 6)]
        gop = overfit.Gop(None, clouds, None, 64, 'cuda', block_layers=bl)
        assert gop.scale_num == 4 and [f.n_scales for f in gop.frames] == [4, 4, 2]
        assert max(range(3), key=lambda j: gop.frames[j].rows) == 1
        _gops[bl] = gop
    return _gops[bl]


def _run(c_loop, bl=1, hidden=8, tp='f32', qat=0, keep='best', c_step=False, adam=ADAM, epochs=EPOCHS, ckpt=None, poke=None, min_lr=MIN_LR):
    """A fresh model of the module's seed through one overfit -> everything the contract compares."""
    from linr_pcgc_amd import overfit
    from linr_pcgc_amd.model_core import FlatAdam
    gop = _gop(bl)
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=SEED, block_layers=bl, hidden=hidden)
    model.train_precision = tp
    if c_step:
        model._wide.c_step = True
    opt = FlatAdam(model, **adam)
    if ckpt is not None:
        overfit.warm_start(model, opt, ckpt)
    if poke is not None:
        poke(model)
    info, err, losses = {}, None, None
    try:
        losses = overfit.overfit_gop(model, opt, gop, epochs, min_lr, keep=keep, info=info, qat_epochs=qat, c_loop=c_loop)
    except FloatingPointError as e:
        err = str(e)
    torch.cuda.synchronize()
    return {'params': model.flat_parameters().clone(), 'exp_avg': opt.exp_avg.clone(), 'exp_avg_sq': opt.exp_avg_sq.clone(), 't': opt.t,
            't_scale': opt.t_scale.tolist(), 'lr': opt.lr, 'sched_steps': opt.sched_steps, 'info': info, 'losses': losses, 'err': err,
            'model': model, 'opt': opt}


def _ref(name):
    if name not in _refs:
        _refs[name] = _run(False, **CASES[name])
    return _refs[name]


def _unambiguous(losses, first=0):
    """The precondition: the two smallest competing losses differ by more than the bound."""
    c = sorted(x for x in losses[first:] if math.isfinite(x))
    assert len(c) >= 1
    if len(c) > 1:
        assert (c[1] - c[0]) > LOSS_REL * c[1], ('change the seed of the case, not the bound', losses)


def _same_state(py, c):
    for key in ('params', 'exp_avg', 'exp_avg_sq'):          # bit patterns: a diverged run's NaNs are equal, too
        assert torch.equal(py[key].view(torch.int32), c[key].view(torch.int32)), key
    for key in ('t', 't_scale', 'lr', 'sched_steps'):
        assert py[key] == c[key], (key, py[key], c[key])


def _same_losses(py, c):
    assert len(py) == len(c)
    for e, (a, b) in enumerate(zip(py, c)):
        print('epoch %d: loop %.17g, call %.17g, rel %.3g (bound %.3g)' % (e, a, b, abs(a - b) / a if math.isfinite(a) and a else 0.0, LOSS_REL))
        assert (a == b) or abs(a - b) <= LOSS_REL * a, (e, a, b)


def _compare(name, py, c):
    kw = CASES[name]
    assert py['err'] is None and c['err'] is None
    first = EPOCHS - kw['qat'] if kw.get('qat') else 0
    if kw.get('keep', 'best') == 'best':
        _unambiguous(py['losses'], first)
    _same_losses(py['losses'], c['losses'])
    _same_state(py, c)
    assert py['info']['coded_epoch'] == c['info']['coded_epoch']
    assert c['info']['coded_loss'] == c['losses'][c['info']['coded_epoch']]
    assert py['info'].get('qat_from') == c['info'].get('qat_from') == (first if kw.get('qat') else None)
    if kw.get('qat'):
        assert c['info']['coded_epoch'] >= first          # only the aware epochs compete


def test_the_schedule_reaches_the_clamp_in_epoch_1(pkg):
    from linr_pcgc_amd import engine
    plan = engine.overfit_plan(_gop(1).frames, EPOCHS, 4, min_lr=MIN_LR, **ADAM)
    assert plan['end_lr'][0] > MIN_LR > plan['end_lr'][1] and plan['lr'][2 * N_FRAMES] == MIN_LR
    assert plan['scale_steps'][2].tolist() == [3, 3, 3, 3] and plan['scale_steps'][-1].tolist() == [12] * 4


@pytest.mark.parametrize('name', sorted(CASES))
def test_c_loop_equals_the_python_loop(pkg, name):
    _compare(name, _ref(name), _run(True, **CASES[name]))
    if name == 'last':
        assert _ref(name)['info']['coded_epoch'] == EPOCHS - 1 and _ref(name)['lr'] == MIN_LR          # the state after the last clamp


@pytest.mark.parametrize('name', sorted(CASES))
def test_c_loop_under_poison(pkg, name, monkeypatch):
    """The case list with the LDS and the vector registers of every CU filled with a NaN pattern in front of every launch, the epoch
    kernels' included (class 12), and every scratch buffer - the call's workspace among them - filled with 0xFF: results unchanged."""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    monkeypatch.setenv('LINR_DEBUG_POISON', '1')          # _lib.scratch reads it per call
    L.linr_debug_poison(0xFFFFFF)
    try:
        dirty = _run(True, **CASES[name])
    finally:
        L.linr_debug_poison(0)
        monkeypatch.undo()
        L.linr_debug_poison(0xFFFFFF if os.environ.get('LINR_DEBUG_POISON') else 0)
    _compare(name, _ref(name), dirty)


BEST_EARLY = dict(lr=0.004, step_size=3, gamma=4.0)          # the rate grows fourfold per epoch: the loss falls, then rises again


def test_the_best_epoch_is_not_the_last(pkg):
    from linr_pcgc_amd import engine
    py = _run(False, adam=BEST_EARLY, min_lr=4e-4)
    print('losses', py['losses'])
    best = int(np.argmin(py['losses']))
    assert py['err'] is None and all(math.isfinite(x) for x in py['losses']) and 0 < best < EPOCHS - 1, py['losses']          # the precondition
    _unambiguous(py['losses'])
    c = _run(True, adam=BEST_EARLY, min_lr=4e-4)
    assert c['err'] is None
    _same_losses(py['losses'], c['losses'])
    _same_state(py, c)
    assert c['info']['coded_epoch'] == py['info']['coded_epoch'] == best
    plan = engine.overfit_plan(_gop(1).frames, EPOCHS, 4, min_lr=4e-4, **BEST_EARLY)
    assert c['lr'] == plan['end_lr'][best] and c['t'] == N_FRAMES * (best + 1) and c['sched_steps'] == plan['end_sched'][best]


@pytest.mark.parametrize('keep', ['best', 'last'])
def test_a_non_finite_parameter_is_a_diverged_overfit_not_a_fault(pkg, keep):
    def poke(model):
        model.flat_parameters()[1234] = float('inf')
    py = _run(False, keep=keep, poke=poke)
    c = _run(True, keep=keep, poke=poke)
    assert py['err'] is not None and py['err'] == c['err'] and 'no finite epoch to keep' in c['err']
    assert "['inf', 'inf', 'inf', 'inf']" in c['err']
    _same_state(py, c)


DIVERGE_LATE = dict(lr=0.01, step_size=3, gamma=1e4)          # 0.01, 100, 1e6, 1e10 per epoch: finite first, non-finite parameters later


def test_parameters_that_become_non_finite_later_keep_the_same_earlier_epoch(pkg):
    py = _run(False, adam=DIVERGE_LATE, min_lr=4e-4)
    print('losses', py['losses'])
    assert py['err'] is None and math.isfinite(py['losses'][0]) and math.isinf(py['losses'][-1]), py['losses']          # the precondition
    _unambiguous(py['losses'])
    c = _run(True, adam=DIVERGE_LATE, min_lr=4e-4)
    assert c['err'] is None
    _same_losses(py['losses'], c['losses'])
    _same_state(py, c)
    assert c['info']['coded_epoch'] == py['info']['coded_epoch'] < EPOCHS - 1
    assert bool(torch.isfinite(c['params']).all())


def test_warm_start_continues_identically(pkg):
    from linr_pcgc_amd import overfit
    first = _ref('f32-bl1')
    ckpt = overfit.checkpoint(first['model'], first['opt'], first['info']['coded_epoch'], first['info']['coded_loss'])
    assert first['t'] > 0 and bool(first['exp_avg'].abs().sum() > 0)
    py = _run(False, ckpt=ckpt, epochs=3)
    c = _run(True, ckpt=ckpt, epochs=3)
    assert py['err'] is None and c['err'] is None and py['t'] > first['t']
    _unambiguous(py['losses'])
    _same_losses(py['losses'], c['losses'])
    _same_state(py, c)
    assert c['info']['coded_epoch'] == py['info']['coded_epoch']


def test_more_frames_than_one_start_launch_takes(pkg):
    """33 frames: the point numbers reach the workspace in chunks of 32 per start launch (overfit_init_k with base > 0) - a second
    launch whose one frame must land in slot 32, beside a first that keeps the starting state.  450 .. 1,000-point clouds, 2 epochs."""
    from linr_pcgc_amd import _lib, overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam
    n = 33
    gop = overfit.Gop(None, [synthetic.sphere_shell(5, 6 + t % 3) for t in range(n)], None, 64, 'cuda')
    assert len(set(gop.point_nums)) == 3 and gop.point_nums[32] != gop.point_nums[31]          # a wrong slot would show in the loss
    bound = 2 * n * 2.0 ** -53 + 2.0 ** -52          # the module's bound at this n_frames

    def run(c_loop):
        model = overfit.gen_model(gop.scale_num, 'cuda', seed=SEED)
        opt = FlatAdam(model, **ADAM)
        info = {}
        losses = overfit.overfit_gop(model, opt, gop, 2, MIN_LR, info=info, c_loop=c_loop)
        torch.cuda.synchronize()
        return losses, info['coded_epoch'], model.flat_parameters().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.lr, opt.t
    py, c = run(False), run(True)
    lo, hi = sorted(py[0])
    assert hi - lo > bound * hi, py[0]          # the precondition: the kept epoch is unambiguous
    for a, b in zip(py[0], c[0]):
        print('loop %.17g, call %.17g, bound %.3g' % (a, b, bound))
        assert abs(a - b) <= bound * a
    assert py[1] == c[1] and py[5:] == c[5:]
    for a, b in zip(py[2:5], c[2:5]):
        assert torch.equal(a, b)
    L = _lib.lib()
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=SEED)
    counts = _prof(L, lambda: overfit.overfit_gop(model, FlatAdam(model, **ADAM), gop, 1, MIN_LR, c_loop=True))
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=SEED)
    loop = _prof(L, lambda: overfit.overfit_gop(model, FlatAdam(model, **ADAM), gop, 1, MIN_LR, c_loop=False))
    assert counts[12] == loop[12] + 2 + 3 + 1          # TWO start launches


def _prof(L, fn):
    tot, nl, npass = ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
    torch.cuda.synchronize()
    try:
        L.linr_prof_mask(0xFFFFFFFF)
        assert L.linr_prof_enable(1) == 0
        fn()
        torch.cuda.synchronize()
        L.linr_prof_enable(0)
        out = []
        for k in range(24):
            assert L.linr_prof_read(k, ctypes.byref(tot), ctypes.byref(nl), ctypes.byref(npass)) == 0
            out.append(nl.value)
        return out
    finally:
        L.linr_prof_mask(3)
        L.linr_prof_enable(0)


def test_the_call_launches_every_step_and_its_own_kernels_once(pkg):
    """The launch counts of the library's profiler: epochs x n_frames steps, each with the launches of the Python loop's step, plus -
    in class 12 - the call's own: one start launch, per epoch the finite check, the epoch's close and the conditional snapshot, and
    the one restore.  That is what this test holds: the issue lets the single host synchronisation be checked by counting launches,
    and no counter of the library sees a wait - a second hipStreamSynchronize added to linr_overfit_gop would NOT fail here.  That there
    is one is read off csrc/overfit.hip: nothing between the launches reads a device value, the only wait follows the copy of the
    losses and the state."""
    from linr_pcgc_amd import _lib, overfit
    from linr_pcgc_amd.model_core import FlatAdam
    L = _lib.lib()
    gop = _gop(1)
    epochs = 2

    def make():
        model = overfit.gen_model(gop.scale_num, 'cuda', seed=SEED)
        return model, FlatAdam(model, **ADAM)
    model, opt = make()
    loop = _prof(L, lambda: overfit.overfit_gop(model, opt, gop, epochs, MIN_LR, c_loop=False))
    model, opt = make()
    call = _prof(L, lambda: overfit.overfit_gop(model, opt, gop, epochs, MIN_LR, c_loop=True))
    model, opt = make()
    one = _prof(L, lambda: overfit.overfit_gop(model, opt, gop.subset(1), 1, MIN_LR, keep='last', c_loop=False))
    print(loop, call, one)
    assert one[0] > 0 and loop[0] == epochs * N_FRAMES * one[0]          # class 0: the fused backward, the same count for every frame
    own = 1 + epochs * 3 + 1
    assert call == [n + (own if k == 12 else 0) for k, n in enumerate(loop)]


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, 'rb').read()
    return out


def _tensors(x, prefix=''):
    if torch.is_tensor(x):
        return {prefix: x}
    out = {}
    if isinstance(x, dict):
        for k, v in x.items():
            out.update(_tensors(v, '%s/%s' % (prefix, k)))
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            out.update(_tensors(v, '%s/%d' % (prefix, i)))
    return out


def test_run_with_c_overfit_writes_the_files_of_the_plain_run(pkg, tmp_path):
    from linr_pcgc_amd import run
    base = ['--config', 'sphere8', '--frames', '4', '--gop', '2', '--first-epoch', '3', '--others-epoch', '2', '--decode']
    got = {}
    for name, extra in (('plain', []), ('c', ['--c-overfit']), ('c-pipe', ['--c-overfit', '--pipeline'])):
        out = str(tmp_path / name)
        summary, results = run.run_sequence_job(run.parse(base + extra + ['--out', out]), 0, 1, None)
        assert summary['lossless'] is True, name
        if name == 'plain':          # the precondition, from the Python loop's own losses: every GOP's kept epoch is unambiguous
            for r in results.values():
                two = sorted(r['loss'])[:2]
                assert two[1] - two[0] > (2 * 2 * 2.0 ** -53 + 2.0 ** -52) * two[1], r['loss']
        ck = torch.load(os.path.join(out, 'output', 'gop_0_1', 'model.pth'), map_location='cpu', weights_only=False)
        got[name] = (_tree(os.path.join(out, 'result_enc')), _tensors(ck['model']), _tensors(ck['optimizer_state_dict']),
                     ck['optimizer_state_dict']['param_groups'][0]['lr'], ck['epoch'], {g: r['coded_epoch'] for g, r in results.items()})
    plain = got['plain']
    assert len(plain[0]) > 4 and len(plain[1]) > 10
    for name in ('c', 'c-pipe'):
        tree, model, optim, lr, epoch, coded = got[name]
        assert sorted(tree) == sorted(plain[0])
        for f in tree:
            assert tree[f] == plain[0][f], (name, f)
        for a, b in ((model, plain[1]), (optim, plain[2])):
            assert sorted(a) == sorted(b)
            for k in a:
                assert torch.equal(a[k], b[k]), (name, k)
        assert (lr, epoch, coded) == plain[3:], name


def test_run_writes_the_epoch_records_of_a_diverged_one_call_overfit(pkg, tmp_path):
    """The Python loop has written every epoch's record to info.log and result.json when it raises; the one call's records are written
    from the losses its error carries."""
    import json
    from linr_pcgc_amd import run
    logs = {}
    for name, extra in (('plain', []), ('c', ['--c-overfit'])):
        out = str(tmp_path / name)
        args = run.parse(['--config', 'sphere8', '--frames', '2', '--gop', '2', '--first-epoch', '2', '--learning-rate', '1e8', '--out', out] + extra)
        with pytest.raises(FloatingPointError, match='no finite epoch to keep'):
            run.run_sequence_job(args, 0, 1, None)
        records = json.load(open(os.path.join(out, 'output', 'gop_0_1', 'result.json')))
        logs[name] = ([(r['epoch'], r['loss']) for r in records], open(os.path.join(out, 'info.log')).read().count('epoch: '))
    assert logs['plain'][0] == logs['c'][0] == [(0, float('inf')), (1, float('inf'))] and logs['plain'][1] == logs['c'][1] == 2
