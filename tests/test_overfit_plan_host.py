"""CPU: the host side of the one-call overfit (csrc/overfit.hip): linr_overfit_plan against a replay of FlatAdam.advance / scheduler_step /
clamp_lr (exact equality of every double and integer), the refusals of linr_overfit_gop with their place in the documented order - each
returns in front of the first launch, so the entry runs here on sentinel-filled host memory that must come back untouched - and the
refusals of the Python switches.  Nothing needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('linr_overfit_plan', 'linr_overfit_ws_bytes', 'linr_overfit_gop')
EINVAL, ENOSPC, EALIGN = -1, -2, -3
F32, BF16, WIDE = 0, 1, 2
MUL_BF16 = 16
SENTINEL = 0xA5


@pytest.fixture(scope='module')
def lib():
    from linr_pcgc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_exports(lib):
    from linr_pcgc_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'linr_hip.h')).read()
    declared = set(re.findall(r'^LINR_API\s+[\w\s\*]+?\b(linr_\w+)\(', header, flags=re.M))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.linr_abi_version() == 27          # additive exports only
    assert (_lib.LINR_OVERFIT_F32, _lib.LINR_OVERFIT_BF16, _lib.LINR_OVERFIT_WIDE) == (F32, BF16, WIDE)
    for name, value in (('F32', 0), ('BF16', 1), ('WIDE', 2)):
        assert re.search(r'#define LINR_OVERFIT_%s\s+%d\b' % (name, value), header)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
class _Stub:
    """What FlatAdam.advance and engine.overfit_plan read of a frame."""

    def __init__(self, rows_per_scale, scale_idx=None):
        self.n_scales = len(rows_per_scale)
        self.row_off = np.concatenate([[0], np.cumsum(rows_per_scale)]).astype(np.int64)
        self.scale_idx = np.asarray(range(self.n_scales) if scale_idx is None else scale_idx, dtype=np.int32)


class _Model:
    def __init__(self, scale_num):
        import torch
        self.scale_num = scale_num
        self._flat = torch.zeros(4)

    def flat_parameters(self):
        return self._flat


def _replay(frames, epochs, S, start, step_size, gamma, min_lr):
    """overfit_gop's loop over the optimiser's host state alone: model_core.train_step's advance / commit / scheduler_step per frame,
    BestState.offer's meta and clamp_lr per epoch."""
    from linr_pcgc_amd.model_core import FlatAdam
    opt = FlatAdam(_Model(S), lr=start['lr'], step_size=step_size, gamma=gamma)
    opt.t, opt.sched_steps = start['step'], start['sched_steps']
    opt.t_scale = np.asarray(start['scale_steps'], dtype=np.int64).copy()
    out = {k: [] for k in ('lr', 'step', 'scale_steps', 'end_step', 'end_sched', 'end_lr', 'end_scale_steps')}
    for _ in range(epochs):
        for f in frames:
            t, t_scale = opt.advance(f)
            out['lr'].append(opt.lr)
            out['step'].append(t)
            out['scale_steps'].append(t_scale.copy())
            opt.t, opt.t_scale = t, t_scale
            opt.scheduler_step()
        out['end_step'].append(opt.t)
        out['end_sched'].append(opt.sched_steps)
        out['end_lr'].append(opt.lr)
        out['end_scale_steps'].append(opt.t_scale.copy())
        opt.clamp_lr(min_lr)
    return out


COLD = dict(step=0, sched_steps=0, lr=0.01, scale_steps=[0] * 5)
PLAN_CASES = {
    # frames 1 and 2 lack the coarsest scales (custom_dataset.py:325)
    'lacks_coarsest': ([_Stub([50, 20, 9, 4, 2]), _Stub([30, 12, 5]), _Stub([20, 7])], 3, 5, COLD, 32, 0.992, 4e-4),
    # scale 1 of frame 0 has zero rows: not present, its counter starts with frame 1
    'zero_rows': ([_Stub([40, 0, 6]), _Stub([30, 9, 4]), _Stub([10, 0, 0])], 3, 5, COLD, 32, 0.992, 4e-4),
    # scales 3 and 4 first appear in frame 2 of epoch 0
    'late_scale': ([_Stub([40, 10]), _Stub([30, 9, 4]), _Stub([50, 20, 9, 4, 2])], 4, 5, COLD, 32, 0.992, 4e-4),
    # the clamp is reached in epoch 1 and must persist through the later gamma steps
    'clamp': ([_Stub([50, 20, 9, 4, 2]), _Stub([9, 4, 2], [2, 3, 4]), _Stub([20, 7])], 4, 5, COLD, 2, 0.5, 4e-3),
    # warm start: non-zero counters, scale 4 never started, a learning rate below min_lr
    'warm': ([_Stub([50, 20, 9, 4]), _Stub([30, 12, 5]), _Stub([20, 7, 3, 2, 1])], 3, 5,
             dict(step=96, sched_steps=97, lr=3.7e-4, scale_steps=[96, 96, 90, 64, 0]), 32, 0.992, 4e-4),
    'warm_clamp': ([_Stub([50, 20, 9]), _Stub([30, 12, 5, 2])], 5, 6,
                   dict(step=7, sched_steps=7, lr=0.013, scale_steps=[7, 7, 7, 0, 0, 0]), 3, 0.7, 5e-3),
}


@pytest.mark.parametrize('case', sorted(PLAN_CASES))
def test_plan_equals_the_replay_of_flat_adam(lib, case):
    from linr_pcgc_amd import engine
    frames, epochs, S, start, step_size, gamma, min_lr = PLAN_CASES[case]
    got = engine.overfit_plan(frames, epochs, S, start['step'], start['sched_steps'], start['lr'], start['scale_steps'], step_size, gamma,
                              min_lr)
    ref = _replay(frames, epochs, S, start, step_size, gamma, min_lr)
    for key in ('lr', 'end_lr'):
        assert got[key].dtype == np.float64
        assert got[key].tobytes() == np.asarray(ref[key], dtype=np.float64).tobytes(), (key, got[key], ref[key])
    for key in ('step', 'end_step', 'end_sched'):
        assert got[key].tolist() == [int(v) for v in ref[key]], key
    for key in ('scale_steps', 'end_scale_steps'):
        assert np.array_equal(got[key], np.asarray(ref[key], dtype=np.int64).reshape(got[key].shape)), key
    if case == 'clamp':          # the case is what it says: the clamp acts in epoch 1 and later steps start from it
        assert ref['end_lr'][1] < min_lr and ref['lr'][2 * len(frames)] == min_lr
        assert ref['lr'][-1] in (min_lr, min_lr * gamma)
    if case == 'late_scale':
        assert got['scale_steps'][1].tolist() == [2, 2, 1, 0, 0] and got['scale_steps'][2].tolist() == [3, 3, 2, 1, 1]
    if case == 'zero_rows':
        assert got['scale_steps'][0].tolist() == [1, 0, 1, 0, 0] and got['scale_steps'][2].tolist() == [3, 2, 3, 0, 0]


def test_plan_refusals_and_null_outputs(lib):
    from linr_pcgc_amd import _lib, engine
    frames = PLAN_CASES['clamp'][0]
    assert engine.overfit_plan(frames, 0, 5)['lr'].size == 0
    for kw in (dict(epochs=-1), dict(model_scale_num=0), dict(model_scale_num=17), dict(step_size=0)):
        a = dict(frames=frames, epochs=2, model_scale_num=5)
        a.update(kw)
        with pytest.raises(_lib.LinrError):
            engine.overfit_plan(**a)
    with pytest.raises(_lib.LinrError):
        engine.overfit_plan([], 2, 5)
    with pytest.raises(_lib.LinrError):
        engine.overfit_plan([_Stub([5, 3], [0, 5])], 2, 5)          # a scale outside the model
    n = [None] * 7
    assert lib.linr_overfit_plan(None, 1, 1, 5, 0, 0, 0.01, None, 32, 0.9, 1e-4, *n) == EINVAL
    f = _Frame(10, 0)
    ptrs = (ctypes.c_void_p * 1)(ctypes.addressof(f.c))
    assert lib.linr_overfit_plan(ptrs, 1, 3, 5, 0, 0, 0.01, None, 32, 0.9, 1e-4, *n) == 0          # every output may be NULL


# ---- linr_overfit_gop: refusals ---------------------------------------------------------------------------------------------------------
class _Frame:
    """A linr_frame over host memory: good enough for every check that comes in front of the first launch."""

    def __init__(self, rows, p, **kw):
        from linr_pcgc_amd._lib import LinrFrame
        self.row_off = np.asarray([0, rows], dtype=np.int64)
        self.sidx = np.asarray([0], dtype=np.int32)
        f = dict(rows=rows, n_scales=1, model_scale_num=5, block_layers=1, flags=1, row_off_h=self.row_off.ctypes.data,
                 scale_idx_h=self.sidx.ctypes.data, nbr=p, nbr_ld=(rows + 63) // 64 * 64, nbr_lo=p, nbr_mask=p, offset_feat=p, occ=p,
                 nbr8t=p)
        f.update(kw)
        self.c = LinrFrame(**f)


class _Host:
    """Sentinel-filled host memory that stands in for every device buffer of a call; untouched() after a refusal."""

    def __init__(self, nbytes=1 << 16):
        self.buf = (ctypes.c_ubyte * nbytes)()
        ctypes.memset(self.buf, SENTINEL, nbytes)
        self.n = nbytes
        self.p = (ctypes.addressof(self.buf) + 63) & ~63

    def untouched(self):
        return bytes(self.buf) == bytes([SENTINEL]) * self.n


def test_ws_bytes(lib):
    W = lib.linr_overfit_ws_bytes
    assert W(-1, 1, 1) == 0 and W(10, -1, 1) == 0 and W(10, 1, -1) == 0
    assert W(54712, 32, 10) >= 3 * 4 * 54712 + 8 * (32 + 32 + 10)
    assert W(54713, 3, 4) >= 3 * 4 * 54713 + 8 * (3 + 3 + 4) and W(54713, 3, 4) % 16 == 0
    assert W(0, 0, 0) >= 0 and W(100, 3, 5) > W(100, 3, 4) >= W(100, 2, 4) and W(104, 3, 4) > W(100, 3, 4)


def test_gop_refusals_and_their_order(lib):
    """NULL pieces, n_frames, epochs, qat_from, qparams / bitdepth, the executor, hidden and flags, the workspace, then every frame as
    the executor's step entry checks it (the arena's size among them): each refusal is shown with later ones present, too, and none of
    them writes a byte or touches a GPU."""
    from linr_pcgc_amd._lib import LinrOverfitArgs, LinrOverfitFrame, LinrOverfitResult
    h = _Host(1 << 20)
    p = h.p
    n_params = lib.linr_param_count(5, 1)
    n_wide = lib.linr_param_count_wide(5, 1, 16)
    arena = {F32: lib.linr_net_arena_bytes(100, 1), BF16: lib.linr_net_train_bf16_arena_bytes(100, 1),
             WIDE: lib.linr_net_wide_train_arena_bytes(100, 16, 1)}
    losses = np.zeros(8)
    good = _Frame(100, p)

    def call(frames=(good, good), pn=(100.0, 90.0), args='good', result='good', **kw):
        executor = kw.get('executor', F32)
        n = n_wide if executor == WIDE else n_params
        a = dict(executor=F32, hidden=16 if executor == WIDE else 8, flags=0, n_frames=0 if frames is None else len(frames), params=p,
                 exp_avg=p + 1024, exp_avg_sq=p + 2048, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-4, lr=0.01, min_lr=4e-4,
                 gamma=0.992, step_size=32, step=0, sched_steps=0, scale_steps_h=None, epochs=4, keep_best=1, qat_from=4, bitdepth=8,
                 qparams=None, arena=p, arena_bytes=arena.get(executor, 0), ws=p + 4096, ws_bytes=lib.linr_overfit_ws_bytes(n, 2, 4))
        a.update(kw)
        fr = None
        if frames is not None:
            fr = (LinrOverfitFrame * max(len(frames), 1))()
            for j, f in enumerate(frames):
                fr[j].f = None if f is None else ctypes.pointer(f.c)
                fr[j].point_num = pn[j]
        res = LinrOverfitResult(losses_h=losses.ctypes.data)
        rc = lib.linr_overfit_gop(fr, None if args is None else ctypes.byref(LinrOverfitArgs(**a)),
                                  None if result is None else ctypes.byref(res), None)
        assert h.untouched(), 'a refused call wrote'
        return rc
    bad_frame = _Frame(100, p, nbr_lo=None)
    # 1. NULL pieces in front of everything (bad counts, bad executor, short buffers, a bad frame present)
    later = dict(epochs=-1, executor=7, ws_bytes=0, arena_bytes=0)
    assert call(frames=None, **later) == EINVAL
    assert call(args=None) == EINVAL
    assert call(result=None, **later) == EINVAL
    for piece in ('params', 'exp_avg', 'exp_avg_sq', 'arena', 'ws'):
        assert call(frames=(bad_frame, good), **{**later, piece: None}) == EINVAL, piece
    # 2. n_frames < 1, 3. a NULL frame, epochs < 0
    assert call(n_frames=0, executor=7, ws_bytes=0) == EINVAL
    assert call(n_frames=-2, executor=7, ws_bytes=0) == EINVAL
    assert call(frames=(good, None), executor=7, ws_bytes=0) == EINVAL
    assert call(epochs=-1, qat_from=-1, ws_bytes=0) == EINVAL
    # 4. qat_from outside [0, epochs]; with aware epochs qparams is needed; bitdepth 2..16 with qparams
    assert call(qat_from=-1, ws_bytes=0) == EINVAL
    assert call(qat_from=5, ws_bytes=0) == EINVAL
    assert call(qat_from=2, ws_bytes=0) == EINVAL
    for depth in (1, 17, 0, -8):
        assert call(qat_from=2, qparams=p + 8192, bitdepth=depth, ws_bytes=0) == EINVAL
        assert call(qparams=p + 8192, bitdepth=depth, ws_bytes=0) == EINVAL          # read with qparams even when no epoch is aware
    assert call(step_size=0, ws_bytes=0) == EINVAL
    assert call(step=-1, ws_bytes=0) == EINVAL
    for bad_pn in (0.0, -3.0, float('inf'), float('nan')):
        assert call(pn=(100.0, bad_pn), ws_bytes=0) == EINVAL
    # 5. the executor, hidden and flags in front of the sizes (a short workspace would be LINR_ENOSPC)
    for executor in (-1, 3, 7):
        assert call(executor=executor, hidden=8, ws_bytes=0) == EINVAL
    assert call(executor=WIDE, hidden=8, ws_bytes=0) == EINVAL
    assert call(executor=WIDE, hidden=24, ws_bytes=0) == EINVAL
    assert call(executor=F32, hidden=16, ws_bytes=0) == EINVAL
    assert call(executor=BF16, hidden=32, ws_bytes=0) == EINVAL
    assert call(executor=F32, flags=MUL_BF16, ws_bytes=0) == EINVAL
    assert call(executor=WIDE, flags=1, ws_bytes=0) == EINVAL
    assert call(frames=(good, _Frame(100, p, model_scale_num=6)), ws_bytes=0) == EINVAL          # one model for the whole GOP
    assert call(frames=(good, _Frame(100, p, block_layers=2)), ws_bytes=0) == EINVAL
    assert call(params=p + 4, ws_bytes=0) == EALIGN
    assert call(ws=p + 4096 + 8, ws_bytes=0) == EALIGN
    # 6. the workspace, in front of the frames and the arena
    for executor in (F32, BF16, WIDE):
        n = n_wide if executor == WIDE else n_params
        assert call(frames=(bad_frame, good), executor=executor, ws_bytes=lib.linr_overfit_ws_bytes(n, 2, 4) - 1, arena_bytes=0) == ENOSPC
    # 7. every frame as the step entry checks it: the arena for the largest frame, the frame's structure and matrices
    for executor in (F32, BF16, WIDE):
        assert call(executor=executor, arena_bytes=arena[executor] - 1) == ENOSPC, executor
        assert call(frames=(good, _Frame(200, p)), executor=executor) == ENOSPC, executor          # the arena is sized for 100 rows
        assert call(frames=(good, bad_frame), executor=executor) == EINVAL, executor
        wrong = _Frame(100, p)
        wrong.row_off[1] = 99
        assert call(frames=(good, wrong), executor=executor) == EINVAL
        assert call(executor=executor, qat_from=2, qparams=p) == EINVAL          # qparams == params
        assert call(executor=executor, qat_from=2, qparams=p + 8196) == EALIGN
    assert call(executor=WIDE, flags=MUL_BF16, arena_bytes=arena[WIDE] - 1) == ENOSPC
    # ... and the counters: a started count below zero would leave a scale of the frame at 0 at its own step
    for executor in (F32, BF16, WIDE):
        ts = np.asarray([-1, 0, 0, 0, 0], dtype=np.int64)
        assert call(executor=executor, scale_steps_h=ts.ctypes.data) == EINVAL
        ts = np.asarray([3, 0, -2, 0, 0], dtype=np.int64)
        assert call(executor=executor, scale_steps_h=ts.ctypes.data) == EINVAL


# ---- the Python switches ----------------------------------------------------------------------------------------------------------------
def test_c_loop_with_on_epoch_is_refused_before_anything_runs():
    from linr_pcgc_amd import overfit
    assert overfit.C_OVERFIT is (os.environ.get('LINR_C_OVERFIT', '0') == '1')          # opt-in
    with pytest.raises(ValueError, match='on_epoch'):
        overfit.overfit_gop(None, None, None, 4, on_epoch=lambda e, x: None, c_loop=True)          # nothing of model, opt, gop is touched


def test_run_refuses_c_overfit_with_mid_test(monkeypatch):
    from linr_pcgc_amd import overfit, run
    monkeypatch.setattr(overfit, 'C_OVERFIT', False)
    assert run.parse([]).c_overfit is False
    assert run.parse(['--c-overfit']).c_overfit is True
    args = run.parse(['--c-overfit', '--pipeline', '--qat-epochs', '2', '--keep', 'last', '--decode', '--train-precision', 'bf16'])
    assert args.c_overfit and args.pipeline and args.qat_epochs == 2
    for width in ('16', '32'):          # the call runs the one-call step of the wide models, whatever LINR_WIDE_C_STEP says
        assert run.parse(['--c-overfit', '--qat-epochs', '1', '--hidden-channel-conv', width]).qat_epochs == 1
    with pytest.raises(SystemExit):
        run.parse(['--c-overfit', '--mid-test'])
    # LINR_C_OVERFIT=1 is the same switch: the same refusal, the same exemption of the wide models' aware epochs
    monkeypatch.setattr(overfit, 'C_OVERFIT', True)
    assert run.parse([]).c_overfit is True
    with pytest.raises(SystemExit):
        run.parse(['--mid-test'])
    assert run.parse(['--qat-epochs', '1', '--hidden-channel-conv', '16']).qat_epochs == 1
