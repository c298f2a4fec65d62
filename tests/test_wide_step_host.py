"""CPU: the host side of the wide training step (csrc/wide_train.hip): exports, the arena size, and every refusal with its place in the
documented order.  Refusals return in front of the first launch, so the entries run here on host memory filled with a sentinel that
must come back untouched; nothing needs a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('linr_net_wide_train_arena_bytes', 'linr_net_forward_train_wide', 'linr_net_backward_wide', 'linr_net_train_step_wide')
EINVAL, ENOSPC, EALIGN = -1, -2, -3
MUL_BF16 = 16
SENTINEL = 0xA5


@pytest.fixture(scope='module')
def lib():
    from linr_pcgc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_header_binding_and_library_agree_on_the_exports(lib):
    from linr_pcgc_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'linr_hip.h')).read()
    declared = set(re.findall(r'^LINR_API\s+[\w\s\*]+?\b(linr_\w+)\(', header, flags=re.M))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert declared == set(_lib.EXPORTS)
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    dynamic = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('linr_') and ln.split()[-2] in 'TW'}
    assert dynamic == declared, (sorted(dynamic - declared), sorted(declared - dynamic))
    assert lib.linr_abi_version() == 27          # additive exports only


def test_train_arena_size(lib):
    T, A = lib.linr_net_wide_train_arena_bytes, lib.linr_net_wide_arena_bytes
    assert T(-1, 16, 1) == 0 and T(100, 8, 1) == 0 and T(100, 24, 1) == 0 and T(100, 0, 1) == 0 and T(100, 64, 1) == 0
    assert T(100, 16, 0) == 0 and T(100, 16, 5) == 0 and T(100, 32, -1) == 0
    assert T((1 << 27) - 1, 16, 1) == 0          # over linr_frame's row bound
    for hidden in (16, 32):
        for bl in (1, 2, 3, 4):
            sizes = [T(r, hidden, bl) for r in (0, 1, 100, 1000, 100000, (1 << 27) - 2)]
            assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), (hidden, bl, sizes)
            for r in (0, 1, 1000, 100000):
                assert T(r, hidden, bl) > A(r, hidden, bl, 0)          # the tape, the gradients and the slabs on top of the forward's roles
        assert T(100000, hidden, 3) > T(100000, hidden, 1)          # no alternating roles: every layer's tensors stay live
        assert T(100000, hidden, 4) > T(100000, hidden, 3) > T(100000, hidden, 2)
        # a layer of block_in is 3 half-wide + 1 full-wide tensors of (rows + 1) x 8 floats per block
        nb, nh = hidden // 8, hidden // 16
        assert T(100000, hidden, 3) - T(100000, hidden, 2) >= (3 * nh + nb) * 100001 * 32
    assert T(1000, 16, 1) < T(1000, 32, 1)
    # no 32-bit wrap at the largest frame: at least the 8 prune outputs of (rows + 1) x 32 bytes per block, over 2^35
    rows = (1 << 27) - 2
    for hidden in (16, 32):
        big = T(rows, hidden, 1)
        assert big > 8 * (hidden // 8) * (rows + 1) * 32 > 1 << 35
        assert big - T(rows - 1000, hidden, 1) >= 1000 * 32 * 8 * (hidden // 8)          # still linear in the rows up there


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

    def ref(self):
        return ctypes.byref(self.c)


class _Host:
    """Sentinel-filled host memory that stands in for every device buffer of a call; untouched() after a refusal."""

    def __init__(self, nbytes=1 << 16):
        self.buf = (ctypes.c_ubyte * nbytes)()
        ctypes.memset(self.buf, SENTINEL, nbytes)
        self.n = nbytes
        self.p = (ctypes.addressof(self.buf) + 63) & ~63

    def untouched(self):
        return bytes(self.buf) == bytes([SENTINEL]) * self.n


def _args(p, **kw):
    from linr_pcgc_amd._lib import LinrStepArgs
    a = dict(gscale=1.0, exp_avg=p + 1024, exp_avg_sq=p + 2048, lr=0.01, step=1, scale_steps_h=None, beta1=0.9, beta2=0.999, eps=1e-8,
             weight_decay=1e-4, bits_acc=p + 3072, qparams=None, bitdepth=8)
    a.update(kw)
    return LinrStepArgs(**a)


def test_step_refusals_and_their_order(lib):
    """NULL, alignment, hidden, flags, arena size, the step's arguments, the frame, the step counters against the frame: each refusal
    is shown with the later ones present, too, and none of them writes a byte."""
    h = _Host()
    p = h.p
    need = lib.linr_net_wide_train_arena_bytes(100, 16, 1)
    assert need > 0

    def call(f, params, arena, nbytes, hidden=16, flags=0, args='good', **akw):
        fr = None if f is None else f.ref()
        a = None if args is None else ctypes.byref(_args(p, **akw))
        rc = lib.linr_net_train_step_wide(fr, params, hidden, arena, nbytes, flags, a, None)
        assert h.untouched(), 'a refused call wrote'
        return rc
    good = _Frame(100, p)
    bad_frame = _Frame(100, p, model_scale_num=0)
    # 1. NULL in front of everything (misaligned arena, bad width, bad flags, short arena, bad step, bad frame present)
    assert call(None, p, p, need) == EINVAL
    assert call(bad_frame, None, p + 4, 0, hidden=24, flags=1, step=0) == EINVAL
    assert call(good, p, None, need) == EINVAL
    assert call(good, p, p, need, args=None) == EINVAL
    # 2. alignment in front of hidden, flags, size, step
    assert call(bad_frame, p, p + 16, 0, hidden=24, flags=1, step=0) == EALIGN
    assert call(good, p, p + 32, need) == EALIGN
    # 3. hidden, 4. flags in front of the size (a short arena would be LINR_ENOSPC)
    for hidden in (8, 24, 64, 0):
        assert call(good, p, p, 0, hidden=hidden) == EINVAL
    for flags in (1, 2, 4, 8, 32, MUL_BF16 | 1, 1 << 31):
        assert call(good, p, p, 0, flags=flags) == EINVAL
    # 5. the size in front of the step's arguments and the frame
    assert call(bad_frame, p, p, need - 1, step=0) == ENOSPC
    assert call(good, p, p, 0, flags=MUL_BF16, exp_avg=None) == ENOSPC
    assert call(_Frame(100, p, block_layers=5), p, p, need) == EINVAL          # no arena of that depth
    assert call(_Frame(-1, p), p, p, need) == EINVAL
    # 6. the step's arguments in front of the frame
    for akw in (dict(step=0), dict(step=-3), dict(exp_avg=None), dict(exp_avg_sq=None), dict(bits_acc=None), dict(qparams=p),
                dict(qparams=p + 4096, bitdepth=1), dict(qparams=p + 4096, bitdepth=17)):
        assert call(bad_frame, p, p, need, **akw) == EINVAL, akw
    assert call(bad_frame, p, p, need, qparams=p + 4100) == EALIGN
    assert call(bad_frame, p + 4, p, need, qparams=p + 4096) == EALIGN          # the master is read 16 bytes at a time, too
    # 7. the frame
    assert call(bad_frame, p, p, need) == EINVAL
    assert call(_Frame(100, p, n_scales=0), p, p, need) == EINVAL
    assert call(_Frame(100, p, n_scales=17), p, p, need) == EINVAL
    assert call(_Frame(100, p, row_off_h=None), p, p, need) == EINVAL
    wrong = _Frame(100, p)
    wrong.row_off[1] = 99
    assert call(wrong, p, p, need) == EINVAL
    wrong = _Frame(100, p)
    wrong.sidx[0] = 5
    assert call(wrong, p, p, need) == EINVAL
    for field in ('nbr_lo', 'nbr_mask', 'offset_feat', 'occ', 'nbr', 'nbr8t'):          # nbr / nbr8t: the weight-gradient kernels' tables
        assert call(_Frame(100, p, **{field: None}), p, p, need) == EINVAL, field
    assert call(_Frame(100, p, nbr_ld=64), p, p, need) == EINVAL
    assert call(_Frame(100, p, occ=p + 4), p, p, need) == EALIGN
    assert call(_Frame(100, p, nbr8t=p + 4), p, p, need) == EALIGN
    # ... then the step counters against it: a negative count, a scale of this frame that has never started
    for counts in ([1, 1, -1, 1, 1], [0, 1, 1, 1, 1]):
        ts = np.asarray(counts, dtype=np.int64)
        assert call(good, p, p, need, scale_steps_h=ts.ctypes.data) == EINVAL
    # rows == 0: nothing to do, behind the checks, and nothing changes
    need0 = lib.linr_net_wide_train_arena_bytes(0, 16, 1)
    assert call(_Frame(0, p), p, p, need0) == 0
    assert call(_Frame(0, p), p, p, need0, flags=MUL_BF16, qparams=p + 4096) == 0
    assert call(_Frame(0, p), p, p, need0 - 1) == ENOSPC
    assert call(_Frame(0, p), p, p, need0, step=0) == EINVAL
    assert call(_Frame(0, p), p, p, 1 << 30, hidden=24) == EINVAL


@pytest.mark.parametrize('entry', ['forward', 'backward'])
def test_split_entry_refusals_and_their_order(lib, entry):
    h = _Host()
    p = h.p
    need = lib.linr_net_wide_train_arena_bytes(100, 32, 2)

    def call(f, params, arena, nbytes, hidden=32, flags=0, grads=p + 1024):
        fr = None if f is None else f.ref()
        if entry == 'forward':
            rc = lib.linr_net_forward_train_wide(fr, params, hidden, arena, nbytes, flags, p + 3072, None)
        else:
            rc = lib.linr_net_backward_wide(fr, params, hidden, arena, nbytes, flags, 1.0, grads, None)
        assert h.untouched(), 'a refused call wrote'
        return rc
    good = _Frame(100, p, block_layers=2)
    bad_frame = _Frame(100, p, block_layers=2, n_scales=0)
    assert call(None, p, p, need) == EINVAL
    assert call(good, None, p + 4, 0, hidden=24, flags=3) == EINVAL
    assert call(good, p, None, need) == EINVAL
    if entry == 'backward':
        assert call(good, p, p + 4, 0, hidden=24, flags=3, grads=None) == EINVAL
    assert call(bad_frame, p, p + 32, 0, hidden=24, flags=3) == EALIGN
    assert call(bad_frame, p, p, 0, hidden=8, flags=3) == EINVAL
    assert call(bad_frame, p, p, 0, flags=3) == EINVAL
    assert call(bad_frame, p, p, need - 1) == ENOSPC
    assert call(good, p, p, lib.linr_net_wide_train_arena_bytes(100, 32, 1)) == ENOSPC          # a deeper block_in needs more
    assert call(bad_frame, p, p, need, flags=MUL_BF16) == EINVAL
    for field in ('nbr_lo', 'nbr_mask', 'offset_feat', 'occ', 'nbr', 'nbr8t'):
        assert call(_Frame(100, p, block_layers=2, **{field: None}), p, p, need) == EINVAL, field
    assert call(_Frame(0, p, block_layers=2), p, p, lib.linr_net_wide_train_arena_bytes(0, 32, 2)) == 0


def test_python_switch_default():
    """WideNet.c_step: opt-in, on only with LINR_WIDE_C_STEP=1; run.py takes --qat-epochs at widths 16 / 32 with it, and refuses without."""
    from linr_pcgc_amd.wide_net import WideNet
    assert WideNet.c_step is (os.environ.get('LINR_WIDE_C_STEP', '0') == '1')


def test_run_takes_qat_epochs_for_the_wide_models_with_the_c_step(monkeypatch):
    from linr_pcgc_amd import run
    from linr_pcgc_amd.wide_net import WideNet
    monkeypatch.setattr(WideNet, 'c_step', True)
    for width in ('16', '32'):
        assert run.parse(['--qat-epochs', '1', '--hidden-channel-conv', width]).qat_epochs == 1
    monkeypatch.setattr(WideNet, 'c_step', False)
    for width in ('16', '32'):
        with pytest.raises(SystemExit):
            run.parse(['--qat-epochs', '1', '--hidden-channel-conv', width])
