"""CPU: the C-ABI and command-line face of the bf16 training executor at block_layers 1..4 (linr_net_*_bf16, csrc/train_bf16.hip;
run.py --train-precision bf16-deep, the opt-in above block_layers 1).  Every call below is refused in front of the first launch, so
nothing here needs a GPU."""
import ctypes
import os

import pytest


@pytest.fixture(scope='module')
def lib():
    from linr_pcgc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_deep_arena_bytes(lib):
    deep = lib.linr_net_train_bf16_arena_bytes
    assert deep(-1, 1) == 0 and deep(-1, 3) == 0
    assert deep(100, 0) == 0 and deep(100, 5) == 0
    # block_layers 1: the figures of the executor before it took deeper models, byte for byte
    one_layer = {0: 119802432, 1: 119802624, 100: 119960640, 6821: 130606912, 337000: 653694720}
    for rows in (0, 1, 100, 6821, 337000):
        assert deep(rows, 1) == one_layer[rows]
        sizes = [deep(rows, bl) for bl in (1, 2, 3, 4)]
        assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes
    # an extra layer: eight weight images (64 lanes x 8 bytes), its parameters in the slab (512 rows) and the flat gradient, five
    # matrices of 16-byte rows and one of 8-byte rows (each with its zero row, rounded up to 64 bytes)
    per_layer = 27 * 8 * 4 + 4 + 2 * (27 * 4 * 4 + 4) + 8 * 4 + 4 + 4 * 4 + 4
    up64 = lambda n: (n + 63) // 64 * 64
    for bl in (2, 3, 4):
        p0, p1 = lib.linr_param_count(16, bl - 1), lib.linr_param_count(16, bl)
        assert p1 - p0 == per_layer
        want = (8 * 64 * 8 + (up64(p1 * 4) - up64(p0 * 4)) + (up64(512 * p1 * 4) - up64(512 * p0 * 4))
                + 5 * up64(101 * 16) + up64(101 * 8))
        assert deep(100, bl) - deep(100, bl - 1) == want, (bl, deep(100, bl) - deep(100, bl - 1), want)
    assert deep(100, 2) == 123659264, 'what the entry for deeper models returned before the two were merged'


def test_deep_entries_check_their_arguments_like_their_namesakes(lib):
    from linr_pcgc_amd._lib import LinrFrame
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    p16 = (p + 15) & ~15
    p64 = (p + 63) & ~63
    keep = []

    def frame(rows=16, n_scales=2, row_off=(0, 8, 16), sidx=(0, 1), msn=7, bl=1, cmap=True, mask=True, feat=p64, occ=p64):
        ro, si = (ctypes.c_int64 * 18)(*row_off), (ctypes.c_int32 * 17)(*sidx)
        f = LinrFrame(rows, n_scales, msn, bl, 0, ctypes.addressof(ro), ctypes.addressof(si), p64, rows,
                      p64 if cmap else None, p64 if cmap and mask else None, feat, occ, None)
        keep.append((ro, si, f))
        return ctypes.byref(f)

    # NULL frame / parameters / arena
    from linr_pcgc_amd._lib import LinrStepArgs
    sargs = lambda m=p64, v=p64, bits=p64, step=1, steps=None, q=None, depth=0: ctypes.byref(
        LinrStepArgs(1.0, m, v, 0.01, step, steps, 0.9, 0.999, 1e-8, 0.0, bits, q, depth))
    assert lib.linr_net_train_step_bf16(None, p16, p16, 4096, None, sargs(None, None, None), None) == -1
    assert lib.linr_net_forward_train_bf16(None, p16, p16, 4096, None, None, None, None) == -1
    assert lib.linr_net_backward_bf16(None, p16, p16, 4096, None, 1.0, None, None) == -1
    tfwd = lambda f, a, nb: lib.linr_net_forward_train_bf16(f, p64, a, nb, None, None, None, None)
    tbwd = lambda f, a, nb: lib.linr_net_backward_bf16(f, p64, a, nb, None, 1.0, p64, None)
    tstep = lambda f, a, nb: lib.linr_net_train_step_bf16(f, p64, a, nb, None, sargs(), None)
    bound = (1 << 27) - 1
    faults = [dict(n_scales=0), dict(n_scales=17, rows=17, row_off=range(18), sidx=[0] * 17), dict(row_off=(1, 8, 16)),
              dict(n_scales=3, row_off=(0, 12, 8, 16), sidx=(0, 1, 2)), dict(row_off=(0, 8, 15)), dict(sidx=(0, 7)), dict(sidx=(-1, 1)),
              dict(bl=5), dict(rows=bound, row_off=(0, 8, bound)), dict(cmap=False), dict(mask=False), dict(feat=None), dict(occ=None)]
    need = lib.linr_net_train_bf16_arena_bytes
    for call in (tfwd, tbwd, tstep):
        for fault in faults:
            assert call(frame(**fault), p64, 1 << 40) == -1, fault
            assert call(frame(**fault), p64 + 4, 0) == -1, fault                                # EINVAL before ENOSPC / EALIGN
        assert call(frame(), None, 1 << 40) == -1
        for bl in (0, 1, 2, 3, 4):                                                              # 0 is read as 1
            n16 = need(16, max(bl, 1))
            assert call(frame(bl=bl), p64, n16 - 1) == -2                                       # short arena
            assert call(frame(bl=bl), p64 + 4, n16 - 1) == -2                                   # ENOSPC before EALIGN
            assert call(frame(bl=bl), p64 + 16, n16) == -3                                      # misaligned arena
        assert call(frame(bl=2), p64, need(16, 1)) == -2                                        # the depth is the frame's
        assert call(frame(rows=bound - 1, row_off=(0, 8, bound - 1), bl=3), p64, need(16, 3)) == -2          # one row below the bound: accepted
        assert call(frame(rows=0, row_off=(0, 0, 0), bl=5), p64, 1 << 40) == -1
    assert lib.linr_net_forward_train_bf16(frame(bl=2), p64, p64, need(16, 2), p64 + 4, None, None, None) == -3       # occ_bf16
    assert lib.linr_net_backward_bf16(frame(bl=2), p64, p64, need(16, 2), None, 1.0, None, None) == -1                # no grads
    # the step: the struct, moments, bits, step >= 1, scale_steps, the QAT image (tests/test_cpu_host.py: the same on both executors)
    assert lib.linr_net_train_step_bf16(frame(bl=2), p64, p64, need(16, 2), None, None, None) == -1
    step = lambda **kw: lib.linr_net_train_step_bf16(frame(bl=2), p64, p64, need(16, 2), None, sargs(**kw), None)
    assert step(m=None) == -1 and step(v=None) == -1 and step(bits=None) == -1 and step(step=0) == -1
    assert step(q=p64, depth=8) == -1, 'the fake-quantised image must not alias the master'
    assert step(q=p64 + 2048, depth=0) == -1 and step(q=p64 + 2048, depth=17) == -1
    never = (ctypes.c_int64 * 7)(0, 0, 0, 0, 0, 0, 0)
    assert step(steps=ctypes.addressof(never)) == -1, 'a scale with rows cannot be "never started"'
    neg = (ctypes.c_int64 * 7)(1, 1, -1, 1, 1, 1, 1)
    assert step(steps=ctypes.addressof(neg)) == -1


def test_without_deep_python_refuses_deeper_models_before_any_library_call(monkeypatch):
    """The entries take the frame's block_layers; that 'bf16' and deep=False stay at block_layers 1 is decided in Python, in front of
    the library (which this test takes away)."""
    import types
    from linr_pcgc_amd import _lib, engine, model_core, overfit

    def no_library():
        raise AssertionError('the refusal must come before the library is touched')
    monkeypatch.setattr(_lib, 'lib', no_library)
    only_one = "the bf16 training executor supports block_layers=1 only (train_precision 'bf16-deep': 1..4)"
    frame = engine.Frame.__new__(engine.Frame)
    frame.block_layers, frame.rows = 2, 16
    with pytest.raises(_lib.LinrError) as e:
        frame.train_bf16_arena()
    assert str(e.value) == only_one
    gop = overfit.Gop.__new__(overfit.Gop)
    gop.block_layers, gop.frames = 2, [frame]
    with pytest.raises(_lib.LinrError) as e:
        gop.share_train_bf16_arena()
    assert str(e.value) == only_one
    for fn in (engine.net_forward_train_bf16, engine.net_backward_bf16, engine.net_train_step_bf16):
        with pytest.raises(_lib.LinrError) as e:
            fn(frame, *[None] * (12 if fn is engine.net_train_step_bf16 else 3 if fn is engine.net_backward_bf16 else 1))
        assert str(e.value) == only_one
    model = types.SimpleNamespace(_wide=None, train_precision='bf16', block_layers=2)
    opt = types.SimpleNamespace(advance=lambda f: (1, None))
    with pytest.raises(_lib.LinrError) as e:
        model_core.train_step(model, opt, frame, 100, out=object())
    assert str(e.value) == 'the bf16 training executor supports block_layers=1 only'


def test_run_train_precision_bf16_deep():
    from linr_pcgc_amd import run
    assert run.train_precision(run.parse(['--train-precision', 'bf16-deep', '--block_layers', '3'])) == 'bf16-deep'
    assert run.train_precision(run.parse(['--train_precision', 'bf16-deep'])) == 'bf16-deep'
    assert run.train_precision(run.parse(['--precision', 'bf16', '--block_layers', '3'])) == 'f32', 'the default rule never picks it'
    with pytest.raises(SystemExit):
        run.parse(['--train-precision', 'bf16-deeper'])


def test_train_step_names_the_precisions_it_knows():
    """model_core.train_step: an unknown train_precision is a ValueError that names 'bf16-deep'; no GPU is touched before it."""
    import inspect
    from linr_pcgc_amd import engine, model_core, overfit
    assert "'bf16-deep'" in inspect.getsource(model_core.train_step)
    for fn in (engine.net_forward_train_bf16, engine.net_backward_bf16, engine.net_train_step_bf16, engine.Frame.train_bf16_arena,
               overfit.Gop.share_train_bf16_arena):
        assert inspect.signature(fn).parameters['deep'].default is False, fn
