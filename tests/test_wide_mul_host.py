"""CPU: the host side of train_precision 'bf16-mul' (bf16 products in the wide models' 3x3x3 convolutions, csrc/wide_mul.hip) - the
flag's argument checks at the C-ABI, train_step's refusals and run.py's option.  Nothing is launched here."""
import ctypes
import os
import types

import pytest

from linr_pcgc_amd import _lib

MUL = 16          # LINR_MUL_BF16


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope='module')
def p16():
    buf = (ctypes.c_char * 4096)()
    p = ((ctypes.addressof(buf) + 15) & ~15)
    yield p
    del buf


def test_abi_declares_the_flag_and_one_entry_per_wide_op(lib):
    assert _lib.ABI_VERSION == 27 and lib.linr_abi_version() == 27
    assert _lib.LINR_MUL_BF16 == MUL
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'linr_hip.h')).read()
    assert '#define LINR_MUL_BF16 16u' in header and '#define LINR_ABI_VERSION 27' in header
    for name in ('linr_spconv_wide', 'linr_spconv_wgrad_wide', 'linr_spconv_wgrad_wide2'):          # each takes the flags word itself
        assert name in _lib.EXPORTS and hasattr(lib, name) and name + '(' in header
    for name in ('linr_spconv_wide_pw', 'linr_spconv_wgrad_wide_f', 'linr_spconv_wgrad_wide2_f'):   # ABI 26's twins are gone
        assert name not in _lib.EXPORTS and name not in header and not hasattr(lib, name)


def test_conv_entries_take_flag_16_and_still_refuse_every_other_bit(lib, p16):
    b2 = (ctypes.c_void_p * 2)(p16, p16)
    pw = _lib.LinrWidePw(1, p16, p16, None, ctypes.cast(b2, ctypes.c_void_p))
    conv = lambda cout, flags, n=16: lib.linr_spconv_wide(0, b2, p16, p16, 16, n, p16, p16, 16, cout, None, None, b2, flags, None, None)
    conv_pw = lambda cout, flags, n=16: lib.linr_spconv_wide(0, b2, p16, p16, 16, n, p16, p16, 16, cout, None, None, b2, flags,
                                                              ctypes.byref(pw), None)
    for entry, cout in ((conv, 16), (conv_pw, 8)):
        for flags in (64, MUL | 64, 32):
            assert entry(cout, flags) == -1, flags
        assert entry(12, MUL) == -1                    # the argument's own code: cout is no multiple of 8
    b2m = (ctypes.c_void_p * 2)(p16, p16 + 4)
    # flag 16 passes the flags check: a later check answers (a misaligned gathered block: LINR_EALIGN, not the flag's LINR_EINVAL)
    for flags in (MUL, MUL | 1 | 2):
        assert lib.linr_spconv_wide(0, b2m, p16, p16, 16, 16, p16, p16, 16, 16, None, None, b2, flags, None, None) == -3
    assert lib.linr_spconv_wide(0, b2, p16, p16, 16, 16, p16, p16, 16, 16, None, None, b2, MUL | 4, None, None) == -1    # mask without act


def test_wgrad_entries_with_flags_refuse_every_bit_but_16_and_what_the_old_entries_refuse(lib, p16):
    b2 = (ctypes.c_void_p * 2)(p16, p16)
    b2m = (ctypes.c_void_p * 2)(p16 + 4, p16 + 4)
    wg = lambda flags, cout=16, slab=p16, tile=p16, n=16: lib.linr_spconv_wgrad_wide(b2, 16, b2, cout, p16, tile, 16, n, slab, p16, p16,
                                                                                     flags, None)
    wg2 = lambda flags, h=8, n=16, a=b2: lib.linr_spconv_wgrad_wide2(a, b2, b2, b2, h, p16, n, p16, flags, None)
    for bit in range(32):
        if (1 << bit) != MUL:
            assert wg(1 << bit) == -1 and wg(MUL | (1 << bit)) == -1, bit
            assert wg2(1 << bit) == -1 and wg2(MUL | (1 << bit)) == -1, bit
    for flags in (0, MUL):
        assert wg(flags, cout=5) == -1                 # cout 5
        assert wg(flags, slab=None) == -1              # no slab
        assert wg2(flags, h=12) == -1                  # h is 8 or 16
        assert wg2(flags, n=0) == -1                   # partials need rows
        assert wg2(flags, a=b2m) == -3                 # a misaligned input block
    # the bf16 products exist in the one-launch form only: without the tiled table there is nothing to fall back to
    assert wg(MUL, tile=None) == -1 and wg(MUL, cout=24) == -1
    # n == 0 launches nothing: zeroed gradients, as without the flag (checked on the host: the memsets would need a device)
    assert lib.linr_spconv_wgrad_wide(b2, 16, b2, 16, p16, p16, 16, 0, p16, None, p16, MUL, None) == -1      # deferred + no rows


def _fake_model(wide, tp):
    return types.SimpleNamespace(_wide=object() if wide else None, train_precision=tp, block_layers=1)


def test_train_step_refusals_come_before_any_library_call(monkeypatch):
    """wide + 'bf16' / 'bf16-deep': today's LinrError; width 8 + 'bf16-mul': LinrError; an unknown name: ValueError that lists every
    name.  The library is made unloadable and frame / optimiser are None: a refusal that came after any call or allocation would fail
    differently."""
    from linr_pcgc_amd import model_core

    def no_lib():
        raise AssertionError('the library was called before the refusal')
    monkeypatch.setattr(_lib, 'lib', no_lib)
    for tp in ('bf16', 'bf16-deep'):
        with pytest.raises(_lib.LinrError, match='the bf16 training executor exists for hidden_channel_conv=8 only'):
            model_core.train_step(_fake_model(True, tp), None, None, 1000)
    with pytest.raises(_lib.LinrError, match="'bf16-mul' exists for hidden_channel_conv 16 / 32 only"):
        model_core.train_step(_fake_model(False, 'bf16-mul'), None, None, 1000)
    for wide in (False, True):
        with pytest.raises(ValueError) as e:
            model_core.train_step(_fake_model(wide, 'fp16'), None, None, 1000)
        for name in ('f32', 'bf16', 'bf16-deep', 'bf16-mul'):
            assert repr(name) in str(e.value)


def test_ops_mul_names():
    from linr_pcgc_amd import ops
    assert ops._mul_flag('f32') == 0 and ops._mul_flag('bf16') == MUL
    with pytest.raises(ValueError):
        ops._mul_flag('fp16')


def test_run_parser_takes_bf16_mul_and_the_default_rule_never_picks_it():
    from linr_pcgc_amd import run
    args = run.parse(['--hidden-channel-conv', '16', '--train-precision', 'bf16-mul'])
    assert args.train_precision == 'bf16-mul' and run.train_precision(args) == 'bf16-mul'
    for hidden in ('16', '32'):
        for prec in ('f32', 'bf16'):
            args = run.parse(['--hidden-channel-conv', hidden, '--precision', prec])
            assert run.train_precision(args) == 'f32'
    assert run.train_precision(run.parse(['--precision', 'bf16'])) == 'bf16'          # width 8: as before
    with pytest.raises(SystemExit):
        run.parse(['--train-precision', 'bf16-mull'])


def test_a_pass_multiplies_in_bf16_only_while_training_a_bf16_mul_model():
    """What a pass multiplies in is a field of the pass object that forward / backward build per call (WideNet._pass): 'bf16' in the
    training passes of a 'bf16-mul' model, 'f32' in its other forwards and in every pass of a model that did not ask."""
    import torch
    from linr_pcgc_amd import wide_net
    frame = types.SimpleNamespace(nbr_lo=None, nbr_mask=None, nbr=None, nbr8t=None, rows=3, occ=torch.zeros(3, 8))
    net = wide_net.WideNet(types.SimpleNamespace(train_precision='bf16-mul'), 16)
    assert net._pass(frame, True, False).mul == 'bf16'                      # forward(keep=True)
    assert net._pass(frame, False, False).mul == 'f32'                      # forward(keep=False): codec, decoder, probabilities
    back = net._pass(frame, True, False, defer=[])                          # backward
    assert back.mul == 'bf16' and back.defer == [] and net._pass(frame, True, False).defer is None
    net.model.train_precision = 'f32'
    for training in (True, False):
        assert net._pass(frame, training, False).mul == 'f32'
        assert net._pass(frame, training, False, defer=[]).mul == 'f32'
    # a pass is its own object: nothing of it stays on the executor, and a fresh-buffer pass hands out zero-padded blocks of the frame
    assert back.pool is None and back.n == 3 and not {'lo', 'mask', 'nbr', 'tile8t', 'n', 'mul', 'defer'} & set(vars(net))
    blk = back.blocks(2)
    assert len(blk) == 2 and all(b.shape == (3, 8) and not b._base[:, 0].any() for b in blk)
