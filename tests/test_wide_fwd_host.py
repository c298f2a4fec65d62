"""CPU: the host side of the wide C forward (csrc/wide_fwd.hip) and of the wide decoder scale entries (csrc/decode.hip): exports, the
wide parameter layout against the Python model, arena / workspace sizes, and every refusal with its place in the order - all of them
in front of the first launch, so nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('linr_param_count_wide', 'linr_net_wide_arena_bytes', 'linr_net_forward_wide', 'linr_net_forward_wide_bf16',
       'linr_decode_scale_wide_ws_bytes', 'linr_decode_scale_wide', 'linr_decode_scale_batch_wide_ws_bytes',
       'linr_decode_scale_batch_wide')
EINVAL, ENOSPC, EALIGN = -1, -2, -3


@pytest.fixture(scope='module')
def lib():
    from linr_pcgc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_header_and_library_export_the_new_symbols(lib):
    from linr_pcgc_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'linr_hip.h')).read()
    declared = set(re.findall(r'^LINR_API\s+[\w\s\*]+?\b(linr_\w+)\(', header, flags=re.M))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert declared == set(_lib.EXPORTS)
    assert lib.linr_abi_version() == 27          # additive exports only


@pytest.mark.parametrize('hidden', [16, 32])
def test_param_count_wide_is_the_models(lib, hidden):
    from linr_pcgc_amd.model_core import LINR_PCGC_Model
    for block_layers in (1, 2, 3, 4):
        for scale_num in (1, 5, 16):
            model = LINR_PCGC_Model({'scale_num': scale_num, 'in_channel': 7, 'hidden_channel_conv': hidden, 'block_layers': block_layers,
                                     'outstage': 8, 'instage': 1})
            assert lib.linr_param_count_wide(scale_num, block_layers, hidden) == model.flat_parameters().numel(), (scale_num, block_layers)


def test_param_count_wide_refuses_what_it_does_not_lay_out(lib):
    for hidden in (8, 24, 64, 0, -16):
        assert lib.linr_param_count_wide(5, 1, hidden) == 0
    for scale_num, block_layers in ((0, 1), (17, 1), (5, 0), (5, 5)):
        assert lib.linr_param_count_wide(scale_num, block_layers, 16) == 0


def test_arena_and_workspace_sizes(lib):
    A = lib.linr_net_wide_arena_bytes
    for bf16 in (0, 1):
        assert A(-1, 16, 1, bf16) == 0 and A(100, 8, 1, bf16) == 0 and A(100, 24, 1, bf16) == 0
        assert A(100, 16, 0, bf16) == 0 and A(100, 16, 5, bf16) == 0 and A((1 << 27) - 1, 16, 1, bf16) == 0
        assert 0 < A(0, 16, 1, bf16) < A(100, 16, 1, bf16) < A(1000, 16, 1, bf16) < A(100000, 16, 1, bf16)
        assert A(1000, 16, 1, bf16) < A(1000, 32, 1, bf16)
    assert A(0, 16, 1, 1) > A(0, 16, 1, 0)               # the de-quantised parameters and the images
    assert A(0, 16, 2, 1) > A(0, 16, 1, 1)               # ... of a deeper block_in
    # per-role blocks: a deeper block_in adds none
    assert A(100000, 16, 4, 0) == A(100000, 16, 1, 0)
    W, WB = lib.linr_decode_scale_wide_ws_bytes, lib.linr_decode_scale_batch_wide_ws_bytes
    for bf16 in (0, 1):
        assert W(100, 1, bf16, -1, 0, 8) == lib.linr_decode_scale_ws_bytes(100, 1, bf16, -1, 0)
        assert WB(100, 3, 1, bf16, -1, 0, 8) == lib.linr_decode_scale_batch_ws_bytes(100, 3, 1, bf16, -1, 0)
        for hidden in (16, 32):
            assert W(-1, 1, bf16, -1, 0, hidden) == 0 and W(100, 0, bf16, -1, 0, hidden) == 0 and W(100, 5, bf16, -1, 0, hidden) == 0
            assert W(100, 1, bf16, -2, 0, hidden) == 0 and W(100, 1, bf16, 10, -1, hidden) == 0
            assert 0 < W(100, 1, bf16, -1, 0, hidden) < W(1000, 1, bf16, -1, 0, hidden) < W(100000, 1, bf16, -1, 0, hidden)
            assert W(100, 1, bf16, 10, 8, hidden) >= W(100, 1, bf16, -1, 0, hidden) + 512
            assert WB(-1, 3, 1, bf16, -1, 0, hidden) == 0 and WB(100, 0, 1, bf16, -1, 0, hidden) == 0 and WB(100, 65, 1, bf16, -1, 0, hidden) == 0
            assert WB(1 << 26, 3, 1, bf16, -1, 0, hidden) == 0
            assert 0 < WB(100, 3, 1, bf16, -1, 0, hidden) < WB(1000, 3, 1, bf16, -1, 0, hidden)
        for hidden in (0, 12, 24, 64):
            assert W(100, 1, bf16, -1, 0, hidden) == 0 and WB(100, 3, 1, bf16, -1, 0, hidden) == 0


class _Frame:
    """A linr_frame over host memory: good enough for every check that comes in front of the first launch."""

    def __init__(self, rows, p, **kw):
        from linr_pcgc_amd._lib import LinrFrame
        self.row_off = np.asarray([0, rows], dtype=np.int64)
        self.sidx = np.asarray([0], dtype=np.int32)
        f = dict(rows=rows, n_scales=1, model_scale_num=5, block_layers=1, flags=1, row_off_h=self.row_off.ctypes.data,
                 scale_idx_h=self.sidx.ctypes.data, nbr=p, nbr_ld=(rows + 63) // 64 * 64, nbr_lo=p, nbr_mask=p, offset_feat=p, occ=p,
                 nbr8t=None)
        f.update(kw)
        self.c = LinrFrame(**f)

    def ref(self):
        return ctypes.byref(self.c)


@pytest.mark.parametrize('bf16', [0, 1])
def test_forward_refusals_and_their_order(lib, bf16):
    """NULL, alignment, hidden, stage range, arena size, then the frame: each refusal is shown with the later ones present, too."""
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 63) & ~63

    def call(f, model, arena, nbytes, hidden=16, k0=0, k1=8):
        fr = None if f is None else f.ref()
        if bf16:
            return lib.linr_net_forward_wide_bf16(fr, model, 0.0, 1.0, hidden, arena, nbytes, k0, k1, p, None, None)
        return lib.linr_net_forward_wide(fr, model, hidden, arena, nbytes, k0, k1, p, None, None)
    good = _Frame(100, p)
    need = lib.linr_net_wide_arena_bytes(100, 16, 1, bf16)
    assert need > 0
    # NULL in front of everything (misaligned arena, bad width, bad range, short arena, bad frame present)
    assert call(None, p, p, need) == EINVAL
    assert call(good, None, p + 4, 0, hidden=24, k0=3, k1=3) == EINVAL
    assert call(good, p, None, need) == EINVAL
    # alignment in front of hidden, the range and the size
    assert call(good, p, p + 16, 0, hidden=24, k0=3, k1=3) == EALIGN
    assert call(good, p, p + 32, need) == EALIGN
    # hidden and the stage range in front of the size (a short arena would be LINR_ENOSPC)
    for hidden in (8, 24, 64):
        assert call(good, p, p, 0, hidden=hidden) == EINVAL
    for k0, k1 in ((-1, 8), (0, 9), (3, 3), (5, 2)):
        assert call(good, p, p, 0, k0=k0, k1=k1) == EINVAL
    # the size in front of the frame: a frame linr_frame_layout refuses, with a short arena, is LINR_ENOSPC
    bad = _Frame(100, p, model_scale_num=0)
    assert call(bad, p, p, need - 1) == ENOSPC
    assert call(good, p, p, need - 1) == ENOSPC and call(good, p, p, 0) == ENOSPC
    assert call(_Frame(100, p, block_layers=5), p, p, need) == EINVAL          # no arena of that depth
    assert call(_Frame(-1, p), p, p, need) == EINVAL
    # ... and with the arena in order the frame is refused
    assert call(bad, p, p, need) == EINVAL
    assert call(_Frame(100, p, n_scales=0), p, p, need) == EINVAL
    assert call(_Frame(100, p, n_scales=17), p, p, need) == EINVAL
    assert call(_Frame(100, p, row_off_h=None), p, p, need) == EINVAL
    wrong = _Frame(100, p)
    wrong.row_off[1] = 99
    assert call(wrong, p, p, need) == EINVAL
    wrong = _Frame(100, p)
    wrong.sidx[0] = 5
    assert call(wrong, p, p, need) == EINVAL
    for field in ('nbr_lo', 'nbr_mask', 'offset_feat', 'occ'):
        assert call(_Frame(100, p, **{field: None}), p, p, need) == EINVAL, field
    assert call(_Frame(100, p, nbr_ld=64), p, p, need) == EINVAL
    assert call(_Frame(100, p, occ=p + 4), p, p, need) == EALIGN
    # rows == 0: nothing to do, behind the checks
    assert call(_Frame(0, p), p, p, lib.linr_net_wide_arena_bytes(0, 16, 1, bf16)) == 0
    assert call(_Frame(0, p), p, p, 0) == ENOSPC
    assert call(_Frame(0, p), p, p, 1 << 20, hidden=24) == EINVAL


def _scale_call(lib, batch, p, **kw):
    """linr_decode_scale_wide / _batch_wide on 100 rows with every argument in order unless overridden."""
    a = dict(coord=p, params=p, codes=None, streams=(ctypes.c_void_p * 24)(*([p] * 24)), lens=(ctypes.c_int64 * 24)(*([4] * 24)),
             ws=p, ws_bytes=1 << 40, p_pinned=p, s_pinned=p, child=p, cap=800, opts=None, hidden=16, block_layers=1, n=100)
    a.update(kw)
    out = (ctypes.c_int64 * 4)(7, 7, 7, 7)
    if batch:
        seg = np.asarray([0, a['n'] // 2, a['n'] // 2, a['n']], dtype=np.int64)
        rc = lib.linr_decode_scale_batch_wide(a['coord'], seg.ctypes.data, 3, 0, 5, a['block_layers'], a['params'], a['codes'], 0.0, 1.0,
                                              a['streams'], a['lens'], a['ws'], a['ws_bytes'], a['p_pinned'], a['s_pinned'], a['child'],
                                              a['cap'], out, a['opts'], a['hidden'], None)
    else:
        rc = lib.linr_decode_scale_wide(a['coord'], a['n'], 0, 5, a['block_layers'], 10, a['params'], a['codes'], 0.0, 1.0, a['streams'],
                                        a['lens'], a['ws'], a['ws_bytes'], a['p_pinned'], a['s_pinned'], a['child'], a['cap'], out, a['opts'],
                                        a['hidden'], None)
    return rc, list(out)


@pytest.mark.parametrize('batch', [False, True])
def test_scale_entry_refusals_and_their_order(lib, batch):
    """LINR_EINVAL, then LINR_EALIGN, then LINR_ENOSPC, as for width 8 - and a width that is none is LINR_EINVAL in front of them."""
    from linr_pcgc_amd._lib import LinrDecodeOpts
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 255) & ~255
    for hidden in (0, 12, 24, 64):
        assert _scale_call(lib, batch, p, hidden=hidden, ws=p + 8, ws_bytes=0)[0] == EINVAL
    assert _scale_call(lib, batch, p, block_layers=0)[0] == EINVAL
    for bad in (dict(coord=None), dict(params=None), dict(streams=None), dict(lens=None), dict(ws=None), dict(p_pinned=None),
                dict(s_pinned=None)):
        rc, out = _scale_call(lib, batch, p, ws_bytes=0, **({} if 'ws' in bad else dict(ws=p + 8)), **bad)
        assert rc == EINVAL, bad          # (a misaligned, short workspace present)
        assert out[0] == 0
    assert _scale_call(lib, batch, p, ws=p + 8, ws_bytes=0)[0] == EALIGN
    assert _scale_call(lib, batch, p, ws=p + 128, ws_bytes=0)[0] == EALIGN
    for codes in (None, p):          # fp32 parameters / the uint8 codes: another arena, the same order
        kw = dict(codes=codes, params=None if codes else p)
        bf16 = 1 if codes else 0
        need = (lib.linr_decode_scale_batch_wide_ws_bytes(100, 3, 1, bf16, -1, 0, 16) if batch else
                lib.linr_decode_scale_wide_ws_bytes(100, 1, bf16, -1, 0, 16)) - 256
        assert _scale_call(lib, batch, p, ws_bytes=0, **kw)[0] == ENOSPC
        assert _scale_call(lib, batch, p, ws_bytes=need - 1, **kw)[0] == ENOSPC
        assert _scale_call(lib, batch, p, ws_bytes=need - 1, hidden=32, **kw)[0] == ENOSPC
    # the device decoders take no pinned buffers; their workspace is larger
    dev = ctypes.pointer(LinrDecodeOpts(0, 1, 1))
    host_need = (lib.linr_decode_scale_batch_wide_ws_bytes(100, 3, 1, 0, -1, 0, 16) if batch else
                 lib.linr_decode_scale_wide_ws_bytes(100, 1, 0, -1, 0, 16)) - 256
    assert _scale_call(lib, batch, p, opts=dev, p_pinned=None, s_pinned=None, ws_bytes=host_need)[0] == ENOSPC
    # a chunk size that is none is refused by the plan, in front of the first launch
    assert _scale_call(lib, batch, p, opts=ctypes.pointer(LinrDecodeOpts(100, 1, 0)))[0] == EINVAL
    # no rows: nothing to do, whatever the pointers are
    rc, out = _scale_call(lib, batch, p, n=0, coord=None, params=None, ws=None)
    assert rc == 0 and out[0] == 0
