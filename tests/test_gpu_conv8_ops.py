"""Every entry of the width-8 fp32 convolution family (csrc/fused.hip, fused_bwd.hip + fused_bwd_split.h, wgrad.hip, occ_wgrad.hip,
spconv.hip) at op level against float64, on tiny clouds chosen for what the kernels do with them: linr_spconv_cmap forward and backward,
linr_spconv_fwd / _bwd_data, linr_spconv_bwd_weight, linr_spconv_wgrad_cmap (three index sources), linr_spconv_bwd_fused,
linr_inception_fwd / _bwd_data / _bwd_fused, linr_spconv_wgrad_dual44, linr_occ_conv7, linr_occ_wgrad7 and linr_slab_reduce, through the
public C entries only.

The clouds, the inputs, the float64 references and the criterion are in tests/conv8_ref.py (checked without a GPU by
tests/test_conv8_ref.py): every produced entry within gpu_common._within_rounding (64 x 2^-24 x the same sum over absolute values) of the
float64 value of its own sum; where one call has several outputs, each is checked from the device's own earlier outputs.  On every cloud
the library's kernel map must equal oracle.octree.neighbour_table, linr_kmap_compress must decode back to it and linr_kmap_tile8t must
match the header's formula before anything else runs.  Each cloud runs with map ld = n and ld = the next multiple of 64.

Nothing else is touched: every output, slab and scratch buffer starts as NaN; afterwards the row in front of every output (the pad row at
index -1), the rows from n on, the channels beyond the produced width and the slab rows beyond the written ones must still be NaN.  Outputs
that the entry itself gathers in a later launch (H of linr_inception_fwd; gM, gH of linr_inception_bwd_data; gH of _bwd_fused) need their
zero row: it must still be zero.  Every slab row of the fused backward entries must be finite.  Every input keeps its bits, and every entry
runs once more behind linr_debug_poison_now and must give the same bits.  The gather, compressed-map and fused forms, the index sources of
the weight gradients and the two fused-backward kernels (LINR_FUSED_SPLIT) must agree bit for bit.

Measured on the MI355X (test_zz_figures_of_this_run prints these): the 283 test cases make 19,422 checks in 8.4 s, all pass, also under
LINR_DEBUG_POISON=1: no kernel bug found.  Worst entry per entry kind as a fraction of its bound: linr_spconv_cmap forward 0.071, backward
0.075; linr_spconv_bwd_weight 0.037; linr_spconv_wgrad_cmap 0.037; linr_spconv_bwd_fused gin 0.048, slab 0.035; linr_inception_fwd 0.060;
linr_inception_bwd_data 0.047; linr_inception_bwd_fused slab 0.035; linr_spconv_wgrad_dual44 0.022; linr_occ_conv7 0.045; linr_occ_wgrad7
0.040; linr_slab_reduce 0.047.  linr_spconv_fwd / _bwd_data, the second fused-backward kernel and the other index sources gave the bits of
the entry they are compared with everywhere.  On the CPU (tests/test_conv8_ref.py) a weight gradient that drops its last 8-row group, the
last tile of a wave or one row of the bias sum lands far above 1 on the clouds named there."""
import ctypes
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import conv8_ref as cr                      # noqa: E402

pytestmark = pytest.mark.gpu

TAIL = 3                                    # NaN rows behind row n - 1 of every output
NAN = float('nan')
WORST = {}                                  # entry kind -> worst ratio to the bound seen in this run
COUNT = {'cases': 0}
T0 = time.time()


def _note(kind, ratio):
    WORST[kind] = max(WORST.get(kind, 0.0), ratio)
    COUNT['cases'] += 1


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cu(v):
    if torch.is_tensor(v):
        return v.cuda().contiguous()
    if isinstance(v, dict):
        return {k: _cu(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_cu(x) for x in v]
    return v


_DEV = {}


def _case(fn, *args):
    """A case of conv8_ref on the device (made once)."""
    if (fn, args) not in _DEV:
        _DEV[(fn, args)] = _cu(fn(*args))
    return _DEV[(fn, args)]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- matrices ---------------------------------------------------------------------------------------------------------------------------------------
def _in(t, ld=None, col=0, other=None):
    """Device tensor [n, c] -> a gathered operand: buffer [n + 1, ld] whose row 0 is the zero row (LINR_PAD_ROW contract), t in channels
    col .. col + c - 1, zeros (or `other`) in the rest.  Returns (buffer, pointer of row 0 of t)."""
    n, c = t.shape
    ld = c if ld is None else ld
    buf = torch.zeros((n + 1, ld), device='cuda')
    if other is not None:
        buf[1:, :other.shape[1]] = other
    buf[1:, col:col + c] = t
    return buf, buf[1:, col:].data_ptr()


def _out(n, ld, width, old=None, pad_zero=False):
    """A NaN-filled output [1 + n + TAIL, ld]; rows 1 .. n, channels 0 .. width - 1 are the entry's (pre-filled with `old` for LINR_ACCUM);
    pad_zero: the entry gathers this output itself and needs its zero row."""
    buf = torch.full((n + 1 + TAIL, ld), NAN, device='cuda')
    if pad_zero:
        buf[0] = 0.0
    if old is not None:
        buf[1:n + 1, :width] = old
    return buf


def _own(buf, n, width):
    return buf[1:n + 1, :width]


def _untouched(buf, n, width, what, pad_zero=False):
    b = buf.clone()
    b[1:n + 1, :width] = NAN
    if pad_zero:
        assert bool((buf[0].view(torch.int32) == 0).all()), what + ': the zero row in front is no longer zero'
        b[0] = NAN
    assert bool(torch.isnan(b).all()), '%s: %d elements written outside rows 0 .. n - 1 x the produced width' % (what, int((~torch.isnan(b)).sum()))


def _twice(call, outs, ins, what):
    """call() once, then once more on the same initial outputs behind linr_debug_poison_now: the same bits; the inputs keep theirs."""
    from linr_pcgc_amd import _lib
    init = [o.clone() for o in outs]
    keep = [i.clone() for i in ins]
    call()
    first = [o.clone() for o in outs]
    for o, i in zip(outs, init):
        o.copy_(i)
    _lib.check(_lib.lib().linr_debug_poison_now(_stream()), 'linr_debug_poison_now')
    call()
    for o, f in zip(outs, first):
        assert _bits_equal(o, f), what + ': other bits behind poisoned on-chip state'
    for i, k in zip(ins, keep):
        assert _bits_equal(i, k), what + ': an input was written'


class _single_stream:
    """LINR_FUSED_SPLIT=0 for the launches inside: conv_bwd_wgrad_single_k instead of the wave-specialised conv_bwd_wgrad_k."""
    def __enter__(self):
        self.old = os.environ.get('LINR_FUSED_SPLIT')
        os.environ['LINR_FUSED_SPLIT'] = '0'

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ['LINR_FUSED_SPLIT']
        else:
            os.environ['LINR_FUSED_SPLIT'] = self.old


# ---- maps -------------------------------------------------------------------------------------------------------------------------------------------
_MAPS = {}


def _maps(key, padded):
    """The library's maps of a cloud with ld = n or the next multiple of 64, each checked against its definition (made once)."""
    if (key, padded) not in _MAPS:
        from linr_pcgc_amd import ops
        c = cr.cloud(key)
        n = c['n']
        ld = cr.padded_ld(n) if padded else n
        built = ops.kmap_build(torch.from_numpy(c['coord']).cuda().contiguous())
        assert torch.equal(built.t().long().cpu(), c['nbr']), key + ': kernel map and oracle table differ'
        nbr = torch.full((27, ld), -1, dtype=torch.int32, device='cuda')
        nbr[:, :n] = built
        lo, mask = ops.kmap_compress(nbr, n)
        assert lo.stride(0) == ld
        assert torch.equal(cr.decode_cmap(lo[:, :n], mask[:n]), built), key + ': the compressed map does not decode to the table'
        t8 = None
        if padded:
            t8 = ops.kmap_tile8t(nbr, n)
            want = torch.from_numpy(cr.tile8t_ref(nbr.cpu().numpy(), n))
            assert t8.numel() == want.numel() and torch.equal(t8.cpu(), want), key + ': linr_kmap_tile8t differs from the header\'s formula'
        _MAPS[(key, padded)] = {'n': n, 'ld': ld, 'nbr': nbr, 'lo': lo, 'mask': mask, 't8': t8, 'tab': c['nbr'].cuda()}
    return _MAPS[(key, padded)]


@pytest.mark.parametrize('key', cr.ALL_CLOUDS)
def test_maps_equal_their_definitions(pkg, key):
    """linr_kmap_build == oracle.octree.neighbour_table, linr_kmap_compress decodes back to it, linr_kmap_tile8t is the header's formula
    with its -1 fill (position 27, j = 7, rows past n, the spare groups); both layouts."""
    for padded in (False, True):
        _maps(key, padded)


# ---- linr_slab_reduce ---------------------------------------------------------------------------------------------------------------------------------
def _check_reduce(slab, rows, split, what, full=True):
    """linr_slab_reduce over the first `rows` rows of a slab [.., elems]: both destinations, either one NULL, LINR_ACCUM - each fp32 result
    within the bound of the float64 sum of the same slab rows (absum = the sum of |slab|); nothing behind the destinations is written."""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    elems = slab.shape[1]
    exact, absum = cr.slab_ref(slab[:rows])
    gen = torch.Generator().manual_seed(rows + elems)
    old = torch.randn(elems, generator=gen).cuda()
    for a_on, b_on, accum in ([(True, True, False), (True, False, False), (False, True, False), (True, True, True)] if full else [(True, True, False)]):
        dA = torch.full((split + 1,), NAN, device='cuda')
        dB = torch.full((elems - split + 1,), NAN, device='cuda')
        if accum:
            dA[:split], dB[:elems - split] = old[:split], old[split:]

        def call():
            _lib.check(L.linr_slab_reduce(slab.data_ptr(), rows, elems, split, dA.data_ptr() if a_on else None, dB.data_ptr() if b_on else None,
                                          _lib.LINR_ACCUM if accum else 0, _stream()), 'linr_slab_reduce')
        _twice(call, [dA, dB], [slab], what + ': linr_slab_reduce')
        e, a = (exact + old.double(), absum + old.double().abs()) if accum else (exact, absum)
        tag = '%s: linr_slab_reduce of %d rows%s' % (what, rows, ', LINR_ACCUM' if accum else '')
        if a_on:
            assert bool(torch.isnan(dA[split:]).all())
            if split:
                _note('slab_reduce', cr._within_rounding(dA[:split], e[:split], a[:split], tag + ', dstA'))
        else:
            assert bool(torch.isnan(dA).all()), tag + ': a NULL destination\'s neighbour was written'
        if b_on:
            assert bool(torch.isnan(dB[elems - split:]).all())
            _note('slab_reduce', cr._within_rounding(dB[:elems - split], e[split:], a[split:], tag + ', dstB'))
        else:
            assert bool(torch.isnan(dB).all())


def _slab_sum_ok(slab, rows, exact, absum, kind, what):
    """The written slab rows are finite, the rows behind them still NaN, their float64 sum within the bound."""
    assert bool(torch.isfinite(slab[:rows]).all()), '%s: %d slab entries never written' % (what, int((~torch.isfinite(slab[:rows])).sum()))
    assert bool(torch.isnan(slab[rows:]).all()), what + ': slab rows behind the written ones were touched'
    _note(kind, cr._within_rounding(slab[:rows].double().sum(0), exact, absum, what))


# ---- forward ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', cr.ALL_CLOUDS)
def test_forward_convolutions(pkg, key):
    """linr_spconv_cmap forward: (cin, cout) in (8,8), (8,4), (4,4), (1..7, 8) x none / LINR_RELU / res / res + LINR_RELU; cout 4 into an 8-wide
    matrix; a 4-channel slice of an 8-wide matrix in and out.  linr_spconv_fwd with and without LINR_PAD_ROW: the same bits."""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    for padded in (False, True):
        m = _maps(key, padded)
        n, tab = m['n'], m['tab']
        for cin, cout, layout in cr.FWD_LAYOUTS:
            t = _case(cr.fwd_case, key, cin, cout)
            if layout == 'slice':
                xbuf, xp = _in(t['x'], 8, col=4, other=t['other'])
            else:
                xbuf, xp = _in(t['x'], 4 if cin == 4 else 8)
            in_ld = xbuf.shape[1]
            out_ld = cout if layout == 'tight' else 8
            for form in (cr.FWD_FORMS if layout == 'tight' else ('none', 'res_relu')):
                res = t['res'] if 'res' in form else None
                flags = _lib.LINR_RELU if 'relu' in form else 0
                what = 'forward %d -> %d %s %s on %s, ld %d' % (cin, cout, layout, form, key, m['ld'])
                out = _out(n, out_ld, cout)
                ins = [xbuf, t['W'], t['b']] + ([res] if res is not None else [])
                rargs = (None, 0) if res is None else (res.data_ptr(), cout)

                def cmap():
                    _lib.check(L.linr_spconv_cmap(0, xp, in_ld, m['lo'].data_ptr(), m['mask'].data_ptr(), m['ld'], n, t['W'].data_ptr(),
                                                  t['b'].data_ptr(), cin, cout, rargs[0], rargs[1], None, 0, out[1:].data_ptr(), out_ld,
                                                  flags | _lib.LINR_PAD_ROW, _stream()), 'linr_spconv_cmap')
                _twice(cmap, [out], ins, what)
                _untouched(out, n, cout, what)
                e, a, _ = cr.fwd_ref(t['x'], tab, t['W'], t['b'], res=res, relu='relu' in form)
                _note('spconv_cmap forward', cr._within_rounding(_own(out, n, cout), e, a, what))
                for pad in (_lib.LINR_PAD_ROW, 0):
                    out2 = _out(n, out_ld, cout)

                    def gather():
                        _lib.check(L.linr_spconv_fwd(xp, in_ld, m['nbr'].data_ptr(), m['ld'], n, t['W'].data_ptr(), t['b'].data_ptr(), cin, cout,
                                                     rargs[0], rargs[1], out2[1:].data_ptr(), out_ld, flags | pad, _stream()), 'linr_spconv_fwd')
                    _twice(gather, [out2], ins, what + ' (linr_spconv_fwd)')
                    assert _bits_equal(out, out2), what + ': linr_spconv_fwd (pad_row %d) and linr_spconv_cmap differ' % pad
                    COUNT['cases'] += 1


# ---- backward-data ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', cr.ALL_CLOUDS)
def test_backward_data_convolutions(pkg, key):
    """linr_spconv_cmap backward: (8,8), (8,4), (4,4) x none / LINR_ACCUM / LINR_RELU_MASK / both; linr_spconv_bwd_data the same bits."""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    for padded in (False, True):
        m = _maps(key, padded)
        n, tab = m['n'], m['tab']
        for cin, cout in cr.BWD_SHAPES:
            t = _case(cr.bwd_case, key, cin, cout)
            gbuf, gp = _in(t['g'])
            for form in cr.BWD_FORMS:
                old = t['old'] if 'accum' in form else None
                act = t['act'] if 'mask' in form else None
                flags = (_lib.LINR_ACCUM if old is not None else 0) | (_lib.LINR_RELU_MASK if act is not None else 0)
                what = 'backward-data %d -> %d %s on %s, ld %d' % (cin, cout, form, key, m['ld'])
                out = _out(n, cin, cin, old=old)
                ins = [gbuf, t['W']] + ([act] if act is not None else [])
                aargs = (None, 0) if act is None else (act.data_ptr(), cin)

                def cmap():
                    _lib.check(L.linr_spconv_cmap(1, gp, cout, m['lo'].data_ptr(), m['mask'].data_ptr(), m['ld'], n, t['W'].data_ptr(), None, cin,
                                                  cout, None, 0, aargs[0], aargs[1], out[1:].data_ptr(), cin, flags | _lib.LINR_PAD_ROW, _stream()),
                               'linr_spconv_cmap')
                _twice(cmap, [out], ins, what)
                _untouched(out, n, cin, what)
                e, a = cr.bwd_ref(t['g'], tab, t['W'], old=old, act=act)
                _note('spconv_cmap backward', cr._within_rounding(_own(out, n, cin), e, a, what))
                for pad in (_lib.LINR_PAD_ROW, 0):
                    out2 = _out(n, cin, cin, old=old)

                    def gather():
                        _lib.check(L.linr_spconv_bwd_data(gp, cout, m['nbr'].data_ptr(), m['ld'], n, t['W'].data_ptr(), cin, cout, aargs[0],
                                                          aargs[1], out2[1:].data_ptr(), cin, flags | pad, _stream()), 'linr_spconv_bwd_data')
                    _twice(gather, [out2], ins, what + ' (linr_spconv_bwd_data)')
                    assert _bits_equal(out, out2), what + ': linr_spconv_bwd_data (pad_row %d) and linr_spconv_cmap differ' % pad
                    COUNT['cases'] += 1


# ---- weight gradients ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', cr.ALL_CLOUDS)
def test_weight_gradient_entries(pkg, key):
    """linr_spconv_bwd_weight and linr_spconv_wgrad_cmap for (8,8), (8,4), (3,8): indices from nbr, from nbr with the padded ld and from
    tile8t - the three slabs equal bit for bit, their float64 sum within the bound, linr_slab_reduce of them within its own."""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    nb = int(L.linr_spconv_wgrad_cmap_blocks())
    assert nb == 512
    for cin, cout in cr.WGRAD_SHAPES:
        t = _case(cr.wgrad_case, key, cin, cout)
        n = t['x'].shape[0]
        xbuf, xp = _in(t['x'], 8)
        elems, split = (27 * cin + 1) * cout, 27 * cin * cout
        slabs = []
        for padded, tiled in ((False, False), (True, False), (True, True)):
            m = _maps(key, padded)
            what = 'weight gradient %d -> %d on %s, ld %d%s' % (cin, cout, key, m['ld'], ', tile8t' if tiled else '')
            exact, absum = cr.wgrad_ref(t['x'], t['g'], m['tab'])
            slab = torch.full((nb + 1, elems), NAN, device='cuda')

            def cmap():
                _lib.check(L.linr_spconv_wgrad_cmap(xp, 8, t['g'].data_ptr(), cout, m['nbr'].data_ptr(), m['t8'].data_ptr() if tiled else None,
                                                    m['ld'], n, cin, cout, slab.data_ptr(), _stream()), 'linr_spconv_wgrad_cmap')
            _twice(cmap, [slab], [xbuf, t['g'], m['nbr']], what)
            _slab_sum_ok(slab, nb, exact, absum, 'spconv_wgrad_cmap', what)
            slabs.append(slab)
            if tiled:
                continue
            for pad in (_lib.LINR_PAD_ROW, 0):          # the two-pass gather entry, dense results
                gw = torch.full((split + 1,), NAN, device='cuda')
                gb = torch.full((cout + 1,), NAN, device='cuda')
                ws = torch.full((max(int(L.linr_spconv_bwd_weight_workspace_bytes(n, cin, cout)), 4) // 4 + 1,), NAN, device='cuda')

                def dense():
                    _lib.check(L.linr_spconv_bwd_weight(xp, 8, t['g'].data_ptr(), cout, m['nbr'].data_ptr(), m['ld'], n, cin, cout, gw.data_ptr(),
                                                        gb.data_ptr(), pad, ws.data_ptr(), ws.numel() * 4, _stream()), 'linr_spconv_bwd_weight')
                _twice(dense, [gw, gb], [xbuf, t['g']], what + ' (linr_spconv_bwd_weight)')
                assert bool(torch.isnan(gw[split:]).all()) and bool(torch.isnan(gb[cout:]).all())
                _note('spconv_bwd_weight', cr._within_rounding(torch.cat([gw[:split], gb[:cout]]), exact, absum, what + ' (linr_spconv_bwd_weight)'))
        assert _bits_equal(slabs[0], slabs[1]) and _bits_equal(slabs[0], slabs[2]), \
            'weight gradient %d -> %d on %s: the index sources give different partials' % (cin, cout, key)
        _check_reduce(slabs[0], nb, split, 'weight gradient %d -> %d on %s' % (cin, cout, key), full=(cin, cout) == (8, 4))
        _check_reduce(slabs[0], nb - 1, split, 'weight gradient %d -> %d on %s' % (cin, cout, key), full=False)


# ---- fused backward of a convolution 8 -> 8 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', cr.ALL_CLOUDS)
def test_fused_backward_8_to_8(pkg, key):
    """linr_spconv_bwd_fused with nblocks 1, 2, 5, 256 (257 rows at nblocks 1: 5 tiles at 2 per wave, a wave carries a tile's last chunk
    into its next tile; 1025: 17 tiles at 5 per wave; 1025 at nblocks 2: waves without a tile): the wave-specialised and the single-stream
    kernel bit for bit, gin bit for bit linr_spconv_cmap's backward, every slab row finite, the slab's float64 sum within the bound."""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    t = _case(cr.fused_case, key)
    n = t['g'].shape[0]
    gbuf, gp = _in(t['g'])
    for padded in (False, True):
        m = _maps(key, padded)
        gin_ref = _out(n, 8, 8)
        _lib.check(L.linr_spconv_cmap(1, gp, 8, m['lo'].data_ptr(), m['mask'].data_ptr(), m['ld'], n, t['W'].data_ptr(), None, 8, 8, None, 0, None,
                                      0, gin_ref[1:].data_ptr(), 8, _lib.LINR_PAD_ROW, _stream()), 'linr_spconv_cmap')
        ge, ga = cr.bwd_ref(t['g'], m['tab'], t['W'])
        se, sa = cr.wgrad_ref(t['x'], t['g'], m['tab'])
        for nblocks in cr.FUSED_NBLOCKS:
            what = 'fused backward on %s, ld %d, nblocks %d' % (key, m['ld'], nblocks)
            res = []
            for single in (False, True):
                gin = _out(n, 8, 8)
                slab = torch.full((nblocks + 1, 1736), NAN, device='cuda')

                def call():
                    _lib.check(L.linr_spconv_bwd_fused(gp, t['x'].data_ptr(), m['lo'].data_ptr(), m['mask'].data_ptr(), m['ld'], n,
                                                       t['W'].data_ptr(), gin[1:].data_ptr(), slab.data_ptr(), nblocks, _stream()),
                               'linr_spconv_bwd_fused')
                if single:
                    with _single_stream():
                        _twice(call, [gin, slab], [gbuf, t['x'], t['W']], what + ' (LINR_FUSED_SPLIT=0)')
                else:
                    _twice(call, [gin, slab], [gbuf, t['x'], t['W']], what)
                res.append((gin, slab))
            (gin, slab), (gin1, slab1) = res
            assert _bits_equal(gin, gin1) and _bits_equal(slab, slab1), what + ': LINR_FUSED_SPLIT=0 gives other bits'
            assert _bits_equal(gin, gin_ref), what + ': gin differs from linr_spconv_cmap\'s backward'
            _note('spconv_bwd_fused gin', cr._within_rounding(_own(gin, n, 8), ge, ga, what + ', gin'))
            _slab_sum_ok(slab, nblocks, se, sa, 'spconv_bwd_fused slab', what + ', slab')
            if nblocks % 2:
                _check_reduce(slab, nblocks, 1728, what, full=nblocks == 5)


# ---- Inception layer ------------------------------------------------------------------------------------------------------------------------------------
def _inc_struct(w):
    from linr_pcgc_amd import _lib
    return _lib.LinrInceptionParams(**{k: v.data_ptr() for k, v in w.items()})


@pytest.mark.parametrize('key', cr.ENTRY_CLOUDS)
def test_inception_forward(pkg, key):
    """linr_inception_fwd: H from x, M from the device's H, I from the device's H and M."""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    t = _case(cr.inception_case, key)
    n, w = t['x'].shape[0], t['w']
    q = _inc_struct(w)
    xbuf, xp = _in(t['x'])
    for padded in (False, True):
        m = _maps(key, padded)
        what = 'linr_inception_fwd on %s, ld %d' % (key, m['ld'])
        H, M, I = _out(n, 8, 8, pad_zero=True), _out(n, 4, 4), _out(n, 8, 8)

        def call():
            _lib.check(L.linr_inception_fwd(xp, m['lo'].data_ptr(), m['mask'].data_ptr(), m['ld'], n, ctypes.byref(q), H[1:].data_ptr(),
                                            M[1:].data_ptr(), I[1:].data_ptr(), _stream()), 'linr_inception_fwd')
        _twice(call, [H, M, I], [xbuf] + list(w.values()), what)
        _untouched(H, n, 8, what + ', H', pad_zero=True)
        _untouched(M, n, 4, what + ', M')
        _untouched(I, n, 8, what + ', I')
        Hd, Md = _own(H, n, 8), _own(M, n, 4)
        _note('inception_fwd', cr._within_rounding(Hd, *cr.inception_H_ref(t['x'], m['tab'], w)[:2], what + ', H'))
        _note('inception_fwd', cr._within_rounding(Md, *cr.inception_M_ref(Hd, m['tab'], w)[:2], what + ', M'))
        _note('inception_fwd', cr._within_rounding(_own(I, n, 8), *cr.inception_I_ref(t['x'], Hd, Md, m['tab'], w), what + ', I'))


@pytest.mark.parametrize('key', cr.ENTRY_CLOUDS)
def test_inception_backward(pkg, key):
    """linr_inception_bwd_data with flags 0 and LINR_RELU_MASK | LINR_ACCUM: gM from gI, gH from the device's gM, gX from the device's gH.
    linr_inception_bwd_fused with the same flags and nblocks 1, 3, 256: gH, gX bit for bit, every slab row finite, the slab's sum within the
    bound.  linr_spconv_wgrad_dual44 with and without tile8t: the same partials, their sum within the bound."""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    t = _case(cr.inception_case, key)
    n, w = t['x'].shape[0], t['w']
    q = _inc_struct(w)
    (xbuf, xp), (Hbuf, Hp), (Mbuf, Mp), (gIbuf, gIp) = _in(t['x']), _in(t['Hb']), _in(t['Mb']), _in(t['gI'])
    ins = [xbuf, Hbuf, Mbuf, gIbuf] + list(w.values())
    d44 = []
    for padded in (False, True):
        m = _maps(key, padded)
        tab = m['tab']
        for flags in (0, _lib.LINR_RELU_MASK | _lib.LINR_ACCUM):
            what = 'linr_inception_bwd_data on %s, ld %d, flags %d' % (key, m['ld'], flags)
            old = t['old'] if flags else None
            gM, gH, gX = _out(n, 4, 4, pad_zero=True), _out(n, 8, 8, pad_zero=True), _out(n, 8, 8, old=old)

            def data():
                _lib.check(L.linr_inception_bwd_data(gIp, xp, Hp, Mp, m['lo'].data_ptr(), m['mask'].data_ptr(), m['ld'], n, ctypes.byref(q),
                                                     gM[1:].data_ptr(), gH[1:].data_ptr(), gX[1:].data_ptr(), flags, _stream()),
                           'linr_inception_bwd_data')
            _twice(data, [gM, gH, gX], ins, what)
            _untouched(gM, n, 4, what + ', gM', pad_zero=True)
            _untouched(gH, n, 8, what + ', gH', pad_zero=True)
            _untouched(gX, n, 8, what + ', gX')
            gMd, gHd = _own(gM, n, 4), _own(gH, n, 8)
            _note('inception_bwd_data', cr._within_rounding(gMd, *cr.inception_gM_ref(t['gI'], t['Mb'], w), what + ', gM'))
            _note('inception_bwd_data', cr._within_rounding(gHd, *cr.inception_gH_ref(t['gI'], gMd, t['Hb'], tab, w), what + ', gH'))
            _note('inception_bwd_data', cr._within_rounding(_own(gX, n, 8), *cr.inception_gX_ref(t['gI'], gHd, t['x'], tab, w, old=old,
                                                                                                 mask=bool(flags)), what + ', gX'))
            se, sa = cr.inception_slab_ref(t['gI'], gMd, gHd, t['x'], t['Hb'], tab)
            for nblocks in cr.INC_NBLOCKS:
                whatf = 'linr_inception_bwd_fused on %s, ld %d, flags %d, nblocks %d' % (key, m['ld'], flags, nblocks)
                gH2, gX2 = _out(n, 8, 8, pad_zero=True), _out(n, 8, 8, old=old)
                slab = torch.full((nblocks + 1, 1776), NAN, device='cuda')

                def fused():
                    _lib.check(L.linr_inception_bwd_fused(gIp, gM[1:].data_ptr(), xp, Hp, m['lo'].data_ptr(), m['mask'].data_ptr(), m['ld'], n,
                                                          ctypes.byref(q), gH2[1:].data_ptr(), gX2[1:].data_ptr(), flags, slab.data_ptr(), nblocks,
                                                          _stream()), 'linr_inception_bwd_fused')
                _twice(fused, [gH2, gX2, slab], ins + [gM], whatf)
                assert _bits_equal(gH, gH2) and _bits_equal(gX, gX2), whatf + ': gH / gX differ from linr_inception_bwd_data\'s'
                _slab_sum_ok(slab, nblocks, se, sa, 'inception_bwd_fused slab', whatf)
                if nblocks == 3 and flags:
                    _check_reduce(slab, nblocks, 864, whatf, full=False)
            if flags:
                continue
            de, da = cr.dual44_ref(t['Hb'], t['gI'][:, 0:4], gMd, tab)
            for tiled in ((False, True) if padded else (False,)):
                whatd = 'linr_spconv_wgrad_dual44 on %s, ld %d%s' % (key, m['ld'], ', tile8t' if tiled else '')
                slab = torch.full((513, 872), NAN, device='cuda')

                def dual():
                    _lib.check(L.linr_spconv_wgrad_dual44(Hp, gIp, 8, gM[1:].data_ptr(), 4, m['nbr'].data_ptr(), m['t8'].data_ptr() if tiled else None,
                                                          m['ld'], n, slab.data_ptr(), _stream()), 'linr_spconv_wgrad_dual44')
                _twice(dual, [slab], [Hbuf, gIbuf, gM], whatd)
                _slab_sum_ok(slab, 512, de, da, 'spconv_wgrad_dual44', whatd)
                d44.append(slab)
    assert all(_bits_equal(d44[0], s) for s in d44[1:]), 'linr_spconv_wgrad_dual44 on %s: the index sources give different partials' % key
    _check_reduce(d44[0], 512, 436, 'linr_spconv_wgrad_dual44 on %s' % key, full=False)


# ---- first convolutions of the outter blocks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', cr.ENTRY_CLOUDS)
def test_occupancy_convolutions(pkg, key):
    """linr_occ_conv7 (all seven blocks, `params` at a non-zero base offset) and linr_occ_wgrad7 with nblocks 1, 3, 256: only the
    *rows_written_h first slab rows are written, their float64 sum within the bound."""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    t = _case(cr.occ_case, key)
    n = t['occ'].shape[0]
    params_h, w_off, b_off = cr.occ_params(cr.occ_case(key))
    params = params_h.cuda()
    obuf, op = _in(t['occ'])
    arr = lambda v: (ctypes.c_int64 * 7)(*v)
    gptrs = (ctypes.c_void_p * 7)(*[g.data_ptr() for g in t['gouts']])
    for padded in (False, True):
        m = _maps(key, padded)
        what = 'linr_occ_conv7 on %s, ld %d' % (key, m['ld'])
        rows = n + 1 + TAIL
        out = torch.full((7 * rows, 8), NAN, device='cuda')

        def conv7():
            _lib.check(L.linr_occ_conv7(op, m['lo'].data_ptr(), m['mask'].data_ptr(), m['ld'], n, params.data_ptr(), arr(w_off), arr(b_off),
                                        out[1:].data_ptr(), arr([g * rows * 8 for g in range(7)]), _stream()), 'linr_occ_conv7')
        _twice(conv7, [out], [obuf, params], what)
        for g in range(7):
            blk = out[g * rows:(g + 1) * rows]
            _untouched(blk, n, 8, '%s, block %d' % (what, g + 1))
            e, a, _ = cr.fwd_ref(t['occ'][:, :g + 1], m['tab'], t['ws'][g], t['bs'][g], relu=True)
            _note('occ_conv7', cr._within_rounding(_own(blk, n, 8), e, a, '%s, block %d' % (what, g + 1)))
        se, sa = cr.occ_wgrad7_ref(t['occ'], t['gouts'], m['tab'])
        for nblocks in cr.OCC_NBLOCKS:
            whatw = 'linr_occ_wgrad7 on %s, ld %d, nblocks %d' % (key, m['ld'], nblocks)
            slab = torch.full((nblocks + 1, 6104), NAN, device='cuda')
            written = ctypes.c_int32(-1)

            def wgrad7():
                _lib.check(L.linr_occ_wgrad7(op, gptrs, m['lo'].data_ptr(), m['mask'].data_ptr(), m['ld'], n, slab.data_ptr(), nblocks,
                                             ctypes.byref(written), _stream()), 'linr_occ_wgrad7')
            _twice(wgrad7, [slab], [obuf] + t['gouts'], whatw)
            assert 1 <= written.value <= nblocks, (whatw, written.value)
            _slab_sum_ok(slab, written.value, se, sa, 'occ_wgrad7', whatw)
            if nblocks == 3:
                _check_reduce(slab, written.value, 6104 - 8, whatw, full=False)


def test_zz_figures_of_this_run(pkg):
    """Prints what the module docstring reports: the checks made, the worst entry per entry kind as a fraction of its bound, the time."""
    torch.cuda.synchronize()
    print('conv8 ops: %d checks in %.1f s' % (COUNT['cases'], time.time() - T0))
    for kind in sorted(WORST):
        print('conv8 ops: worst entry of %-26s at %.3g of its bound' % (kind, WORST[kind]))
