"""Every entry of the wide bf16 / uint8-weight inference executor (csrc/wide_bf16.hip) at op level against float64: the prologue
linr_wide_bf16_prep, all 14 instantiations of wdispatch through linr_spconv_wide_bf16 and linr_head_wide_bf16_fwd (the three WE_PLAIN
ones no network schedule launches included), linr_sce_fwd_bf16 and linr_occ_to_bf16.

The criterion, the inputs and their reasons are in tests/wide_bf16_ops_ref.py (checked without a GPU by tests/test_wide_bf16_ops_ref.py):
every stored bf16 value must lie in the interval the float64 sum and its rounding bound (gpu_common.C_ROUND 2^-24 sum |terms|) leave it,
which determines the stored bits of at least 90 % of the entries of every case; the head's fp32 probabilities within the fp32 logit
tolerance of tests/gpu_common.py, its block partials within 1e-5 relative.  Every output buffer starts as NaN bit patterns (0xFFFF) and
everything outside an entry's own rows and blocks must still hold them afterwards: the pad row, neighbouring blocks (the other half of H
or I), rows past n.  Every entry runs in two layouts that must give the same bits: tight (block stride 8 (n + 1), map ld = n) and as
WideNet._block_bf16 addresses sub-blocks (`_sub` of a wider matrix, block stride 8 (n + 4), map ld = the next multiple of 64).

Measured on the MI355X, all 145 cases pass (1.8 s): no bug found.  Ambiguous entries, worst case per kind (a property of the reference,
the same on the CPU): WE_PLAIN 9.27 % (32 -> 32, bare, 216-row cube), with res + ReLU and / or res2 at most 5.5 %; WE_PW1 3.31 %; WE_PW2
7.32 % (8.94 % at 63 rows); scale context 7.14 %.  Stored values that are not the rounding of the exact sum itself (all of them
ambiguous entries): at most 0.192 % of a case for WE_PLAIN (one entry of 520), 0.006 % for WE_PW1, none for WE_PW2 on the rows whose M is
determined, none for the scale context.  Where a stored value moved, the error of the fp32 value that this proves is at most 0.0081 of
its bound eps for WE_PLAIN and 0.00016 for WE_PW1 (wide_bf16_ops_ref.check_interval; |got - y| / eps itself is 200 ... 2.6e5 on every
case because it holds the store's own rounding, so it is not the figure printed).  Head: worst logit at 0.0054 (C = 16) / 0.087 (C = 32)
of 1e-4 + 1e-4 |z|, every |z64| below 6.3 (no row takes the saturated branch here: tests/test_gpu_heads_saturated.py has those); block
partials within 1.4e-7 relative.  The two layouts gave the same bits everywhere."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wide_bf16_ops_ref as wr               # noqa: E402

pytestmark = pytest.mark.gpu

CONV_LAYERS = [l for l in wr.LAYERS if l[0] != wr.WE_HEAD]
HEAD_LAYERS = [l for l in wr.LAYERS if l[0] == wr.WE_HEAD]
NAN16 = -1          # int16 0xFFFF: a bf16 NaN


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope='module')
def prepped(pkg):
    """The bank on the device after ONE linr_wide_bf16_prep: fp32 parameters (NaN before) and the images (0xFF bytes before, 16 guard
    bytes behind them)."""
    from linr_pcgc_amd import _lib, ops
    L = _lib.lib()
    b = wr.bank()
    for _, cin, co, _ in b['convs']:
        assert int(L.linr_wide_bf16_image_elems(cin, co)) == wr.image_elems(cin, co)
    codes = b['codes'].cuda()
    tab = torch.tensor([list(c) for c in b['convs']], dtype=torch.int64).cuda()
    pf = torch.full((codes.numel(),), float('nan'), device='cuda')
    img = torch.full((8 * b['n_img'] + 16,), 0xFF, dtype=torch.uint8, device='cuda')
    ops.wide_bf16_prep(codes, wr.QRANGE, tab, len(b['convs']), b['n_img'], pf, img)
    torch.cuda.synchronize()
    return {'pf': pf, 'img': img, 'img_ptr': {layer: img.data_ptr() + 8 * c[3] for layer, c in zip(wr.LAYERS, b['convs'])}}


def _p(prepped, layer, name):
    return wr.param(layer, name, pf=prepped['pf'])


_MAPS = {}


def _maps(key, padded):
    """The library's compressed map of a cloud, ld = n or the next multiple of 64 (made once)."""
    if (key, padded) not in _MAPS:
        from linr_pcgc_amd import ops
        c = wr.cloud(key)
        n = c['n']
        ld = (n + 63) // 64 * 64 if padded else n
        nbr = torch.full((27, ld), -1, dtype=torch.int32, device='cuda')
        nbr[:, :n] = ops.kmap_build(torch.from_numpy(c['coord']).cuda().contiguous())
        assert torch.equal(nbr[:, :n].t().long().cpu(), c['nbr']), 'kernel map and oracle table differ'
        lo, mask = ops.kmap_compress(nbr, n)
        assert lo.stride(0) == ld
        _MAPS[(key, padded)] = {'n': n, 'lo': lo, 'mask': mask}
    return _MAPS[(key, padded)]


def _layout(nb, loose):
    """(blocks in front, rows behind row n): the loose layout is _sub(matrix, nb) of a matrix of 2 nb + 1 blocks."""
    return (nb, 3) if loose else (0, 0)


def _in_blocks(t, loose):
    """bf16-valued fp32 [n, c] (host) -> blocked bf16 on the device: zero row in front, channels past c hold 7.0, everything else - blocks
    in front and behind, rows past n - NaN.  Returns (buffer, (pointer of the first block's first row, block stride))."""
    from linr_pcgc_amd.wide_net import _sub
    n, c = t.shape
    nb = (c + 7) // 8
    lead, extra = _layout(nb, loose)
    own = torch.full((nb, n, 8), 7.0)
    for i in range(nb):
        w = min(8, c - 8 * i)
        own[i, :, :w] = t[:, 8 * i:8 * i + w]
    buf = torch.full((lead + nb + 1, n + 1 + extra, 8), NAN16, dtype=torch.int16)
    buf[lead:lead + nb, 1:n + 1] = own.to(torch.bfloat16).view(torch.int16)
    buf[lead:lead + nb, 0] = 0
    buf = buf.cuda()
    return buf, _sub((buf[0, 1].data_ptr(), buf.stride(0)), lead)


def _out_blocks(n, nb, loose):
    from linr_pcgc_amd.wide_net import _sub
    lead, extra = _layout(nb, loose)
    buf = torch.full((lead + nb + 1, n + 1 + extra, 8), NAN16, dtype=torch.int16, device='cuda')
    return buf, _sub((buf[0, 1].data_ptr(), buf.stride(0)), lead)


def _read_out(buf, n, nb, loose, what):
    """The entry's own rows as fp32 [n, 8 nb]; everything else in the buffer must still be the NaN fill."""
    lead, _ = _layout(nb, loose)
    buf = buf.cpu()
    own = buf[lead:lead + nb, 1:n + 1].clone()
    buf[lead:lead + nb, 1:n + 1] = NAN16
    assert bool((buf == NAN16).all()), '%s: %d elements written outside the entry\'s own rows and blocks' % (what, int((buf != NAN16).sum()))
    return own.view(torch.bfloat16).float().permute(1, 0, 2).reshape(n, 8 * nb)


def _run_conv(prepped, layer, key, form, loose):
    from linr_pcgc_amd import ops
    epi, cin, co = layer
    t, m = wr.inputs(layer, key), _maps(key, loose)
    n = m['n']
    nbo = co // 8 * (2 if epi == wr.WE_PW1 else 1)
    keep = []

    def blocks(v):
        buf, ref = _in_blocks(v, loose)
        keep.append(buf)
        return ref
    x = blocks(t['x'])
    res = blocks(t['res']) if 'res_relu' in form else blocks(t['x_hi']) if epi == wr.WE_PW2 else None
    res2 = blocks(t['res2']) if 'res2' in form else None
    pw = None if epi == wr.WE_PLAIN else (_p(prepped, layer, 'pw_w'), _p(prepped, layer, 'pw_b'))
    obuf, out = _out_blocks(n, nbo, loose)
    ops.spconv_wide_bf16(epi, x, cin, m['lo'], m['mask'], n, prepped['img_ptr'][layer], _p(prepped, layer, 'bias'), co, out, res=res,
                         res2=res2, pw=pw, relu='res_relu' in form)
    torch.cuda.synchronize()
    return _read_out(obuf, n, nbo, loose, '%s %s %s' % (wr.layer_id(layer), key, form))


# ---- prologue -------------------------------------------------------------------------------------------------------------------------------
def test_prologue_dequantises_bit_exactly(prepped):
    """pf == q / 255 * range + min step by step in fp32 (range an fp32 subtraction), every parameter; the 16 bytes behind the images keep
    their fill.  The images are not decoded by their layout formula: a wrong slot fails the convolutions below."""
    assert torch.equal(prepped['pf'].cpu(), wr.bank()['pf'])
    assert bool((prepped['img'][-16:] == 0xFF).all())


# ---- the 12 convolution instantiations ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', wr.CLOUDS, ids=str)
@pytest.mark.parametrize('layer', CONV_LAYERS, ids=wr.layer_id)
def test_convolution_entries_store_the_determined_bits(prepped, layer, key):
    """WE_PLAIN bare / + res + ReLU / + res2 / both, WE_PW1 and WE_PW2 with and without res2, in both layouts."""
    for form in wr.forms_of(layer):
        iv = wr.intervals(layer, key, form)
        what = '%s on cloud %s, %s' % (wr.layer_id(layer), key, form)
        tight = _run_conv(prepped, layer, key, form, False)
        amb, off, ratio = wr.check_interval(tight, iv, what)
        assert amb <= wr.AMBIGUOUS_CAP
        print('%s: %.2f %% ambiguous, %.3f %% not the rounding of the exact sum, worst visible error / eps %.3g' % (what, 100 * amb, 100 * off, ratio))
        loose = _run_conv(prepped, layer, key, form, True)
        wr.check_interval(loose, iv, what + ', sub-blocks')
        assert torch.equal(tight, loose), what + ': the two layouts differ'


# ---- head -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', wr.CLOUDS, ids=str)
@pytest.mark.parametrize('layer', HEAD_LAYERS, ids=wr.layer_id)
def test_head_probabilities_and_block_partials(prepped, layer, key):
    """p against the float64 logits of the unrounded prune convolution; partial[b] against the float64 sum of nats(p_stored, t) over
    block b's live rows for t_col 0, 3, 7 (a dead lane that adds row n - 1 again fails n = 1, 65, 257, whose last block is mostly dead);
    with partial = NULL the same bits in p."""
    from linr_pcgc_amd import ops
    _, _, C = layer
    t = wr.inputs(layer, key)
    target = t['target'].cuda().contiguous()
    hp = [_p(prepped, layer, k) for k in ('bias', 'w1', 'b1', 'w2', 'b2')]
    first = None
    for loose in (False, True):
        m = _maps(key, loose)
        n = m['n']
        nb = (n + 255) // 256
        xbuf, x = _in_blocks(t['x'], loose)
        what = '%s on cloud %s%s' % (wr.layer_id(layer), key, ', sub-blocks' if loose else '')

        def run(t_col, partial):
            p = torch.full((n + 3,), float('nan'), device='cuda')
            ops.head_wide_bf16(x, C, m['lo'], m['mask'], n, prepped['img_ptr'][layer], *hp, target.data_ptr(), t_col, p, partial)
            torch.cuda.synchronize()
            assert bool(torch.isnan(p[n:]).all()), what + ': p written past n'
            return p[:n].cpu()
        p0 = run(0, None)
        worst = wr.check_head_p(p0, layer, key, what)
        first = p0 if first is None else first
        assert torch.equal(p0, first), what + ': the two layouts differ'
        rel = 0.0
        for t_col in (0, 3, 7):
            partial = torch.full((nb + 1,), float('nan'), dtype=torch.float64, device='cuda')
            p = run(t_col, partial)
            assert torch.equal(p, p0), what + ': p depends on partial'
            assert bool(torch.isnan(partial[nb:]).all()), what + ': partial written past the last block'
            rel = max(rel, wr.check_partial(partial[:nb], p, t['target'][:, t_col], '%s, t_col %d' % (what, t_col)))
        print('%s: worst logit at %.3g of 1e-4 + 1e-4 |z|, worst block partial %.3g relative' % (what, worst, rel))


# ---- scale context --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(wr.SCE_CASES))
def test_scale_context_stores_the_determined_bits(pkg, name):
    """linr_sce_fwd_bf16 on a three-scale frame whose middle scale is empty (257 + 0 + 65 rows) and on one row, against
    tests/sce_ref.py's float64 scale context under the interval criterion; the zero row's place and the rows past the frame untouched."""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    k = wr.sce_case(name)
    R = int(k['row_off'][-1])
    off, flat = k['off'].cuda().contiguous(), k['flat'].cuda()
    fr = _lib.LinrFrame(rows=R, n_scales=len(k['sidx']), model_scale_num=k['S'], block_layers=1, flags=0, row_off_h=k['row_off'].ctypes.data,
                        scale_idx_h=k['sidx'].ctypes.data, nbr=0, nbr_ld=R, nbr_lo=0, nbr_mask=0, offset_feat=off.data_ptr(), occ=0, nbr8t=0)
    buf = torch.full((R + 4, 8), NAN16, dtype=torch.int16, device='cuda')
    _lib.check(L.linr_sce_fwd_bf16(flat.data_ptr(), ctypes.byref(fr), buf.data_ptr(), _stream()), 'linr_sce_fwd_bf16')
    torch.cuda.synchronize()
    buf = buf.cpu()
    assert bool((buf[0] == NAN16).all()) and bool((buf[R + 1:] == NAN16).all())
    amb, off_nom, ratio = wr.check_interval(buf[1:R + 1].view(torch.bfloat16).float(), k['iv'], 'scale context ' + name)
    print('scale context %s: %.2f %% ambiguous, %.3f %% not the rounding of the exact sum, worst visible error / eps %.3g'
          % (name, 100 * amb, 100 * off_nom, ratio))


# ---- occupancy ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 257])
def test_occupancy_to_bf16_is_exact(pkg, n):
    """Rows 1 .. n are the bf16 of the 0 / 1 occupancy; the zero row in front is as it was (the entry clears it itself:
    engine.Frame.occ_bf16 hands it an uninitialised buffer, so a row that was not zero cannot be asked to survive); rows past n keep
    their fill."""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    occ = (torch.rand(n, 8, generator=torch.Generator().manual_seed(n)) < 0.5).float()
    buf = torch.full((n + 4, 8), NAN16, dtype=torch.int16, device='cuda')
    buf[0] = 0
    occ_d = occ.cuda().contiguous()
    _lib.check(L.linr_occ_to_bf16(occ_d.data_ptr(), n, buf.data_ptr(), _stream()), 'linr_occ_to_bf16')
    torch.cuda.synchronize()
    buf = buf.cpu()
    assert bool((buf[0] == 0).all()) and bool((buf[n + 1:] == NAN16).all())
    assert torch.equal(buf[1:n + 1], occ.to(torch.bfloat16).view(torch.int16))
