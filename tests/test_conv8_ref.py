"""tests/conv8_ref.py on the CPU, no kernel: the clouds are what they are chosen for, the float64 references agree with oracle.network and
with float64 autograd, every committed forward case has a tie-free draw, a plain fp32 emulation of every op (taps ascending and in the
kernels' LINR_TAP order) passes the criterion on every cloud, and each of eight wrong emulations fails it on a committed case that the
test names - so the GPU test (tests/test_gpu_conv8_ops.py) can tell right from wrong before any GPU sees it."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import conv8_ref as cr                      # noqa: E402
from oracle import network as onet          # noqa: E402

ORDERS = {'ascending': cr.TAPS_ASC, 'LINR_TAP': cr.TAPS_LINR}


# ---- clouds and maps ----------------------------------------------------------------------------------------------------------------------------
def test_clouds_are_what_they_are_chosen_for():
    assert sorted(cr.TAPS_LINR) == list(range(27)) and cr.TAPS_LINR[:4] == (0, 9, 18, 3)
    for key in cr.PAIR_CLOUDS:
        k, c = int(key[5:]), cr.cloud(key)
        present = c['nbr'] >= 0
        assert c['n'] == 2 and bool(present[:, 13].all()) and present.sum(1).tolist() == [2, 2]
        others = sorted(int(torch.nonzero(present[r] & (torch.arange(27) != 13))[0]) for r in range(2))
        assert others == sorted((k, 26 - k)), key
    for key, side in (('cube3', 3), ('cube5', 5)):
        c = cr.cloud(key)
        assert c['n'] == side ** 3 and int(((c['nbr'] >= 0).sum(1) == 27).sum()) == (side - 2) ** 3
    for key in ('single', 'isolated257'):
        c = cr.cloud(key)
        assert c['n'] == (1 if key == 'single' else 257)
        assert bool(((c['nbr'] >= 0).sum(1) == 1).all()) and torch.equal(c['nbr'][:, 13], torch.arange(c['n']))
    for n in cr.BOX_NS:
        c = cr.cloud('box_%d' % n)
        assert c['n'] == n
        if n >= 255:          # about one third occupancy: every tap occurs, rows with few and with many neighbours
            cnt = (c['nbr'] >= 0).sum(1)
            assert bool((c['nbr'] >= 0).any(0).all()) and int(cnt.min()) <= 4 and int(cnt.max()) >= 12
    for key in cr.ALL_CLOUDS:
        co = cr.cloud(key)['coord'].astype(np.int64)
        ravel = (co[:, 0] << 42) + (co[:, 1] << 21) + co[:, 2]
        assert bool((np.diff(ravel) > 0).all()), key + ': not sorted x-major and unique'
    assert cr.fb_grid(257, 1) == (2, 1) and cr.fb_grid(1025, 1) == (5, 1) and cr.fb_grid(1025, 2) == (3, 2)


@pytest.mark.parametrize('key', cr.ALL_CLOUDS)
def test_compressed_and_tiled_forms_stand_for_the_table(key):
    c = cr.cloud(key)
    n, nbr = c['n'], c['nbr']
    lo, mask = cr.compress(nbr)
    assert torch.equal(cr.decode_cmap(lo, mask).t(), nbr)
    assert torch.equal(((mask.view(-1, 1) >> (3 * (torch.arange(27) % 9) + torch.arange(27) // 9)) & 1) == 1, nbr >= 0)
    t8 = cr.tile8t_ref(nbr.t().numpy(), n).reshape(-1, 4, 8, 8)
    assert t8.shape[0] == (n + 7) // 8 + cr.TILE8T_SPARE
    assert (t8[:, :, :, 7] == -1).all() and (t8[:, 3, :, 6] == -1).all() and (t8[(n + 7) // 8:] == -1).all()
    back = np.full((n, 27), -2, dtype=np.int64)
    for p in range(27):
        back[:, cr.TAPS_LINR[p]] = t8[:, p % 4, :, p // 4].reshape(-1)[:n]
        assert (t8[:, p % 4, :, p // 4].reshape(-1)[n:] == -1).all()
    assert (back == nbr.numpy()).all()


# ---- the references against oracle.network and float64 autograd ----------------------------------------------------------------------------------
def _sd(w):
    return {'p.conv%s.%s' % (k[1] + '_' + k[2], 'kernel' if k[0] == 'w' else 'bias'): (v if k[0] == 'w' else v.view(1, -1)) for k, v in w.items()}


@pytest.mark.parametrize('key', ['pair_5', 'cube3', 'box_65', 'isolated257'])
def test_references_agree_with_the_oracle_and_autograd(key):
    nbr, n = cr.cloud(key)['nbr'], cr.cloud(key)['n']
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-13)
    # forward / backward-data / weight gradient of one convolution
    t, tb = cr.fwd_case(key, 8, 4), cr.bwd_case(key, 8, 4)
    x, W, b = t['x'].double().requires_grad_(), t['W'].double().requires_grad_(), t['b'].double().requires_grad_()
    y = onet.conv3(x, nbr, W, b.view(1, -1))
    assert close(cr.fwd_ref(t['x'], nbr, t['W'], t['b'])[0], y.detach())
    assert close(cr.fwd_ref(t['x'], nbr, t['W'], t['b'], res=t['res'], relu=True)[0], F.relu(y.detach() + t['res'].double()))
    g = tb['g'].double()
    y.backward(g)
    assert close(cr.bwd_ref(tb['g'], nbr, t['W'])[0], x.grad)
    e, a = cr.wgrad_ref(t['x'], tb['g'], nbr)
    assert close(e, torch.cat([W.grad.reshape(-1), b.grad])) and bool((a >= e.abs() - 1e-12).all())
    e, _ = cr.bwd_ref(tb['g'], nbr, t['W'], old=tb['old'], act=tb['act'])
    assert close(e, (x.grad + tb['old'].double()) * (tb['act'] > 0).double())
    # the Inception layer: forward chain, then each backward output from its own inputs, against autograd through oracle.network.inception
    ti = cr.inception_case(key)
    x0 = torch.randn(n, 8, generator=torch.Generator().manual_seed(1), dtype=torch.float64).requires_grad_()
    xr = F.relu(x0)
    w = {k: v.double().requires_grad_() for k, v in ti['w'].items()}
    out = onet.inception(xr, nbr, _sd(w), 'p')
    xd, wd = xr.detach(), {k: v.detach() for k, v in w.items()}
    H, _, _ = cr.inception_H_ref(xd, nbr, wd)
    M, _, _ = cr.inception_M_ref(H, nbr, wd)
    assert close(cr.inception_I_ref(xd, H, M, nbr, wd)[0], out.detach())
    gI = ti['gI'].double()
    out.backward(gI)
    gM, _ = cr.inception_gM_ref(gI, M, wd)
    gH, _ = cr.inception_gH_ref(gI, gM, H, nbr, wd)
    assert close(cr.inception_gX_ref(gI, gH, xd, nbr, wd, mask=True)[0], x0.grad)
    old = ti['old'].double()
    assert close(cr.inception_gX_ref(gI, gH, xd, nbr, wd, old=old, mask=True)[0], (x0.grad + old * (xd > 0)))
    slab, sa = cr.inception_slab_ref(gI, gM, gH, xd, H, nbr)
    want = torch.cat([w[k].grad.reshape(-1) for k in ('w00', 'b00', 'w01', 'b01', 'w11', 'b11', 'w10', 'b10')])
    assert slab.numel() == 1776 and close(slab, want) and bool((sa >= slab.abs() - 1e-12).all())
    d44, _ = cr.dual44_ref(H, gI[:, 0:4], gM, nbr)
    assert d44.numel() == 872 and close(d44, torch.cat([w[k].grad.reshape(-1) for k in ('w01', 'b01', 'w11', 'b11')]))
    # first convolutions of the outter blocks
    to = cr.occ_case(key)
    wants = []
    for bk in range(1, 8):
        Wb, bb = to['ws'][bk - 1].double().requires_grad_(), to['bs'][bk - 1].double().requires_grad_()
        yb = onet.conv3(to['occ'][:, :bk].double(), nbr, Wb, bb.view(1, -1))
        assert close(cr.fwd_ref(to['occ'][:, :bk], nbr, to['ws'][bk - 1], to['bs'][bk - 1], relu=True)[0], F.relu(yb.detach()))
        yb.backward(to['gouts'][bk - 1].double())
        wants += [Wb.grad.reshape(-1), bb.grad]
    e, _ = cr.occ_wgrad7_ref(to['occ'], to['gouts'], nbr)
    assert e.numel() == 6104 and close(e, torch.cat(wants))


# ---- every committed forward case has a tie-free draw -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', cr.ALL_CLOUDS)
def test_every_relu_case_finds_a_tie_free_draw(key):
    """fwd_case / inception_case / occ_case raise when six draws in a row have a float64 pre-activation below TIE."""
    for cin, cout in cr.FWD_SHAPES:
        assert cr.fwd_case(key, cin, cout)['attempt'] < cr.DRAWS
    if key in cr.ENTRY_CLOUDS:
        assert cr.inception_case(key)['attempt'] < cr.DRAWS and cr.occ_case(key)['attempt'] < cr.DRAWS


# ---- a plain fp32 emulation passes --------------------------------------------------------------------------------------------------------------
def _check_fwd(key, cin, cout, form, got):
    t, nbr = cr.fwd_case(key, cin, cout), cr.cloud(key)['nbr']
    e, a, _ = cr.fwd_ref(t['x'], nbr, t['W'], t['b'], res=t['res'] if 'res' in form else None, relu='relu' in form)
    return cr._within_rounding(got, e, a, 'forward %d -> %d %s on %s' % (cin, cout, form, key))


def _check_bwd(key, cin, cout, form, got):
    t, nbr = cr.bwd_case(key, cin, cout), cr.cloud(key)['nbr']
    e, a = cr.bwd_ref(t['g'], nbr, t['W'], old=t['old'] if 'accum' in form else None, act=t['act'] if 'mask' in form else None)
    return cr._within_rounding(got, e, a, 'backward-data %d -> %d %s on %s' % (cin, cout, form, key))


def _check_wgrad(key, cin, cout, got):
    t, nbr = cr.wgrad_case(key, cin, cout), cr.cloud(key)['nbr']
    e, a = cr.wgrad_ref(t['x'], t['g'], nbr)
    return cr._within_rounding(got, e, a, 'weight gradient %d -> %d on %s' % (cin, cout, key))


@pytest.mark.parametrize('order', sorted(ORDERS))
@pytest.mark.parametrize('key', cr.ALL_CLOUDS)
def test_plain_fp32_emulation_passes(key, order):
    o = ORDERS[order]
    for cin, cout in cr.FWD_SHAPES:
        for form in cr.FWD_FORMS:
            _check_fwd(key, cin, cout, form, cr.emu_fwd(key, cin, cout, form, o))
    for cin, cout in cr.BWD_SHAPES:
        for form in cr.BWD_FORMS:
            _check_bwd(key, cin, cout, form, cr.emu_bwd(key, cin, cout, form, o))
    for cin, cout in cr.WGRAD_SHAPES:
        got = cr.emu_wgrad(key, cin, cout)
        _check_wgrad(key, cin, cout, got)
        e, a = cr.slab_ref(got.view(1, -1).repeat(5, 1))          # linr_slab_reduce: an fp32 sum of five rows
        cr._within_rounding(((((got + got) + got) + got) + got), e, a, 'slab sum')
    if key not in cr.ENTRY_CLOUDS:
        return
    nbr = cr.cloud(key)['nbr']
    t = cr.inception_case(key)
    H, M, I = cr.emu_inception_fwd(key, o)
    cr._within_rounding(H, *cr.inception_H_ref(t['x'], nbr, t['w'])[:2], 'H on ' + key)
    cr._within_rounding(M, *cr.inception_M_ref(H, nbr, t['w'])[:2], 'M on ' + key)
    cr._within_rounding(I, *cr.inception_I_ref(t['x'], H, M, nbr, t['w']), 'I on ' + key)
    for flags in (0, 6):
        gM, gH, gX = cr.emu_inception_bwd(key, o, flags)
        cr._within_rounding(gM, *cr.inception_gM_ref(t['gI'], t['Mb'], t['w']), 'gM on ' + key)
        cr._within_rounding(gH, *cr.inception_gH_ref(t['gI'], gM, t['Hb'], nbr, t['w']), 'gH on ' + key)
        cr._within_rounding(gX, *cr.inception_gX_ref(t['gI'], gH, t['x'], nbr, t['w'], old=t['old'] if flags else None, mask=bool(flags)),
                            'gX on ' + key)
    to = cr.occ_case(key)
    for g, got in enumerate(cr.emu_occ_conv7(key, o)):
        cr._within_rounding(got, *cr.fwd_ref(to['occ'][:, :g + 1], nbr, to['ws'][g], to['bs'][g], relu=True)[:2], 'occ_conv7 block %d' % (g + 1))


# ---- every mutant is caught -----------------------------------------------------------------------------------------------------------------------
# mutant -> (the committed cases it must fail on, a function that checks the emulation with this mutant on such a case)
CAUGHT = {
    'taps_swapped': (['pair_3', 'pair_17', 'cube3', 'box_257'], lambda key, m: _check_fwd(key, 8, 8, 'none', cr.emu_fwd(key, 8, 8, 'none', cr.TAPS_LINR, m))),
    'bwd_not_mirrored': (['pair_0', 'pair_22', 'box_9'], lambda key, m: _check_bwd(key, 8, 4, 'none', cr.emu_bwd(key, 8, 4, 'none', cr.TAPS_LINR, m))),
    'third_tap_ignores_b1': (['cube3', 'cube5', 'box_65'], lambda key, m: _check_fwd(key, 4, 4, 'res', cr.emu_fwd(key, 4, 4, 'res', cr.TAPS_LINR, m))),
    'wgrad_last_group_dropped': (['box_1', 'box_9', 'box_17', 'box_257', 'box_1025'], lambda key, m: _check_wgrad(key, 8, 8, cr.emu_wgrad(key, 8, 8, m))),
    'wgrad_wave_tile_dropped': (['box_257', 'box_1025'], lambda key, m: _check_wgrad(key, 8, 8, cr.emu_wgrad(key, 8, 8, m, nblocks=1))),
    'bias_grad_short': (['single', 'box_2', 'box_1025'], lambda key, m: _check_wgrad(key, 3, 8, cr.emu_wgrad(key, 3, 8, m))),
    'accum_ignored': (['pair_4', 'box_7'], lambda key, m: _check_bwd(key, 4, 4, 'accum', cr.emu_bwd(key, 4, 4, 'accum', cr.TAPS_LINR, m))),
    'mask_on_wrong_matrix': (['box_7', 'box_64'], lambda key, m: _check_bwd(key, 8, 8, 'accum_mask', cr.emu_bwd(key, 8, 8, 'accum_mask', cr.TAPS_LINR, m))),
}


@pytest.mark.parametrize('mut', cr.MUTANTS)
def test_every_mutant_fails_on_a_named_case(mut):
    cases, check = CAUGHT[mut]
    for key in cases:
        assert key in cr.ALL_CLOUDS
        ratio = check(key, None)                                  # the unbroken emulation passes the same case ...
        with pytest.raises(AssertionError, match='x its bound'):          # ... and the mutant does not
            check(key, mut)
        print('%s on %s: the unbroken emulation at %.3g of the bound' % (mut, key, ratio))
