"""tests/wide_bf16_ops_ref.py on the CPU, no kernel involved: rb64 is RNE to bf16; the clouds cover every tap; every case that
tests/test_gpu_wide_bf16_ops.py runs stays under the ambiguity cap; and the interval criterion has teeth - a correct fp32 emulation of
every chain is accepted on every cloud, and each of eight mutants (a rounding in the wrong place, a wrong weight slot, a pad channel that
leaks, a dead lane counted into a block's partial) is rejected at 257 rows."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sce_ref as sr                         # noqa: E402
import wide_bf16_ops_ref as wr               # noqa: E402
from oracle import network as onet           # noqa: E402

CONV_LAYERS = [l for l in wr.LAYERS if l[0] != wr.WE_HEAD]
HEAD_LAYERS = [l for l in wr.LAYERS if l[0] == wr.WE_HEAD]
PAD_LAYERS = [l for l in CONV_LAYERS if l[1] % 8]


# ---- rb64 ---------------------------------------------------------------------------------------------------------------------------------
def test_rb64_is_torchs_bfloat16_cast_on_fp32_values():
    """Random fp32 bit patterns of both signs (subnormals included), every exact tie between two bf16 values of a few exponents, zeros,
    the largest finite values: rb64 of the float64 copy == torch's cast."""
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32)
    ties = np.concatenate([(np.arange(0, 2 ** 16, dtype=np.uint32) << 16) | np.uint32(0x8000)])          # every bf16 pattern + half a step
    near = np.concatenate([ties - 1, ties + 1])
    edge = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00008000, 0x00010000, 0x007FFFFF, 0x00800000, 0x7F7F0000, 0x7F7F7FFF,
                     0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000], dtype=np.uint32)
    x = torch.from_numpy(np.concatenate([bits, ties, near, edge]).view(np.float32).copy())
    x = x[torch.isfinite(x)]
    assert int((x < 0).sum()) > 1000 and int((x.abs() < 2.0 ** -126).sum()) > 100
    want = x.to(torch.bfloat16).to(torch.float64)
    got = wr.rb64(x.double())
    assert torch.equal(got, want)
    assert torch.equal(torch.signbit(got), torch.signbit(want))


def test_rb64_does_not_round_twice():
    """2^-30 above the tie between 1 and 1 + 2^-7: a detour through float32 lands ON the tie and then on 1; rb64 goes up.  And the
    mirror image below the tie above an odd value."""
    up = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30, -(1.0 + 2.0 ** -8 + 2.0 ** -30)], dtype=torch.float64)
    assert wr.rb64(up).tolist() == [1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7)]
    assert up.float().to(torch.bfloat16).double().tolist() == [1.0, -1.0]
    down = torch.tensor([1.0 + 3 * 2.0 ** -8 - 2.0 ** -30], dtype=torch.float64)
    assert wr.rb64(down).tolist() == [1.0 + 2.0 ** -7]
    assert down.float().to(torch.bfloat16).double().tolist() == [1.0 + 2.0 ** -6]


# ---- clouds and bank ------------------------------------------------------------------------------------------------------------------------
def test_clouds_cover_every_tap():
    for key in wr.CLOUDS:
        c = wr.cloud(key)
        assert c['n'] == (216 if key == 'cube6' else key)
        if c['n'] >= 257:
            share = wr.tap_shares(key)
            print('cloud %s: rarest tap in %.1f %% of the rows' % (key, 100 * float(share.min())))
            assert float(share.min()) >= wr.TAP_SHARE, (key, share)
    assert int((wr.cloud('cube6')['nbr'] >= 0).all(dim=1).sum()) == 64


def test_bank_layout():
    b = wr.bank()
    assert len(b['convs']) == 14 and all(c[0] > 0 for c in b['convs'])
    assert len({wr.layer_id(l) for l in wr.LAYERS}) == 14
    assert b['codes'].dtype == torch.uint8 and int(b['codes'].min()) == 0 and int(b['codes'].max()) == 255
    assert float(b['pf'].min()) == pytest.approx(wr.QRANGE[0], abs=1e-7) and float(b['pf'].max()) == pytest.approx(wr.QRANGE[1], abs=1e-6)
    for (_, cin, co, start), nxt in zip(b['convs'], [c[3] for c in b['convs'][1:]] + [b['n_img']]):
        assert nxt - start == wr.image_elems(cin, co)


# ---- the ambiguity cap, for every case of the GPU module ------------------------------------------------------------------------------------
@pytest.mark.parametrize('layer', CONV_LAYERS, ids=wr.layer_id)
def test_ambiguity_cap(layer):
    worst = 0.0
    for key in wr.CLOUDS:
        for form in wr.forms_of(layer):
            iv = wr.intervals(layer, key, form)
            assert bool((iv['lo'] <= iv['hi']).all())
            share = wr.ambiguous_share(iv)
            assert share <= wr.AMBIGUOUS_CAP, (wr.layer_id(layer), key, form, share)
            if wr.cloud(key)['n'] >= 216:
                worst = max(worst, share)
    print('%s: at most %.2f %% of the entries ambiguous (clouds of 216 rows and more)' % (wr.layer_id(layer), 100 * worst))


@pytest.mark.parametrize('name', sorted(wr.SCE_CASES))
def test_ambiguity_cap_scale_context(name):
    k = wr.sce_case(name)
    share = wr.ambiguous_share(k['iv'])
    print('scale context %s: %.2f %% of the entries ambiguous' % (name, 100 * share))
    assert share <= wr.AMBIGUOUS_CAP


# ---- the criterion has teeth ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layer', CONV_LAYERS, ids=wr.layer_id)
def test_correct_emulation_is_accepted(layer):
    for key in wr.CLOUDS:
        for form in wr.forms_of(layer):
            wr.check_interval(wr.emulate(layer, key, form), wr.intervals(layer, key, form), '%s %s %s' % (wr.layer_id(layer), key, form))


@pytest.mark.parametrize('layer', HEAD_LAYERS, ids=wr.layer_id)
def test_correct_head_emulation_is_accepted(layer):
    worst = 0.0
    for key in wr.CLOUDS:
        for t_col in (0, 3, 7):
            p, part = wr.emulate_head(layer, key, t_col)
            worst = max(worst, wr.check_head_p(p, layer, key, '%s %s' % (wr.layer_id(layer), key)))
            wr.check_partial(part, p, wr.inputs(layer, key)['target'][:, t_col], 'partial')
    z = wr.head64(layer, 1025)['z64']
    print('%s: fp32 emulation at %.3g of the logit tolerance; |z64| up to %.2f' % (wr.layer_id(layer), worst, float(z.abs().max())))


def _rejected(fn):
    with pytest.raises(AssertionError):
        fn()


def _conv_mutant_rejected(layer, form, mut, key=257):
    what = '%s %s %s' % (wr.layer_id(layer), form, mut)
    _rejected(lambda: wr.check_interval(wr.emulate(layer, key, form, mut), wr.intervals(layer, key, form), what))


@pytest.mark.parametrize('layer', CONV_LAYERS, ids=wr.layer_id)
def test_mutant_truncation_at_the_store(layer):
    for form in wr.forms_of(layer):
        _conv_mutant_rejected(layer, form, 'truncate_store')


@pytest.mark.parametrize('layer', [l for l in CONV_LAYERS if l[0] == wr.WE_PW2], ids=wr.layer_id)
def test_mutant_m_left_unrounded(layer):
    for form in wr.PW_FORMS:
        _conv_mutant_rejected(layer, form, 'm_unrounded')


@pytest.mark.parametrize('layer', CONV_LAYERS, ids=wr.layer_id)
def test_mutant_res2_added_before_the_rounding(layer):
    for form in wr.forms_of(layer):
        if 'res2' in form:
            _conv_mutant_rejected(layer, form, 'res2_before_rounding')


@pytest.mark.parametrize('mut', ['taps_swapped', 'quad_zeroed'])
@pytest.mark.parametrize('layer', wr.LAYERS, ids=wr.layer_id)
def test_mutant_weight_slots(layer, mut):
    if layer[0] == wr.WE_HEAD:
        p, _ = wr.emulate_head(layer, 257, 0, mut)
        _rejected(lambda: wr.check_head_p(p, layer, 257, mut))
    else:
        for form in wr.forms_of(layer):
            _conv_mutant_rejected(layer, form, mut)


@pytest.mark.parametrize('layer', PAD_LAYERS, ids=wr.layer_id)
def test_mutant_pad_channels_not_ignored(layer):
    assert len(PAD_LAYERS) == 4
    for form in wr.forms_of(layer):
        _conv_mutant_rejected(layer, form, 'pad_not_ignored')


@pytest.mark.parametrize('layer', HEAD_LAYERS, ids=wr.layer_id)
def test_mutant_head_fed_a_rounded_c(layer):
    p, _ = wr.emulate_head(layer, 257, 0, 'head_rounded_c')
    _rejected(lambda: wr.check_head_p(p, layer, 257, 'head_rounded_c'))


@pytest.mark.parametrize('layer', HEAD_LAYERS, ids=wr.layer_id)
def test_mutant_dead_lane_counted_into_the_partial(layer):
    """Row n - 1 a second time in the last block's partial, at the sizes whose last block is mostly dead."""
    for key in (1, 65, 257):
        for t_col in (0, 3, 7):
            p, part = wr.emulate_head(layer, key, t_col, 'dead_lane_counted')
            _rejected(lambda: wr.check_partial(part, p, wr.inputs(layer, key)['target'][:, t_col], 'dead lane'))


@pytest.mark.parametrize('name', sorted(wr.SCE_CASES))
def test_scale_context_emulation_is_accepted_and_truncation_rejected(name):
    k = wr.sce_case(name)
    sd = sr.state_dict_of(k['flat'], k['S'])
    x0 = torch.zeros(int(k['row_off'][-1]), 8)
    for j, si in enumerate(int(s) for s in k['sidx']):
        a, b = int(k['row_off'][j]), int(k['row_off'][j + 1])
        if b > a:
            x0[a:b] = onet.scale_context(sd, k['off'][a:b], si)
    wr.check_interval(wr.rb32(x0), k['iv'], 'scale context')
    if x0.shape[0] > 1:
        _rejected(lambda: wr.check_interval(wr.trunc32(x0), k['iv'], 'scale context, truncated'))
