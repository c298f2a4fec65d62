"""GPU tests of the opt-in rate-checked quantiser range: the kernel (linr_params_fake_quant_ranges) against its host twin, the search
(codec.search_qrange, codec.encode_gop qrange_search=) on a model with a planted outlier weight and against its own objective
recomputed through the public API, round trips through the unchanged decoders, and the drivers.

Everything here is exact.  The quantiser is individually rounded fp32 operations on given bounds and its statistics are integer sums,
so kernel and host twin agree bit for bit; a candidate's bits come from the codec's deterministic forward on bit-identical weights, so
a recomputed objective is the recorded one; streams are bytes.  No rate gain is asserted on real weights (profiles/qrange_ab.txt holds
that measurement): the one rate assertion is on an outlier planted in a weight the frames never read, where clipping it MUST win."""
import filecmp
import json
import os

import numpy as np
import pytest
import torch

from gpu_common import _dev                                                            # noqa: E402
from test_fake_quant_host import fake_quant_host                                       # noqa: E402
from test_qrange_host import POISON_C, POISON_Q, outliers, ranges_host, some_ranges    # noqa: E402

pytestmark = pytest.mark.gpu

# 65,536 floats (FQ_HELD) is what a workgroup keeps in registers between the two passes; above it the stride loop runs twice; n % 4
# floats form the tail.  54,712: the model at scale_num 7.
NS = (1, 3, 4, 7, 4096, 65533, 65536, 65537, 65543, 54712)


def _device_ranges(p, bitdepth, ranges, stride=None, codes=True, stats=True):
    """The kernel on poisoned [K][stride] outputs -> full host arrays (padding included)."""
    from linr_pcgc_amd import _lib
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32).reshape(-1, 2))
    K, n = r.shape[0], p.size
    stride = (n + 3) & ~3 if stride is None else stride
    dp = torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).to(_dev())
    q = torch.full((K, stride), POISON_Q, dtype=torch.float32, device=_dev())
    c = torch.from_numpy(np.full((K, stride), POISON_C, dtype=np.uint16)).to(_dev()) if codes else None
    st = torch.full((K, 4), -7, dtype=torch.int64, device=_dev()) if stats else None
    _lib.check(_lib.lib().linr_params_fake_quant_ranges(dp.data_ptr(), n, bitdepth, r.ctypes.data, K, stride, q.data_ptr(),
                                                        None if c is None else c.data_ptr(), None if st is None else st.data_ptr(),
                                                        _lib.current_stream_handle()), 'linr_params_fake_quant_ranges')
    return q.cpu().numpy(), None if c is None else c.cpu().numpy(), None if st is None else st.cpu().numpy()


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize('K', [1, 8, 16])
def test_kernel_equals_host_twin_bitwise(pkg, K):
    from linr_pcgc_amd import _lib
    lib = _lib.lib()
    for i, n in enumerate(NS):
        bitdepth = (8, 2, 16)[i % 3] if n != 54712 else 8
        p = outliers(n, 17 * n + K, nan=n >= 7)
        r = some_ranges(p, K)
        hq, hc, hst = ranges_host(lib, p, bitdepth, r)
        dq, dc, dst = _device_ranges(p, bitdepth, r)
        assert _same(dq, hq) and _same(dc, hc) and _same(dst, hst), (n, bitdepth)          # padding included: still the poison
        if n >= 7:
            assert np.isnan(dq[:, 1]).all() and not dc[:, 1].any()
    # all three depths where the paths change over
    for n in (65536, 65537):
        for bitdepth in (2, 8, 16):
            p = outliers(n, n + bitdepth)
            r = some_ranges(p, K)
            assert all(_same(d, h) for d, h in zip(_device_ranges(p, bitdepth, r), ranges_host(lib, p, bitdepth, r))), (n, bitdepth)


def test_kernel_optional_outputs_and_padding(pkg):
    from linr_pcgc_amd import _lib
    lib = _lib.lib()
    for n in (4099, 65543):
        p = outliers(n, n)
        r = some_ranges(p, 8)
        stride = ((n + 3) & ~3) + 12
        hq, hc, hst = ranges_host(lib, p, 8, r, stride)
        dq, dc, dst = _device_ranges(p, 8, r, stride)
        assert _same(dq, hq) and _same(dc, hc) and _same(dst, hst)
        assert np.all(dq[:, n:] == POISON_Q) and np.all(dc[:, n:] == POISON_C)             # stride > n: the padding is left alone
        q1, c1, s1 = _device_ranges(p, 8, r, stride, codes=False)
        assert c1 is None and _same(q1, hq) and _same(s1, hst)
        q2, c2, s2 = _device_ranges(p, 8, r, stride, stats=False)
        assert s2 is None and _same(q2, hq) and _same(c2, hc)
        q3, _, _ = _device_ranges(p, 8, r, stride, codes=False, stats=False)
        assert _same(q3, hq)
    # an all-equal vector, and a candidate with lo == hi
    p = np.full(1025, 0.25, dtype=np.float32)
    r = [(0.25, 0.25), (0.0, 1.0), (0.5, 0.5)]
    assert all(_same(d, h) for d, h in zip(_device_ranges(p, 8, r), ranges_host(lib, p, 8, r)))


@pytest.mark.parametrize('bitdepth', [2, 8, 16])
def test_true_range_candidate_is_the_plain_kernel(pkg, golden_dir, bitdepth):
    from linr_pcgc_amd import engine
    flat = np.load(os.path.join(golden_dir, 'loot_model_kat.npz'))['flat'].astype(np.float32)
    for p in (flat, outliers(65543, 3, nan=True), outliers(7, 4)):
        q0, c0, mm = engine.params_fake_quant(torch.from_numpy(p).to(_dev()), bitdepth, codes=True)
        mm = mm.cpu().numpy()
        n = p.size
        q, c, st = _device_ranges(p, bitdepth, [(mm[0], mm[1])])
        assert _same(q[0, :n], q0.cpu().numpy()) and _same(c[0, :n], c0.cpu().numpy())
        assert st[0, 0] == 0 and st[0, 1] == 0 and st[0, 2] == int(c0.cpu().numpy().astype(np.int64).sum())
    q, c, st = engine.params_fake_quant_ranges(torch.from_numpy(flat).to(_dev()), [(float(flat.min()), float(flat.max()))], 8)
    hq, hc, _ = fake_quant_host(pkg._lib.lib(), flat, 8)
    assert _same(q.cpu().numpy()[0, :flat.size], hq) and _same(c.cpu().numpy()[0, :flat.size], hc)


# ---- the search ---------------------------------------------------------------------------------------------------------------------
def _unused_rows(model):
    """Flat indices of the last row of the scale embedding: the parameters of a scale no frame of the GOP has."""
    off = 0
    for name, p in model.named_parameters():
        if name == 'scale_emb.weight':
            return list(range(off + 8 * (model.scale_num - 1), off + 8 * model.scale_num))
        off += p.numel()
    raise AssertionError('no scale embedding')


def _neutralise(model):
    """The unused embedding row := the smallest parameter, so that the minimum stands three times or more; returns the row's indices."""
    idx = _unused_rows(model)
    flat = model.flat_parameters()
    with torch.no_grad():
        flat[idx] = flat.min()
    return idx


def _plant(model, idx):
    """+ 100 x the parameter range on ONE unused parameter: the maximum by far, and nothing the frames read."""
    flat = model.flat_parameters()
    with torch.no_grad():
        flat[idx[0]] += 100.0 * (flat.max() - flat.min())


def _small_gop(overfit, synthetic, hidden=8):
    """Two small shells whose octrees stop one level or more short of the model's scale_num."""
    clouds = [synthetic.sphere_shell(7, 40), synthetic.sphere_shell(7, 41)]
    natural = overfit.Gop(None, clouds, None, 64, 'cuda').scale_num
    gop = overfit.Gop(None, clouds, natural, 1024, 'cuda')
    assert gop.scale_num == natural and all(f.n_scales < natural for f in gop.frames)
    return gop


def _total_bytes(enc):
    return sum(len(b) for f in enc['frames'] for b in f) + len(enc['model_bin'])


def _lossless(codec, overfit, gop, enc, hidden=8, **kw):
    dec = codec.decode_gop(overfit.gen_model(gop.scale_num, 'cuda', hidden=hidden), enc, 'cuda', **kw)
    assert len(dec) == len(gop.frames)
    for i, d in enumerate(dec):
        ref = torch.as_tensor(gop.infos[i]['ori']).cuda() + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32)
        assert torch.equal(d, ref), i


@pytest.fixture(scope='module')
def planted(pkg):
    """A small GOP, a model overfitted on it for a few epochs whose unused embedding row is neutral, and the same model with the
    outlier planted."""
    from linr_pcgc_amd import overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam
    gop = _small_gop(overfit, synthetic)
    clean = overfit.gen_model(gop.scale_num, 'cuda', seed=8807)
    overfit.overfit_gop(clean, FlatAdam(clean), gop, 3, keep='best', info={})
    idx = _neutralise(clean)
    dirty = overfit.gen_model(gop.scale_num, 'cuda')
    with torch.no_grad():
        dirty.flat_parameters().copy_(clean.flat_parameters())
    _plant(dirty, idx)
    return gop, clean, dirty


def test_planted_outlier_is_clipped(planted):
    from linr_pcgc_amd import codec, overfit
    gop, clean, dirty = planted
    shell = lambda: overfit.gen_model(gop.scale_num, 'cuda')
    ref = codec.encode_gop(clean, shell(), gop, 8)
    plain = codec.encode_gop(dirty, shell(), gop, 8)
    frames = lambda enc: sum(len(b) for f in enc['frames'] for b in f)
    print('frame bytes: clean %d, planted plain %d' % (frames(ref), frames(plain)))
    assert frames(plain) > frames(ref)                       # one step of the quantiser now spans 100 x the weights' range: a ruined rate
    # the default trims, every frame evaluated
    found = codec.encode_gop(dirty, shell(), gop, 8, qrange_search=True, qrange_frames=0)
    print('default trims: chosen %d, objective %s, total bytes %d vs plain %d' % (found['qrange']['chosen'], found['qrange']['objective_bits'],
                                                                                  _total_bytes(found), _total_bytes(plain)))
    assert found['qrange']['chosen'] >= 1 and found['side_info']['qrange_trim'] == found['qrange']['chosen']
    assert found['side_info']['qrange_candidates'] == len(found['qrange']['trims']) == 8
    assert _total_bytes(found) < _total_bytes(plain)
    _lossless(codec, overfit, gop, found)
    # trims (0, 1): the range without the outlier is the clean model's own (its minimum stands more than once), every weight the frames
    # read has the clean model's code, and the streams are the clean model's streams
    one = codec.encode_gop(dirty, shell(), gop, 8, qrange_search=True, qrange_trims=(0, 1), qrange_frames=0)
    assert one['qrange']['trims'] == [0, 1] and one['qrange']['chosen'] == 1
    assert (one['side_info']['min_param'], one['side_info']['max_param']) == (ref['side_info']['min_param'], ref['side_info']['max_param'])
    assert one['frames'] == ref['frames']
    assert _total_bytes(one) < _total_bytes(plain)
    assert one['qrange']['objective_bits'][1] < one['qrange']['objective_bits'][0] and one['qrange']['search_s'] > 0


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_the_choice_is_honest(pkg, seed):
    """The recorded objective of every candidate, recomputed through the public API: compress_model(qrange=)'s new_model, frame_probs
    on the evaluated frames, laplace_bits_est from the codes.  3 frames of which 2 are evaluated: the up-scaling counts."""
    from linr_pcgc_amd import codec, overfit, synthetic
    from linr_pcgc_amd.model_codec import DEFAULT_QRANGE_TRIMS, Model_Estimate, candidate_ranges, laplace_bits_est
    from linr_pcgc_amd.model_core import FlatAdam
    gop = overfit.Gop(None, [synthetic.sphere_shell(7, 40 + t) for t in range(3)], None, 64, 'cuda')
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=seed)
    overfit.overfit_gop(model, FlatAdam(model), gop, 2, keep='best', info={})
    enc = codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda'), gop, 8, qrange_search=True, qrange_frames=2)
    got = enc['qrange']
    trims, ranges = candidate_ranges(model.flat_parameters().detach().cpu())
    assert got['trims'] == trims == list(DEFAULT_QRANGE_TRIMS)
    todo = codec.qrange_eval_frames(3, 2)
    assert todo == [0, 2]
    n = model.flat_parameters().numel()
    want = []
    for lo, hi in ranges:
        out = Model_Estimate().compress_model(model, 8, True, overfit.gen_model(gop.scale_num, 'cuda'), qrange=(lo, hi))
        cand = out['new_model']
        bits = float(torch.stack([cand.frame_probs(gop.frames[i])[1] for i in todo]).sum())
        dev = int(np.abs(out['symbols'].astype(np.int64) - int(out['mu'])).sum())
        want.append(laplace_bits_est(n, dev, 8) + 3 / 2 * bits)
    print('seed %d: objective %s, chosen %d' % (seed, got['objective_bits'], got['chosen']))
    assert got['objective_bits'] == want
    best = min(range(len(want)), key=lambda j: (want[j], j))             # a tie goes to the smaller trim
    assert got['chosen'] == trims[best]
    assert want[best] <= want[0]
    lo, hi = ranges[best]
    assert (enc['side_info']['min_param'], enc['side_info']['max_param']) == (lo, hi)
    assert enc['side_info']['qrange_trim'] == trims[best] and enc['side_info']['qrange_candidates'] == len(trims)


@pytest.mark.parametrize('precision,hidden', [('f32', 8), ('bf16', 8), ('f32', 16)])
def test_round_trip_through_the_unchanged_decoders(pkg, planted, tmp_path, precision, hidden):
    from linr_pcgc_amd import codec, overfit
    from linr_pcgc_amd.model_codec import candidate_ranges
    gop, _, dirty = planted
    if hidden == 8:
        model = dirty
    else:
        model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807, hidden=hidden)
        _plant(model, _neutralise(model))
    trims = None if hidden == 8 else (0, 1, 2)               # (the channel-blocked executor is several times slower)
    enc = codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda', hidden=hidden), gop, 8, precision=precision,
                           qrange_search=True, qrange_trims=trims)
    chosen = enc['qrange']['chosen']
    assert chosen >= 1
    kept, ranges = candidate_ranges(model.flat_parameters().detach().cpu(), trims)
    lo, hi = ranges[kept.index(chosen)]
    codec.write_gop(enc, str(tmp_path / 'enc'))
    side = json.load(open(str(tmp_path / 'enc' / 'side_info.json')))
    assert (side['min_param'], side['max_param']) == (lo, hi) and side['qrange_trim'] == chosen
    assert side.get('precision', 'f32') == precision
    back = codec.read_gop(str(tmp_path / 'enc'))
    _lossless(codec, overfit, gop, back, hidden)
    _lossless(codec, overfit, gop, back, hidden, lockstep=4)


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_off_means_off(planted, tmp_path):
    from linr_pcgc_amd import codec, overfit
    gop, clean, _ = planted
    plain = codec.encode_gop(clean, overfit.gen_model(gop.scale_num, 'cuda'), gop, 8)
    only0 = codec.encode_gop(clean, overfit.gen_model(gop.scale_num, 'cuda'), gop, 8, qrange_search=True, qrange_trims=(0,))
    assert 'qrange' not in plain and only0['qrange']['trims'] == [0] and only0['qrange']['chosen'] == 0
    codec.write_gop(plain, str(tmp_path / 'plain'))
    codec.write_gop(only0, str(tmp_path / 'only0'))
    names = _tree(str(tmp_path / 'plain'))
    assert names == _tree(str(tmp_path / 'only0')) and 'side_info.json' in names
    for n in names:
        assert filecmp.cmp(str(tmp_path / 'plain' / n), str(tmp_path / 'only0' / n), shallow=False), n


def test_run_with_search_under_the_pipeline(pkg, tmp_path):
    """run.py --qrange-search --decode on a 2-GOP sequence, with and without --pipeline: lossless, and the same files."""
    from linr_pcgc_amd import run
    outs = []
    for flag in ([], ['--pipeline']):
        out = str(tmp_path / ('pipe' if flag else 'plain'))
        args = run.parse(['--config', 'sphere8', '--frames', '4', '--gop', '2', '--first-epoch', '2', '--others-epoch', '1', '--qrange-search',
                          '--qrange-trims', '0,1,2,4', '--decode', '--out', out] + flag)
        summary, results = run.run_sequence_job(args, 0, 1, None)
        assert summary['lossless'] is True and summary['gops'] == 2
        assert all(r['qrange']['trims'] == [0, 1, 2, 4] and r['qrange']['chosen'] in (0, 1, 2, 4) for r in results.values())
        outs.append(os.path.join(out, 'result_enc'))
    names = _tree(outs[0])
    assert names == _tree(outs[1]) and len(names) > 6
    for n in names:
        assert filecmp.cmp(os.path.join(outs[0], n), os.path.join(outs[1], n), shallow=False), n


def test_encoder_mirror_reads_the_same_key(pkg, tmp_path):
    """encoder.encode with the reference's argument dict + 'qrange_search' (default off): the planted outlier is clipped on that road
    too, and decoder.decode - unchanged, comparing with the data set - rebuilds every frame from either set of files."""
    from linr_pcgc_amd import custom_dataset as cd, decoder, encoder, synthetic
    from linr_pcgc_amd.model_core import LINR_PCGC_Model
    ori = tmp_path / 'ori'
    ori.mkdir()
    for t in range(2):
        np.save(str(ori / ('frame_%04d.npy' % t)), synthetic.sphere_shell(7, 40 + t))
        cd.write_ply_ascii(str(ori / ('frame_%04d.ply' % t)), synthetic.sphere_shell(7, 40 + t))
    dataset = cd.MyDataset(str(ori), str(tmp_path / 'handle'), None, 'npy', stage=8)
    dataset.set_prefix_data({'offsets_ini': torch.tensor(cd.OFFSETS_INI, device='cuda'), 'min_point_num': 64})
    dataset[0]
    gen = lambda: LINR_PCGC_Model({'scale_num': dataset.scale_num + 1, 'in_channel': 7, 'hidden_channel_conv': 8, 'block_layers': 1,
                                   'outstage': 8, 'instage': 1}).cuda()                    # one scale more than any frame has
    torch.manual_seed(8807)
    model = gen()
    _plant(model, _neutralise(model))
    out_dir = tmp_path / 'output' / 'gop_0_1'
    out_dir.mkdir(parents=True)
    torch.save({'model': model.state_dict(), 'epoch': 0, 'loss': 0.0, 'bitdepth': 8}, str(out_dir / 'model.pth'))
    test_set = cd.MytestDataset(str(ori), ori_type='ply')
    size, side = {}, {}
    for name, extra in (('plain', {}), ('off', {'qrange_search': False}), ('search', {'qrange_search': True, 'qrange_trims': (0, 1, 2), 'qrange_frames': 0})):
        enc_dir = tmp_path / name
        encoder.encode({'outputdir': str(tmp_path / 'output'), 'gop_names': ['gop_0_1'], 'Gen_Model': gen, 'dataset': dataset,
                        'encode_dir': str(enc_dir), **extra})
        decoder.decode({'gop_names': ['gop_0_1'], 'Gen_Model': gen, 'result_enc_dir': str(enc_dir), 'result_dec_dir': str(tmp_path / ('dec_' + name)),
                        'dataset': test_set, 'write_flag': False})
        files = _tree(str(enc_dir))
        size[name] = sum(os.path.getsize(str(enc_dir / f)) for f in files if f.endswith('.bin'))
        side[name] = json.load(open(str(enc_dir / 'gop_0_1' / 'side_info.json')))
    assert side['off'] == side['plain'] and 'qrange_trim' not in side['plain']
    for f in _tree(str(tmp_path / 'plain')):
        assert filecmp.cmp(str(tmp_path / 'plain' / f), str(tmp_path / 'off' / f), shallow=False), f
    assert side['search']['qrange_trim'] >= 1 and side['search']['qrange_candidates'] == 3
    assert side['search']['max_param'] < side['plain']['max_param'] and side['search']['min_param'] == side['plain']['min_param']
    print('encoder mirror: .bin bytes plain %d, search %d' % (size['plain'], size['search']))
    assert size['search'] < size['plain']


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_search_composes_with_device_codes_and_device_coder(planted, precision):
    """Everything behind the choice of the range is the unchanged encoder: the same streams whichever way they are coded."""
    from linr_pcgc_amd import codec, overfit
    gop, _, dirty = planted
    shell = lambda: overfit.gen_model(gop.scale_num, 'cuda')
    ref = codec.encode_gop(dirty, shell(), gop, 8, precision=precision, qrange_search=True)
    assert ref['qrange']['chosen'] >= 1
    for kw in ({'device_codes': True}, {'device_coder': True, 'coder_group': 2}):
        enc = codec.encode_gop(dirty, shell(), gop, 8, precision=precision, qrange_search=True, **kw)
        assert enc['frames'] == ref['frames'] and enc['model_bin'] == ref['model_bin'] and enc['side_info'] == ref['side_info']
        assert enc['qrange']['chosen'] == ref['qrange']['chosen'] and enc['qrange']['objective_bits'] == ref['qrange']['objective_bits']
