"""GPU: the range coder's inputs computed on the device (linr_ac_codes, csrc/ac_codes.hip) and the opt-in codec path built on
them (model.frame_codes, codec.encode_gop(device_codes=True), run.py --device-codes).  Everything here is integer / byte work:
code values and symbol bits against the numpy statement of the formula, streams against the default path's streams, all exact."""
import filecmp
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def code_values(p):
    """binary_c1 of csrc/ac.cpp in numpy float32: fp32 1 - p, fp32 * 65534 (two roundings), round half to even, + 1, 16-bit wrap."""
    p = np.asarray(p, dtype=np.float32)
    return (((np.rint((np.float32(1) - p) * np.float32(65534)).astype(np.int64) + 1) & 0xFFFF)).astype(np.uint16)


def pack_symbols(s):
    bits = np.zeros(((len(s) + 31) // 32) * 32, dtype=np.uint8)
    bits[:len(s)] = np.asarray(s) != 0
    return np.packbits(bits, bitorder='little').view('<u4').astype(np.uint32)


def ac_codes(L, probs, probs_ld, occ, occ_ld, n, c1, c1_ld, sym, sym_ld):
    return L.linr_ac_codes(probs.data_ptr(), probs_ld, occ.data_ptr(), occ_ld, n, c1.data_ptr(), c1_ld, sym.data_ptr(), sym_ld,
                           torch.cuda.current_stream().cuda_stream)


def test_rounding_exhaustive(pkg):
    """Every fp32 in [0.5, 1.0] (2^23 + 1 values), every 61st bit pattern of [0, 0.5), and for each k in 0..65534 the fp32 nearest to
    the rounding boundary 1 - (k + 0.5) / 65534 with its two neighbours: the device's code value equals the numpy formula element for
    element.  (1 - p) * 65534 contracted into one fused multiply-add rounds once instead of twice and differs on some of them.)"""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    upper = np.arange(np.float32(0.5).view(np.uint32), np.float32(1.0).view(np.uint32) + 1, dtype=np.uint32).view(np.float32)
    assert upper.size == (1 << 23) + 1 and upper[0] == 0.5 and upper[-1] == 1.0
    lower = np.arange(0, np.float32(0.5).view(np.uint32), 61, dtype=np.uint32).view(np.float32)
    edge = (1.0 - (np.arange(65535, dtype=np.float64) + 0.5) / 65534.0).astype(np.float32)
    edges = np.concatenate([np.nextafter(edge, np.float32(-1)), edge, np.nextafter(edge, np.float32(2))])
    p = np.concatenate([upper, lower, edges]).astype(np.float32)
    n = p.size
    want = code_values(p)
    # what the test is able to tell apart: the single-rounding value differs from the formula somewhere in this set
    fused = ((np.rint((1.0 - p.astype(np.float64)) * 65534.0).astype(np.int64) + 1) & 0xFFFF).astype(np.uint16)
    assert int((fused != want).sum()) > 0
    probs = torch.full((8, n), 0.5, dtype=torch.float32, device='cuda')
    probs[0] = torch.from_numpy(p).cuda()
    occ = torch.zeros((n, 8), dtype=torch.float32, device='cuda')
    words = L.linr_ac_codes_sym_words(n)
    c1 = torch.empty((8, n), dtype=torch.uint16, device='cuda')
    sym = torch.empty((8, words), dtype=torch.uint32, device='cuda')
    assert ac_codes(L, probs, n, occ, 8, n, c1, n, sym, words) == 0
    got = c1[0].cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, 'first of %d: p = %r, device %d, formula %d' % (bad.size, p[bad[0]], got[bad[0]], want[bad[0]])
    assert bool((c1[1:].view(torch.int16) == -32768).all()) and not bool(sym.view(torch.int32).any())          # 0.5 -> 32768; no symbol set


@pytest.mark.parametrize('occ_ld', [8, 12])
def test_shapes_planes_pad_bits_and_untouched_padding(pkg, occ_ld):
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(occ_ld)
    for n in (1, 31, 32, 33, 63, 64, 65, 1000):
        ld = n + 3
        words = L.linr_ac_codes_sym_words(n)
        assert words == (n + 31) // 32
        sym_ld = words + 2
        p = rng.random((8, ld)).astype(np.float32)
        o = np.where(rng.random((n, occ_ld)) < 0.4, rng.choice(np.array([1.0, 0.25, -2.0], dtype=np.float32), (n, occ_ld)),
                     np.float32(0)).astype(np.float32)
        c1 = torch.from_numpy(np.full((8, ld), 0xFFFF, dtype=np.uint16)).cuda()
        sym = torch.from_numpy(np.full((8, sym_ld), 0xFFFFFFFF, dtype=np.uint32)).cuda()
        assert ac_codes(L, torch.from_numpy(p).cuda(), ld, torch.from_numpy(o).cuda(), occ_ld, n, c1, ld, sym, sym_ld) == 0
        c1, sym = c1.cpu().numpy(), sym.cpu().numpy()
        for k in range(8):
            assert np.array_equal(c1[k, :n], code_values(p[k, :n])), (n, k)
            assert np.array_equal(sym[k, :words], pack_symbols(o[:, k])), (n, k)
            if n % 32:
                assert int(sym[k, words - 1]) >> (n % 32) == 0          # pad bits of the last word
        assert (c1[:, n:] == 0xFFFF).all() and (sym[:, words:] == 0xFFFFFFFF).all()          # beyond n: left as they were


def test_bad_arguments_launch_nothing(pkg):
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    probs = torch.full((8, 40), 0.25, dtype=torch.float32, device='cuda')
    occ = torch.ones((40, 8), dtype=torch.float32, device='cuda')
    c1 = torch.from_numpy(np.full((8, 40), 0xFFFF, dtype=np.uint16)).cuda()
    sym = torch.from_numpy(np.full((8, 2), 0xFFFFFFFF, dtype=np.uint32)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    P, O, C, S = probs.data_ptr(), occ.data_ptr(), c1.data_ptr(), sym.data_ptr()
    for args in ((None, 40, O, 8, 40, C, 40, S, 2), (P, 40, None, 8, 40, C, 40, S, 2), (P, 40, O, 8, 40, None, 40, S, 2),
                 (P, 40, O, 8, 40, C, 40, None, 2), (P, 40, O, 8, -1, C, 40, S, 2), (P, 39, O, 8, 40, C, 40, S, 2),
                 (P, 40, O, 8, 40, C, 39, S, 2), (P, 40, O, 8, 40, C, 40, S, 1), (P, 40, O, 7, 40, C, 40, S, 2),
                 (P, (1 << 27) - 1, O, 8, (1 << 27) - 1, C, (1 << 27) - 1, S, 1 << 22)):
        assert L.linr_ac_codes(*args, st) == -1, args
    assert L.linr_ac_codes(P, 40, O, 8, 0, C, 40, S, 2, st) == 0
    torch.cuda.synchronize()
    assert (c1.cpu().numpy() == 0xFFFF).all() and (sym.cpu().numpy() == 0xFFFFFFFF).all()          # nothing was written


@pytest.fixture(scope='module')
def shell_gop(pkg, golden_dir):
    """Two frames of the golden 128-cube shell, an untrained model of seed 8807, and the default path's streams (fp32 and bf16)."""
    from linr_pcgc_amd import codec, overfit
    pts = np.load(os.path.join(golden_dir, 'octree_shell128.npz'))['points']
    gop = overfit.Gop(None, [pts, pts], None, 64, 'cuda')
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807)
    ref = {prec: codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda'), gop, 8, precision=prec) for prec in ('f32', 'bf16')}
    return gop, model, ref


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_device_codes_streams_are_the_default_streams(shell_gop, precision):
    from linr_pcgc_amd import codec, overfit
    gop, model, ref = shell_gop
    row_off = gop.frames[0].row_off
    assert any(int(r) % 32 for r in row_off[1:-1]), 'the ragged case: a scale that does not start on a word boundary'
    enc = codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda'), gop, 8, precision=precision, device_codes=True)
    assert enc['frames'] == ref[precision]['frames'] and len(enc['frames']) == 2 and len(enc['frames'][0]) == gop.frames[0].n_scales
    assert enc['model_bin'] == ref[precision]['model_bin'] and enc['side_info'] == ref[precision]['side_info']
    assert enc['low_enc_bytes'] == ref[precision]['low_enc_bytes'] and enc['bpp'] == ref[precision]['bpp']
    dec = codec.decode_gop(overfit.gen_model(gop.scale_num, 'cuda'), enc, 'cuda')
    for d, info, mn in zip(dec, gop.infos, gop.coord_mins):
        assert torch.equal(d, torch.as_tensor(info['ori']).cuda() + torch.tensor(mn, device='cuda', dtype=torch.int32))


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_frame_codes_are_the_code_values_of_frame_probs(shell_gop, precision):
    from linr_pcgc_amd.model_codec import Model_Estimate
    from linr_pcgc_amd.model_core import codes_word_off
    from linr_pcgc_amd import overfit
    gop, model, _ = shell_gop
    coded = Model_Estimate().compress_model(model, 8, True, overfit.gen_model(gop.scale_num, 'cuda'))['new_model']
    f = gop.frames[0]
    probs, bits = coded.frame_probs(f, precision)
    c1, sym, bits_c = coded.frame_codes(f, precision)
    assert c1.dtype == torch.uint16 and tuple(c1.shape) == (8, f.rows) and sym.dtype == torch.uint32
    assert torch.equal(bits, bits_c)
    assert np.array_equal(c1.cpu().numpy(), code_values(probs.cpu().numpy()))
    woff = codes_word_off(f.row_off)
    assert tuple(sym.shape) == (8, int(woff[-1]))
    occ, sym = f.occ.cpu().numpy(), sym.cpu().numpy()
    for i in range(f.n_scales):
        a, b = int(f.row_off[i]), int(f.row_off[i + 1])
        for k in range(8):
            assert np.array_equal(sym[k, woff[i]:woff[i + 1]], pack_symbols(occ[a:b, k])), (i, k)


def test_run_device_codes_writes_identical_files(pkg, golden_dir, tmp_path):
    """run.py --device-codes on the same tiny configuration (the two shell frames as one GOP, read from files, one epoch): every file
    under result_enc/ is the file a run without the flag writes."""
    from linr_pcgc_amd import run
    pts = np.load(os.path.join(golden_dir, 'octree_shell128.npz'))['points']
    for t in range(2):
        np.save(str(tmp_path / ('frame%d.npy' % t)), pts)
    outs = []
    for flag in ([], ['--device-codes']):
        out = str(tmp_path / ('codes' if flag else 'plain'))
        args = run.parse(['--input-glob', str(tmp_path / 'frame*.npy'), '--frames', '2', '--gop', '2', '--first-epoch', '1', '--seed', '8807',
                          '--out', out] + flag)
        assert args.device_codes is bool(flag)
        summary, _ = run.run_sequence_job(args, files=run.resolve_files(args))
        assert summary['gops'] == 1 and summary['frames'] == 2
        outs.append(os.path.join(out, 'result_enc'))
    names = sorted(os.path.relpath(os.path.join(d, f), outs[0]) for d, _, fs in os.walk(outs[0]) for f in fs)
    assert names == sorted(os.path.relpath(os.path.join(d, f), outs[1]) for d, _, fs in os.walk(outs[1]) for f in fs)
    assert len(names) == 2 * 5 + 3                          # frames x scales streams, model.bin, low_enc_bytes.bin, side_info.json
    for n in names:
        assert filecmp.cmp(os.path.join(outs[0], n), os.path.join(outs[1], n), shallow=False), n
