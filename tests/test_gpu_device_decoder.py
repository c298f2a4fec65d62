"""GPU: the device range decoder (opt-in; codec.decode_gop device_decoder=True).  The kernel (linr_rc_decode_probs, csrc/ac_device_dec.hip:
a wave per entry) against the host decoder (linr_ac_decode_binary) on entries packed back to back at odd and even byte offsets, the
decoder's scale entries with the device decoders (linr_decode_opts.device of linr_decode_scale, linr_decode_scale_batch) against the default ones, and the paths that
carry the option: codec.decode_gop, run.py --decode --device-decoder, python -m linr_pcgc_amd.decoder --device-decoder, decoder.decode.
Symbols, untouched sentinels and decoded geometry, all exact; no rate and no time is asserted."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_device_coder_host import REGIMES, draw                                   # noqa: E402
from test_gpu_stream_chunks import _same_files, _shell, _truth, shell_gop, stream_lengths      # noqa: E402,F401
from test_rc_decode_host import decode, encode, garbage_cases, p_for_c1             # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 7.5            # of the occupancy matrix
SENT_U8 = 0xA5
COLUMN = 5
GAP = 3                   # rows between two entries that nothing may touch


# ---- the kernel --------------------------------------------------------------------------------------------------------------

def pack_entries(items, lead_bytes=3, lead_probs=7):
    """items: [(p float32 [n], stream bytes)].  One probability buffer and one byte buffer with the entries back to back behind
    non-zero leads, the byte buffer padded to a multiple of 4 with non-zero bytes, rows GAP apart: (probs, data, table, rows)."""
    ps, bs, tab = [np.full(lead_probs, 0.25, dtype=np.float32)], [np.full(lead_bytes, 0xFF, dtype=np.uint8)], []
    p_at, b_at, row = lead_probs, lead_bytes, 1
    for p, data in items:
        tab.append((p_at, len(p), b_at, len(data), row))
        ps.append(np.asarray(p, dtype=np.float32))
        bs.append(np.frombuffer(bytes(data), dtype=np.uint8))
        p_at, b_at, row = p_at + len(p), b_at + len(data), row + len(p) + GAP
    data = np.concatenate(bs)
    data = np.concatenate([data, np.full((-len(data)) % 4 + 4, 0xEE, dtype=np.uint8)])
    return np.concatenate(ps), data, np.asarray(tab, dtype=np.int64), row


def run_kernel(pkg, probs, data, tab, rows, with_plane):
    from linr_pcgc_amd.model_core import rc_decode_probs
    occ = torch.full((rows, 8), SENTINEL, dtype=torch.float32, device='cuda')
    sym = torch.full((rows,), SENT_U8, dtype=torch.uint8, device='cuda') if with_plane else None
    rc_decode_probs(torch.from_numpy(probs).cuda(), torch.from_numpy(data).cuda(), tab, occ, COLUMN, sym)
    torch.cuda.synchronize()
    return occ, sym


def check_kernel(lib, items, tab, rows, occ, sym):
    occ = occ.cpu().numpy()
    want = np.full((rows, 8), SENTINEL, dtype=np.float32)
    want_u8 = np.full(rows, SENT_U8, dtype=np.uint8)
    for (p, data), (_, n, _, _, row) in zip(items, tab):
        s = decode(lib.linr_ac_decode_binary, p, data)
        want[row:row + n, COLUMN] = s
        want_u8[row:row + n] = s
    bad = np.argwhere(occ != want)
    assert bad.size == 0, ('first difference (row, column)', bad[0].tolist())
    if sym is not None:
        assert np.array_equal(sym.cpu().numpy(), want_u8)


@pytest.mark.parametrize('S', [64, 128])
def test_kernel_gives_the_host_decoders_symbols(pkg, S):
    from linr_pcgc_amd import _lib
    lib = _lib.lib()
    items = []
    for r, n in enumerate(stream_lengths(S) + [20000]):
        c1, s = draw(REGIMES[r % len(REGIMES)], n, 23 * S + r)
        p = p_for_c1(c1)
        items.append((p, encode(lib, p, s)))
    probs, data, tab, rows = pack_entries(items)
    assert {int(o) % 2 for o in tab[:, 2]} == {0, 1} and {int(o) % 4 for o in tab[:, 2]} == {0, 1, 2, 3}
    assert any(int(o) % 64 for o in tab[:, 0]) and len(data) > 3 * 256
    occ, sym = run_kernel(pkg, probs, data, tab, rows, True)
    check_kernel(lib, items, tab, rows, occ, sym)
    occ2, sym2 = run_kernel(pkg, probs, data, tab, rows, True)          # a second call gives the same result bit for bit
    assert torch.equal(occ, occ2) and torch.equal(sym, sym2)
    occ3, none = run_kernel(pkg, probs, data, tab, rows, False)         # without the byte plane: the same column
    assert none is None and torch.equal(occ, occ3)


def test_kernel_on_bytes_that_are_no_streams(pkg):
    from linr_pcgc_amd import _lib
    lib = _lib.lib()
    items = list(garbage_cases())
    for regime in REGIMES:
        c1, s = draw(regime, 300, 41)
        p = p_for_c1(c1)
        data = encode(lib, p, s)
        items += [(p, data[:cut]) for cut in range(0, min(16, len(data)) + 1)]
    for lead in (0, 1, 2, 3):
        probs, data, tab, rows = pack_entries(items, lead_bytes=lead)
        occ, sym = run_kernel(pkg, probs, data, tab, rows, True)
        check_kernel(lib, items, tab, rows, occ, sym)


def test_entry_refuses_a_bad_table_and_writes_nothing(pkg):
    from linr_pcgc_amd import _lib
    from linr_pcgc_amd.model_core import rc_decode_probs
    occ = torch.full((40, 8), SENTINEL, dtype=torch.float32, device='cuda')
    probs = torch.full((64,), 0.5, dtype=torch.float32, device='cuda')
    data = torch.zeros(16, dtype=torch.uint8, device='cuda')
    for tab in ([(0, 20, 0, 8, 0), (20, 20, 8, 8, 19)], [(0, 65, 0, 8, 0)], [(0, 20, 0, 17, 0)], [(0, 20, 0, 8, 21)]):
        with pytest.raises(_lib.LinrError, match='LINR_EINVAL'):
            rc_decode_probs(probs, data, tab, occ, COLUMN)
    rc_decode_probs(probs, data, np.zeros((0, 5), dtype=np.int64), occ, COLUMN)          # no entries: nothing happens
    torch.cuda.synchronize()
    assert bool((occ == SENTINEL).all())


# ---- the scale entries ---------------------------------------------------------------------------------------------------------

def _decoder_model(gop, enc):
    """The model as decode_gop rebuilds it from model.bin."""
    from linr_pcgc_amd.model_codec import Model_Estimate
    side = dict(enc['side_info'])
    side.pop('arith_version', None)
    side['final_bytes'] = enc['model_bin']
    model, _ = Model_Estimate().decompress_model(_shell(gop), side)
    model.inference_precision = side.get('precision', 'f32')
    return model


def _lows(enc):
    from linr_pcgc_amd import codec
    lows, _ = codec.dec_all_frame_low_xyz(enc['low_enc_bytes'])
    return [codec.unique_sorted(torch.tensor(x.astype(np.int32), device='cuda')) for x in lows]


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
@pytest.mark.parametrize('S', [0, 64])
def test_scale_entries_give_the_default_entries_coordinates(shell_gop, precision, S):
    """Every scale of frame 0, coarse to fine: decode_scale(device_decoder=True) against the default call on the same level; then the
    same through decode_scale_batch for three frames, the middle one empty."""
    gop, _, plain, host = shell_gop
    enc = host[precision, S] if S else plain[precision]
    model = _decoder_model(gop, enc)
    lows = _lows(enc)
    f0 = list(enc['frames'][0])
    low, bits = lows[0], max(1, int(lows[0].max()).bit_length())
    for s_idx in range(len(f0) - 1, -1, -1):
        bits = min(bits + 1, 21)
        want = model.decode_scale(low, s_idx, f0[s_idx], bits, S, 4)
        got = model.decode_scale(low, s_idx, f0[s_idx], bits, S, 4, device_decoder=True)
        assert got.dtype == want.dtype and torch.equal(got, want), s_idx
        low = want
    assert torch.equal(low + torch.tensor(gop.coord_mins[0], device='cuda', dtype=torch.int32), _truth(gop, 0))
    group = [lows[0], lows[0].new_zeros((0, 3)), lows[2]]
    f2 = list(enc['frames'][2])
    for s_idx in range(len(f0) - 1, -1, -1):
        encs = [f0[s_idx], f0[s_idx], f2[s_idx]]            # (the empty frame's streams are not read)
        want = model.decode_scale_batch(group, s_idx, encs, 4, S)
        got = model.decode_scale_batch(group, s_idx, encs, 4, S, device_decoder=True)
        assert len(got) == 3 and got[1].shape == (0, 3)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), s_idx
        group = want
    assert torch.equal(group[2] + torch.tensor(gop.coord_mins[2], device='cuda', dtype=torch.int32), _truth(gop, 2))


# ---- the codec path ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', ['f32', 'bf16'])
@pytest.mark.parametrize('S', [0, 64, 128])
def test_gop_round_trip_with_the_device_decoder(shell_gop, precision, S):
    from linr_pcgc_amd import codec
    gop, _, plain, host = shell_gop
    enc = host[precision, S] if S else plain[precision]
    ref = codec.decode_gop(_shell(gop), enc, 'cuda')
    for kw in (dict(workers=1), dict(workers=2), dict(lockstep=3), dict(workers=2, n_threads=4)):
        got = codec.decode_gop(_shell(gop), enc, 'cuda', device_decoder=True, **kw)
        assert len(got) == 3
        for i in range(3):
            assert torch.equal(got[i], ref[i]), (kw, i)
            assert torch.equal(got[i], _truth(gop, i)), (kw, i)
    assert 'device_decoder' not in enc['side_info']          # nothing travels in the stream


def test_wide_models_are_refused(pkg):
    from linr_pcgc_amd import codec, overfit, synthetic
    small = overfit.Gop(None, [synthetic.sphere_shell(6, 20)], None, 64, 'cuda')
    wide = overfit.gen_model(small.scale_num, 'cuda', seed=8807, hidden=16)
    enc = codec.encode_gop(wide, _shell(small, 16), small, 8)
    with pytest.raises(ValueError, match='hidden_channel_conv'):
        codec.decode_gop(_shell(small, 16), enc, 'cuda', device_decoder=True)
    with pytest.raises(ValueError, match='hidden_channel_conv'):
        codec.decode_gop(_shell(small, 16), enc, 'cuda', device_decoder=True, lockstep=2)
    assert len(codec.decode_gop(_shell(small, 16), enc, 'cuda')) == 1


def test_a_corrupted_chunk_header_is_still_refused(shell_gop, tmp_path):
    """As tests/test_gpu_stream_chunks.py's: the first length of stage 0's stream of the finest scale of frame 1 rewritten on disk;
    with the device decoder decode_gop raises LinrError in front of the scale's first launch, per frame and in lock step."""
    from linr_pcgc_amd import _lib, codec
    from linr_pcgc_amd.function_utils import pack_bitstream, unpack_bitstream
    from linr_pcgc_amd.stream_chunks import leb128
    gop, _, _, host = shell_gop
    root = str(tmp_path / 'enc')
    codec.write_gop(host['f32', 64], root)
    path = os.path.join(root, 'bins', 'frame0001_scale0.bin')
    streams = unpack_bitstream(open(path, 'rb').read())
    for head in (b'\xff' * 5, leb128(len(streams[0]) + 1)):
        first = 0
        while streams[0][first] & 0x80:
            first += 1
        with open(path, 'wb') as f:
            f.write(pack_bitstream([head + streams[0][first + 1:]] + streams[1:]))
        enc = codec.read_gop(root)
        for kw in ({}, {'workers': 2}, {'lockstep': 3}):
            with pytest.raises(_lib.LinrError, match='LINR_EINVAL'):
                codec.decode_gop(_shell(gop), enc, 'cuda', device_decoder=True, **kw)
        dec = codec.decode_gop(_shell(gop), enc, 'cuda', frames=[0, 2], device_decoder=True)          # the other frames are fine
        assert torch.equal(dec[0], _truth(gop, 0)) and torch.equal(dec[1], _truth(gop, 2))


# ---- the drivers -------------------------------------------------------------------------------------------------------------

def test_drivers_carry_the_option(pkg, golden_dir, tmp_path):
    """run.py --decode --device-decoder on two GOPs of two frames, alone and with --pipeline --decode-lockstep 2: lossless, and the files
    of the run without the flag; python -m linr_pcgc_amd.decoder --device-decoder rebuilds every frame in another process, and
    decoder.decode with the key 'device_decoder' does."""
    from linr_pcgc_amd import custom_dataset as cd, decoder, run
    from linr_pcgc_amd.model_core import LINR_PCGC_Model
    pts = np.unique(np.load(os.path.join(golden_dir, 'octree_shell128.npz'))['points'], axis=0)
    ori = tmp_path / 'ori'
    ori.mkdir()
    for t in range(4):
        cd.write_ply_ascii(str(ori / ('frame_%04d.ply' % t)), pts + t)
    outs = []
    for name, flags in (('plain', []), ('device', ['--device-decoder']),
                        ('pipe', ['--device-decoder', '--pipeline', '--decode-lockstep', '2'])):
        out = str(tmp_path / name)
        args = run.parse(['--input-glob', str(ori / 'frame_*.ply'), '--frames', '4', '--gop', '2', '--first-epoch', '1', '--others-epoch', '1',
                          '--seed', '8807', '--stream-chunk', '128', '--decode', '--out', out] + flags)
        assert args.device_decoder is bool(flags)
        summary, _ = run.run_sequence_job(args, files=run.resolve_files(args))
        assert summary['gops'] == 2 and summary['frames'] == 4 and summary['lossless'] is True
        outs.append(os.path.join(out, 'result_enc'))
    _same_files(outs[0], outs[1])
    _same_files(outs[0], outs[2])
    assert 'device_decoder' not in json.load(open(os.path.join(outs[1], 'gop_0_1', 'side_info.json')))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
    done = subprocess.run([sys.executable, '-m', 'linr_pcgc_amd.decoder', '--enc-dir', outs[1], '--dec-dir', str(tmp_path / 'dec'), '--ori-dir',
                           str(ori), '--device-decoder'], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    assert 'decoded 4 frames of 2 GOPs' in done.stdout and 'all equal to the input' in done.stdout
    side = json.load(open(os.path.join(outs[1], 'gop_0_1', 'side_info.json')))
    gen = lambda: LINR_PCGC_Model({'scale_num': int(side['scale_num']), 'in_channel': 7, 'hidden_channel_conv': 8, 'block_layers': 1,          # noqa: E731
                                   'outstage': 8, 'instage': 1}).cuda()
    seen = []
    real = decoder.codec.decode_gop

    def spy(*a, **kw):
        seen.append(kw.get('device_decoder', False))
        return real(*a, **kw)
    decoder.codec.decode_gop = spy
    try:
        for key in ({'device_decoder': True}, {}):
            decoder.decode({'gop_names': ['gop_0_1', 'gop_2_3'], 'Gen_Model': gen, 'result_enc_dir': outs[1],
                            'result_dec_dir': str(tmp_path / 'dec_dict'), 'dataset': cd.MytestDataset(str(ori), ori_type='ply'),
                            'write_flag': False, **key})
    finally:
        decoder.codec.decode_gop = real
    assert seen == [True, True, False, False]
