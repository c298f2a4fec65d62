"""GPU: self-checking streams (opt-in; stream_digests.py, include/linr_hip.h "geometry digests").  The digest kernels
(linr_coords_digest_segments) against the numpy restatement of the definition (tests/digest_ref.py), exact, between sentinel bytes;
GOPs encoded with digests=True through every decoder path; what a decoder says when a stored value, a stream byte or the files of
two frames are not what the encoder wrote; the drivers."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import digest_ref
from test_gpu_stream_chunks import _shell, _tree, _truth          # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 0xA5
PAD = 256                  # sentinel bytes in front of and behind the output and the workspace
BLOCK_ROWS = 256           # rows of one workgroup per pass (csrc/digest.hip: DG_BLOCK)
MAX_TILES = 256            # the cap of the grid: workgroups per segment (DG_MAX_TILES), so one pass of the grid is 65,536 rows
TOP = (1 << 20) - 1        # the largest coordinate the kernel map holds


# ---- the kernel --------------------------------------------------------------------------------------------------------------

def _rows(rng, n):
    rows = rng.integers(0, TOP + 1, size=(n, 3), dtype=np.int64).astype(np.int32)
    if n >= 2:
        rows[0] = (0, 0, 0)
        rows[n - 1] = (TOP, TOP, TOP)
    if n >= 5:
        rows[2] = (0, TOP, 0)
        rows[3] = rows[4]                                  # a duplicate: the digest is one of the multiset
    return rows


def _entry(coords, seg, origins, ws_bytes=None, shift=(0, 0, 0), null=()):
    """linr_coords_digest_segments itself on `coords` (a device int32 tensor), its output and workspace between PAD sentinel bytes.
    shift: bytes by which the coords / output / workspace pointers are moved off their alignment; null: the pointers passed as NULL.
    Returns (code, the n_seg digests as uint64, whether any sentinel byte changed, the output bytes)."""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    seg = None if seg is None else np.ascontiguousarray(seg, dtype=np.int64)
    n_seg = 1 if seg is None else len(seg) - 1
    n_out = max(n_seg, 1)
    need = L.linr_coords_digest_ws_bytes(n_seg) or 8
    given = need if ws_bytes is None else ws_bytes
    out = torch.full((PAD + 8 * n_out + PAD + 8,), SENT, dtype=torch.uint8, device='cuda')
    ws = torch.full((PAD + need + PAD + 8,), SENT, dtype=torch.uint8, device='cuda')
    assert out.data_ptr() % 256 == 0 and ws.data_ptr() % 256 == 0
    org = None if origins is None else np.ascontiguousarray(origins, dtype=np.int32)
    ptr = lambda name, p: None if name in null else p                                           # noqa: E731
    rc = L.linr_coords_digest_segments(ptr('coords', (coords.data_ptr() + shift[0]) if coords.numel() else None),
                                       ptr('seg', None if seg is None else seg.ctypes.data), n_seg, None if org is None else org.ctypes.data,
                                       ptr('out', out.data_ptr() + PAD + shift[1]), ptr('ws', ws.data_ptr() + PAD + shift[2]), given,
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o, w = out.cpu().numpy(), ws.cpu().numpy()
    pads_hit = bool((o[:PAD] != SENT).any() or (o[PAD + 8 * n_out:] != SENT).any() or (w[:PAD] != SENT).any() or (w[PAD + need:] != SENT).any())
    return rc, o[PAD:PAD + 8 * n_out].copy().view(np.uint64)[:n_seg], pads_hit, (o, w)


SINGLE = (0, 1, 63, 64, 65, BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1, 300007)


@pytest.mark.parametrize('n', SINGLE)
def test_one_segment_equals_the_reference(pkg, n):
    """300007 rows are more than one pass of the capped grid (MAX_TILES workgroups of BLOCK_ROWS rows = 65,536 rows per pass)."""
    from linr_pcgc_amd import _lib, ops
    assert SINGLE[-1] > 4 * MAX_TILES * BLOCK_ROWS
    rows = _rows(np.random.default_rng(n), n)
    dev = torch.from_numpy(rows).cuda()
    for origin in (None, (10, -20, 30), (-TOP, 5, -1)):
        want = digest_ref.digest(rows, origin)
        rc, got, pads_hit, _ = _entry(dev, [0, n], None if origin is None else [origin])
        assert rc == 0 and not pads_hit
        assert int(got[0]) == want, (n, origin, hex(int(got[0])), hex(want))
        host = _lib.lib().linr_coords_digest_host(rows.ctypes.data if n else None, n,
                                                  None if origin is None else np.asarray(origin, dtype=np.int32).ctypes.data)
        assert int(host) == want                                     # the host twin on the same rows
        t = ops.coords_digest(dev, origins=None if origin is None else [origin])
        assert t.dtype == torch.int64 and t.shape == (1,) and int(t.cpu().numpy().view(np.uint64)[0]) == want
    if n == 0:
        assert digest_ref.digest(rows) == digest_ref.KNOWN[0][2]


def _many_segments():
    cycle = (0, 1, 63, 64, 65, 1000)
    lens = [cycle[j % 6] for j in range(64)]
    lens[0] = lens[63] = 0
    lead = 1                                               # rows in front of the first segment that belong to none
    seg = np.concatenate([[lead], lead + np.cumsum(lens)]).astype(np.int64)
    return lens, seg


def test_64_segments_equal_the_reference(pkg):
    from linr_pcgc_amd import _lib, ops
    lens, seg = _many_segments()
    assert lens[0] == 0 and lens[-1] == 0 and set(lens) == {0, 1, 63, 64, 65, 1000}
    assert all(int(b) % 64 for b in seg), 'a boundary on a multiple of 64'
    total = int(seg[-1]) + 7                               # ... and rows behind the last one
    rng = np.random.default_rng(64)
    rows = _rows(rng, total)
    origins = rng.integers(-TOP, TOP + 1, size=(64, 3)).astype(np.int32)
    origins[1] = (-1, -TOP, 0)
    origins[2] = (0, 0, 0)
    assert (origins < 0).any()
    dev = torch.from_numpy(rows).cuda()
    for org in (origins, None):
        want = digest_ref.digest_segments(rows, seg, org)
        rc, got, pads_hit, _ = _entry(dev, seg, org)
        assert rc == 0 and not pads_hit
        assert [int(g) for g in got] == want
        assert ops.coords_digest(dev, seg, org).cpu().numpy().view(np.uint64).tolist() == want
    empty = digest_ref.KNOWN[0][2]
    assert want[0] == empty and want[63] == empty
    L = _lib.lib()
    for j in (1, 2, 5, 11):                                 # the host twin, segment by segment
        part = np.ascontiguousarray(rows[int(seg[j]):int(seg[j + 1])])
        assert int(L.linr_coords_digest_host(part.ctypes.data, part.shape[0], origins[j].ctypes.data)) == \
            digest_ref.digest(part, origins[j])
    # into a caller's buffer: nothing but its n_seg words
    buf = torch.full((66,), -7, dtype=torch.int64, device='cuda')
    ops.coords_digest(dev, seg, None, out=buf[1:65])
    got = buf.cpu().numpy()
    assert got[0] == -7 and got[65] == -7 and got[1:65].view(np.uint64).tolist() == want


def test_refusals_write_nothing(pkg):
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    EINVAL, ENOSPC, EALIGN = -1, -2, -3
    rows = _rows(np.random.default_rng(3), 700)
    dev = torch.from_numpy(rows).cuda()
    good = [0, 100, 100, 700]
    need = L.linr_coords_digest_ws_bytes(3)
    assert need > 0 and L.linr_coords_digest_ws_bytes(0) == 0 and L.linr_coords_digest_ws_bytes(65) == 0 and L.linr_coords_digest_ws_bytes(64) > 0
    cases = [
        (EINVAL, dict(seg=good, null=('coords',))), (EINVAL, dict(seg=good, null=('seg',))), (EINVAL, dict(seg=good, null=('out',))),
        (EINVAL, dict(seg=good, null=('ws',))),
        (EINVAL, dict(seg=[0], ws_bytes=need)),                                     # n_seg = 0
        (EINVAL, dict(seg=list(range(66)), ws_bytes=1 << 20)),                      # n_seg = 65
        (EINVAL, dict(seg=[-1, 100, 700])), (EINVAL, dict(seg=[0, 300, 299, 700])),
        (EALIGN, dict(seg=good, shift=(2, 0, 0))), (EALIGN, dict(seg=good, shift=(0, 4, 0))), (EALIGN, dict(seg=good, shift=(0, 0, 4))),
        (ENOSPC, dict(seg=good, ws_bytes=need - 1)), (ENOSPC, dict(seg=good, ws_bytes=0)),
    ]
    for code, kw in cases:
        rc, _, _, (o, w) = _entry(dev, kw.pop('seg'), None, **kw)
        assert rc == code, (code, kw, rc)
        assert bool((o == SENT).all()) and bool((w == SENT).all()), (code, kw)
    # the order of the checks: a bad table in front of a bad alignment in front of a short workspace
    assert _entry(dev, [0, 300, 299, 700], None, ws_bytes=0, shift=(2, 0, 0))[0] == EINVAL
    assert _entry(dev, good, None, ws_bytes=0, shift=(0, 4, 0))[0] == EALIGN
    rc, got, pads_hit, _ = _entry(dev, good, None)                                   # ... and the good call
    assert rc == 0 and not pads_hit and [int(g) for g in got] == digest_ref.digest_segments(rows, good)
    rc, got, pads_hit, _ = _entry(dev[:0], [0, 0, 0], None)                          # no rows at all: coords may be NULL
    assert rc == 0 and not pads_hit and [int(g) for g in got] == [digest_ref.KNOWN[0][2]] * 2


# ---- round trips ---------------------------------------------------------------------------------------------------------------

ENCODES = {'f32': {}, 'chunk64': {'stream_chunk': 64}, 'bf16': {'precision': 'bf16'}, 'wide16': {}}
DECODES = [('f32', {}), ('f32', {'workers': 2}), ('f32', {'lockstep': 3}), ('f32', {'device_decoder': True}), ('chunk64', {}),
           ('bf16', {}), ('wide16', {})]


@pytest.fixture(scope='module')
def gops(pkg):
    """Three sphere shells (6 bit, r = 18, 20, 22), untrained models of seed 8807, and per encoder setting the GOP without and with
    digests, each computed once."""
    from linr_pcgc_amd import codec, overfit, synthetic
    gop = overfit.Gop(None, [synthetic.sphere_shell(6, r) for r in (18, 20, 22)], None, 64, 'cuda')
    out = {}
    for name, kw in ENCODES.items():
        hidden = 16 if name == 'wide16' else 8
        model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807, hidden=hidden)
        out[name] = (codec.encode_gop(model, _shell(gop, hidden), gop, 8, **kw),
                     codec.encode_gop(model, _shell(gop, hidden), gop, 8, digests=True, **kw), hidden)
    return gop, out


def _write(enc, path):
    from linr_pcgc_amd import codec
    codec.write_gop(enc, str(path))
    return str(path)


def test_digests_change_nothing_else(gops, tmp_path):
    from linr_pcgc_amd import codec, stream_digests
    gop, encs = gops
    assert all(len(info['all_input_info']) >= 2 for info in gop.infos)
    for name, (plain, dig, _) in encs.items():
        a, b = _write(plain, tmp_path / (name + '_plain')), _write(dig, tmp_path / (name + '_dig'))
        assert [n for n in _tree(b) if n not in _tree(a)] == [os.path.join('bins', 'digests.bin')] and set(_tree(a)) < set(_tree(b))
        for n in _tree(a):
            if n != 'side_info.json':
                assert open(os.path.join(a, n), 'rb').read() == open(os.path.join(b, n), 'rb').read(), n
        sa, sb = json.load(open(os.path.join(a, 'side_info.json'))), json.load(open(os.path.join(b, 'side_info.json')))
        assert sb == {**sa, 'digests': 1} and 'digests' not in sa
        back, back_plain = codec.read_gop(b), codec.read_gop(a)
        assert back_plain['digests_bin'] is None and 'digests_bin' not in plain and 'digest_bits' not in plain
        assert back['digests_bin'] == dig['digests_bin'] == open(os.path.join(b, 'bins', 'digests.bin'), 'rb').read()
        assert {k: v for k, v in back.items() if k != 'digests_bin'} == {k: dig[k] for k in ('frames', 'model_bin', 'low_enc_bytes', 'side_info')}
        # the rate: 8 * len(digests.bin) + 8 bits more, with the model
        points = plain['point_num']
        extra = 8 * len(dig['digests_bin']) + 8
        assert dig['digest_bits'] == extra == stream_digests.bits(dig['digests_bin'])
        assert len(dig['digests_bin']) == 4 * sum(len(f) for f in dig['frames'])
        for key in ('bpp_all', 'model_bpp'):
            total = round(plain['bpp'][key] * points)
            assert total / points == plain['bpp'][key]
            assert dig['bpp'][key] == (total + extra) / points, key
        assert dig['bpp']['point_bpp'] == plain['bpp']['point_bpp'] and dig['bpp']['xyzlow_bpp'] == plain['bpp']['xyzlow_bpp']
        assert dig['bits_est'] == plain['bits_est']


def test_stored_values_are_the_reference_digests_of_the_staged_levels(gops):
    from linr_pcgc_amd import stream_digests
    gop, encs = gops
    want = []
    for info, cmin in zip(gop.infos, gop.coord_mins):
        levels = [sc['ground_truth'].cpu().numpy() for sc in info['all_input_info']]
        want.append([digest_ref.digest(lv, cmin if s == 0 else None) >> 32 for s, lv in enumerate(levels)])
        assert digest_ref.digest(levels[0], cmin) == digest_ref.digest(_truth(gop, len(want) - 1).cpu().numpy())     # the decoder's output
    for name, (_, dig, _) in encs.items():
        assert stream_digests.unpack(dig['digests_bin'], [len(f) for f in dig['frames']]) == want, name


@pytest.mark.parametrize('name,kw', DECODES, ids=['%s-%s' % (n, '-'.join('%s%s' % kv for kv in k.items()) or 'plain') for n, k in DECODES])
def test_round_trip(gops, tmp_path, name, kw):
    """encode_gop(digests=True) -> write_gop -> read_gop -> decode_gop gives the frames, as the run without digests does; verify=False
    decodes the same frames."""
    from linr_pcgc_amd import codec
    gop, encs = gops
    plain, dig, hidden = encs[name]
    enc = codec.read_gop(_write(dig, tmp_path / 'enc'))
    assert enc['digests_bin'] is not None
    seen = []
    real = codec.verify_levels

    def spy(levels, wants, frame_ids, scale, origins=None):
        seen.append((tuple(frame_ids), scale, origins is not None))
        return real(levels, wants, frame_ids, scale, origins)
    codec.verify_levels = spy
    try:
        dec = codec.decode_gop(_shell(gop, hidden), enc, 'cuda', **kw)
        n_checks = len(seen)
        off = codec.decode_gop(_shell(gop, hidden), enc, 'cuda', verify=False, **kw)
        old = codec.decode_gop(_shell(gop, hidden), plain, 'cuda', **kw)               # a GOP without digests decodes as before
        assert len(seen) == n_checks                                                   # ... and nothing new runs for either
    finally:
        codec.verify_levels = real
    n_scales = [len(f) for f in enc['frames']]
    if 'lockstep' in kw:
        assert sorted(seen) == sorted(((0, 1, 2), s, s == 0) for s in range(n_scales[0]))
    else:
        assert sorted(seen) == sorted(((i,), s, s == 0) for i in range(3) for s in range(n_scales[i]))
    for i in range(3):
        assert torch.equal(dec[i], _truth(gop, i)) and torch.equal(off[i], dec[i]) and torch.equal(old[i], dec[i])


# ---- detection -----------------------------------------------------------------------------------------------------------------

PATHS = [{}, {'workers': 2}, {'lockstep': 3}, {'device_decoder': True}]


def _flip(path, offset, mask=0xFF):
    data = bytearray(open(path, 'rb').read())
    data[offset] ^= mask
    with open(path, 'wb') as f:
        f.write(bytes(data))


def test_an_altered_stored_value_is_reported(gops, tmp_path):
    from linr_pcgc_amd import _lib, codec
    gop, encs = gops
    root = _write(encs['f32'][1], tmp_path / 'enc')
    n0 = len(encs['f32'][1]['frames'][0])
    _flip(os.path.join(root, 'bins', 'digests.bin'), 4 * (n0 + 1) + 2, 0x10)                 # (frame 1, scale 1)
    enc = codec.read_gop(root)
    for kw in PATHS:
        with pytest.raises(_lib.LinrDigestError) as e:
            codec.decode_gop(_shell(gop), enc, 'cuda', **kw)
        assert (e.value.frame, e.value.scale) == (1, 1) and e.value.want != e.value.got and e.value.want ^ e.value.got == 0x100000, kw
        assert 'frame 1' in str(e.value) and 'scale 1' in str(e.value)
    dec = codec.decode_gop(_shell(gop), enc, 'cuda', frames=[0, 2])                          # the other frames are fine
    assert torch.equal(dec[0], _truth(gop, 0)) and torch.equal(dec[1], _truth(gop, 2))
    dec = codec.decode_gop(_shell(gop), enc, 'cuda', verify=False)                           # ... and so are the streams
    assert all(torch.equal(dec[i], _truth(gop, i)) for i in range(3))


def test_a_damaged_stream_is_reported_at_its_scale(gops, tmp_path):
    """The first payload byte of stage 0's stream of (frame 1, scale 1) XOR 0xFF: the range decoder is defined on any bytes and decodes
    other symbols; the error names that scale, not a later one, and is no other exception."""
    from linr_pcgc_amd import _lib, codec
    from linr_pcgc_amd.function_utils import pack_bitstream, unpack_bitstream
    gop, encs = gops
    root = _write(encs['f32'][1], tmp_path / 'enc')
    path = os.path.join(root, 'bins', 'frame0001_scale1.bin')
    streams = unpack_bitstream(open(path, 'rb').read())
    assert len(streams) == 8 and len(streams[0]) > 0
    with open(path, 'wb') as f:
        f.write(pack_bitstream([bytes([streams[0][0] ^ 0xFF]) + streams[0][1:]] + streams[1:]))
    enc = codec.read_gop(root)
    for kw in PATHS:
        with pytest.raises(_lib.LinrDigestError) as e:
            codec.decode_gop(_shell(gop), enc, 'cuda', **kw)
        assert (e.value.frame, e.value.scale) == (1, 1) and e.value.want != e.value.got, kw


def test_swapped_frames_are_reported(gops, tmp_path):
    from linr_pcgc_amd import _lib, codec
    gop, encs = gops
    root = _write(encs['f32'][1], tmp_path / 'enc')
    bins = os.path.join(root, 'bins')
    names0 = sorted(n for n in os.listdir(bins) if n.startswith('frame0000_'))
    names2 = sorted(n for n in os.listdir(bins) if n.startswith('frame0002_'))
    assert len(names0) == len(names2) >= 2
    for a, b in zip(names0, names2):
        os.rename(os.path.join(bins, a), os.path.join(bins, 'tmp'))
        os.rename(os.path.join(bins, b), os.path.join(bins, a))
        os.rename(os.path.join(bins, 'tmp'), os.path.join(bins, b))
    enc = codec.read_gop(root)
    with pytest.raises(_lib.LinrDigestError) as e:
        codec.decode_gop(_shell(gop), enc, 'cuda')
    assert e.value.frame == 0
    with pytest.raises(_lib.LinrDigestError) as e:
        codec.decode_gop(_shell(gop), enc, 'cuda', lockstep=3)
    assert e.value.frame == 0


def test_a_short_digests_file_is_refused_before_any_launch(gops, tmp_path):
    from linr_pcgc_amd import _lib, codec, ops
    gop, encs = gops
    enc = dict(encs['f32'][1])
    enc['digests_bin'] = enc['digests_bin'][:-1]
    launched = []
    real_scale, real_digest = codec.Model_Estimate.decompress_model, ops.coords_digest
    codec.Model_Estimate.decompress_model = lambda *a, **k: launched.append('model') or real_scale(*a, **k)
    ops.coords_digest = lambda *a, **k: launched.append('digest') or real_digest(*a, **k)
    try:
        for kw in PATHS:
            with pytest.raises(_lib.LinrError, match='digests.bin has %d bytes' % len(enc['digests_bin'])) as e:
                codec.decode_gop(_shell(gop), enc, 'cuda', **kw)
            assert not isinstance(e.value, _lib.LinrDigestError)
        assert launched == []
        assert len(codec.decode_gop(_shell(gop), enc, 'cuda', verify=False)) == 3
        assert launched == ['model']
        newer = dict(encs['f32'][1], side_info={**encs['f32'][1]['side_info'], 'digests': 2})
        with pytest.raises(_lib.LinrError, match='written by a newer build'):
            codec.decode_gop(_shell(gop), newer, 'cuda')
    finally:
        codec.Model_Estimate.decompress_model, ops.coords_digest = real_scale, real_digest


# ---- the drivers -------------------------------------------------------------------------------------------------------------

def test_drivers_carry_the_option(pkg, golden_dir, tmp_path):
    """run.py --digests --decode on two GOPs of two frames, alone and with --pipeline: lossless, the same files, and apart from
    digests.bin and the one key those of the run without the flag; python -m linr_pcgc_amd.decoder without --ori-dir says that it
    verified them and, after one stored value was altered, exits non-zero naming GOP, frame and scale; decoder.decode honours 'verify'."""
    from linr_pcgc_amd import _lib, custom_dataset as cd, decoder, run
    from linr_pcgc_amd.model_core import LINR_PCGC_Model
    pts = np.unique(np.load(os.path.join(golden_dir, 'octree_shell128.npz'))['points'], axis=0)
    ori = tmp_path / 'ori'
    ori.mkdir()
    for t in range(4):
        cd.write_ply_ascii(str(ori / ('frame_%04d.ply' % t)), pts + t)
    outs = []
    for name, flags in (('plain', []), ('digests', ['--digests']), ('pipe', ['--digests', '--pipeline'])):
        out = str(tmp_path / name)
        args = run.parse(['--input-glob', str(ori / 'frame_*.ply'), '--frames', '4', '--gop', '2', '--first-epoch', '1', '--others-epoch', '1',
                          '--seed', '8807', '--decode', '--out', out] + flags)
        assert args.digests is bool(flags)
        summary, _ = run.run_sequence_job(args, files=run.resolve_files(args))
        assert summary['gops'] == 2 and summary['frames'] == 4 and summary['lossless'] is True
        outs.append(os.path.join(out, 'result_enc'))
    names = _tree(outs[1])
    assert names == _tree(outs[2]) and len(names) > 3
    for n in names:
        assert open(os.path.join(outs[1], n), 'rb').read() == open(os.path.join(outs[2], n), 'rb').read(), n
    assert [n for n in names if n not in _tree(outs[0])] == [os.path.join(g, 'bins', 'digests.bin') for g in ('gop_0_1', 'gop_2_3')]
    for n in _tree(outs[0]):
        if not n.endswith('side_info.json'):
            assert open(os.path.join(outs[0], n), 'rb').read() == open(os.path.join(outs[1], n), 'rb').read(), n
    side = json.load(open(os.path.join(outs[1], 'gop_0_1', 'side_info.json')))
    assert side == {**json.load(open(os.path.join(outs[0], 'gop_0_1', 'side_info.json'))), 'digests': 1}

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))

    def program(enc_dir, dec_dir, *flags):
        return subprocess.run([sys.executable, '-m', 'linr_pcgc_amd.decoder', '--enc-dir', enc_dir, '--dec-dir', str(tmp_path / dec_dir), *flags],
                              cwd=root, env=env, capture_output=True, text=True, timeout=600)
    done = program(outs[1], 'dec')
    assert done.returncode == 0, done.stderr[-2000:]
    assert 'decoded 4 frames of 2 GOPs' in done.stdout and "verified against the stream's digests" in done.stdout
    bad = str(tmp_path / 'bad')
    shutil.copytree(outs[1], bad)
    n0 = len([n for n in os.listdir(os.path.join(bad, 'gop_2_3', 'bins')) if n.startswith('frame0000_')])
    _flip(os.path.join(bad, 'gop_2_3', 'bins', 'digests.bin'), 4 * (n0 + 1))                  # (frame 1, scale 1) of the second GOP
    done = program(bad, 'dec_bad')
    assert done.returncode != 0
    assert 'gop_2_3' in done.stderr and 'frame 1' in done.stderr and 'scale 1' in done.stderr and 'verified' not in done.stdout
    done = program(bad, 'dec_off', '--no-verify')
    assert done.returncode == 0 and 'decoded 4 frames of 2 GOPs' in done.stdout and 'verified' not in done.stdout

    gen = lambda: LINR_PCGC_Model({'scale_num': int(side['scale_num']), 'in_channel': 7, 'hidden_channel_conv': 8, 'block_layers': 1,          # noqa: E731
                                   'outstage': 8, 'instage': 1}).cuda()
    inargs = {'gop_names': ['gop_0_1', 'gop_2_3'], 'Gen_Model': gen, 'result_enc_dir': bad, 'result_dec_dir': str(tmp_path / 'dec_dict'),
              'dataset': cd.MytestDataset(str(ori), ori_type='ply'), 'write_flag': False}
    with pytest.raises(_lib.LinrDigestError) as e:
        decoder.decode(inargs)
    assert (e.value.frame, e.value.scale) == (1, 1)
    decoder.decode({**inargs, 'verify': False})
    decoder.decode({**inargs, 'result_enc_dir': outs[1]})
