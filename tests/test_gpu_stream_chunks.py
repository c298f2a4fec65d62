"""GPU: chunked stage streams (opt-in; side_info.json's stream_chunk = S; linr_pcgc_amd/stream_chunks.py has the format).  The device
coder's chunked entry (linr_rc_encode_codes_chunked, csrc/ac_device.hip: a wave per chunk) against the host coder's chunks joined, the
decoder's chunked scale entries (csrc/decode.hip) through codec.decode_gop, and the paths that carry S: codec.encode_gop, run.py
--stream-chunk, encoder.encode.  S = 64 and 128 on the suite's small shells: a few thousand rows give hundreds of chunks with ragged
tails.  Bytes, lengths, offsets and decoded geometry, all exact; no rate and no time is asserted."""
import filecmp
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_device_coder_host import REGIMES, draw, pack_symbols      # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SIZES = (64, 128)


# ---- the entry -----------------------------------------------------------------------------------------------------------------

def stream_lengths(S):
    """n < S, n = S and n = S + 1 among them, an empty stream, tails of every kind, and two long streams: over 200 chunks together."""
    return [S - 1, S, S + 1, 0, 1, 2 * S, 2 * S + 1, 5 * S + 17, 31, 70 * S + 33, S // 2, 140 * S - 1, 3 * S]


@pytest.fixture(scope='module')
def mixed(pkg):
    """Per S: streams of stream_lengths(S), the coder regimes of the host test in turn, laid out in shared c1 / sym buffers behind a
    non-zero lead (c1 offsets odd and even, every stream's words behind those of the one before it), and the host coder's chunked
    streams (encode_streams_codes(chunk=S), which tests/test_stream_chunks_host.py pins to the unchunked coder), computed once."""
    from linr_pcgc_amd.model_core import encode_streams_codes
    out = {}
    for S in SIZES:
        items = [draw(REGIMES[r % len(REGIMES)], n, 17 * S + r) for r, n in enumerate(stream_lengths(S))]
        c1_all, w_all, desc = [np.full(7, 12345, dtype=np.uint16)], [np.full(3, 0xDEADBEEF, dtype=np.uint32)], []
        cb, wb = 7, 3
        for c1, s in items:
            w = pack_symbols(s)
            desc.append((cb, wb, len(c1)))
            c1_all.append(c1)
            w_all.append(w)
            cb, wb = cb + len(c1), wb + len(w)
        ns = [len(c1) for c1, _ in items]
        want = encode_streams_codes([c1 for c1, _ in items], [pack_symbols(s) for _, s in items], ns, 4, S)
        plain = encode_streams_codes([c1 for c1, _ in items], [pack_symbols(s) for _, s in items], ns, 4)
        out[S] = {'c1': torch.from_numpy(np.concatenate(c1_all)).cuda(), 'sym': torch.from_numpy(np.concatenate(w_all)).cuda(),
                  'desc': np.asarray(desc, dtype=np.int64), 'want': want, 'plain': plain}
    return out


class Call:
    """Buffers of one linr_rc_encode_codes_chunked call, all filled with the sentinel."""

    def __init__(self, m, S, tab=None, gap=4):
        from linr_pcgc_amd import _lib
        from linr_pcgc_amd.model_core import DeviceCoderSet
        self.L = _lib.lib()
        self.m, self.S = m, S
        if tab is None:
            tab = DeviceCoderSet.table(m['desc'], S)[0]
            size = ((tab[:, 4] + 3) & ~3) + gap                      # a gap between the regions that nothing may touch
            tab[:, 3] = np.cumsum(size) - size
        self.tab = np.ascontiguousarray(tab, dtype=np.int64)
        self.n = len(self.tab)
        self.chunks = DeviceCoderSet.chunks(self.tab[:, :3], S) if S else self.n
        self.out_bytes = int((self.tab[:, 3] + self.tab[:, 4]).max())
        self.payload_bytes = int(self.tab[:, 4].sum()) + 5 * (self.chunks - self.n)
        fill = lambda nbytes: torch.from_numpy(np.full(nbytes, SENTINEL, dtype=np.uint8)).cuda()          # noqa: E731
        self.out, self.payload = fill(self.out_bytes + 64), fill(self.payload_bytes + 64)
        self.len, self.offsets = fill(8 * (self.n + 1)).view(torch.int64), fill(8 * (self.n + 2)).view(torch.int64)
        self.ws_bytes = int(self.L.linr_rc_encode_chunked_ws_bytes(self.n, self.chunks) if S else
                            self.L.linr_rc_encode_ws_bytes(self.n, int(self.tab[:, 4].sum())))
        self.ws = _lib.scratch(self.ws_bytes + 64, 'cuda')

    def run(self, entry='chunked'):
        st = torch.cuda.current_stream().cuda_stream
        head = (self.m['c1'].data_ptr(), self.m['sym'].data_ptr(), self.tab.ctypes.data, self.n)
        tail = (self.out.data_ptr(), self.out_bytes, self.len.data_ptr(), self.payload.data_ptr(), self.payload_bytes,
                self.offsets.data_ptr(), self.ws.data_ptr(), self.ws_bytes, st)
        rc = self.L.linr_rc_encode_codes_chunked(*head, self.S, *tail) if entry == 'chunked' else self.L.linr_rc_encode_codes(*head, *tail)
        torch.cuda.synchronize()
        return rc

    def check(self, want, nospc=()):
        n = self.n
        lens, offs = self.len.cpu().numpy(), self.offsets.cpu().numpy()
        out, payload = self.out.cpu().numpy(), self.payload.cpu().numpy()
        assert lens[:n].tolist() == [-2 if i in nospc else len(want[i]) for i in range(n)]
        assert offs[:n + 1].tolist() == np.concatenate([[0], np.cumsum([0 if i in nospc else len(want[i]) for i in range(n)])]).tolist()
        for i in range(n):
            if i not in nospc:
                assert payload[offs[i]:offs[i + 1]].tobytes() == want[i], i
        covered = np.zeros(out.size, dtype=bool)
        for o, cap in self.tab[:, 3:5]:
            covered[o:o + cap] = True
        assert (out[~covered] == SENTINEL).all(), 'a byte outside every stream\'s region was written'
        assert (payload[offs[n]:] == SENTINEL).all()
        sent = np.frombuffer(bytes([SENTINEL]) * 8, dtype=np.int64)[0]
        assert lens[n] == sent and offs[n + 1] == sent


@pytest.mark.parametrize('S', SIZES)
def test_chunked_entry_gives_the_host_coders_chunked_streams(mixed, S):
    from linr_pcgc_amd.model_core import DeviceCoderSet
    from linr_pcgc_amd.stream_chunks import chunk_count
    m = mixed[S]
    ks = [chunk_count(int(n), S) for n in m['desc'][:, 2]]
    assert sum(ks) >= 200 and ks[:3] == [1, 1, 2] and DeviceCoderSet.chunks(m['desc'], S) == sum(ks)
    assert [a != b for a, b, k in zip(m['want'], m['plain'], ks)] == [k > 1 for k in ks]
    call = Call(m, S)
    assert call.run() == 0
    call.check(m['want'])
    first = (call.len.cpu(), call.offsets.cpu(), call.out.cpu(), call.payload.cpu())
    assert call.run() == 0                                  # a second call into the same buffers gives the same result
    for a, b in zip(first, (call.len.cpu(), call.offsets.cpu(), call.out.cpu(), call.payload.cpu())):
        assert torch.equal(a, b)


def test_chunk_symbols_zero_is_the_unchunked_entry(mixed):
    m = mixed[64]
    a, b = Call(m, 0), Call(m, 0)
    assert a.run('chunked') == 0 and b.run('plain') == 0
    a.check(m['plain'])
    for x, y in ((a.len, b.len), (a.offsets, b.offsets), (a.out, b.out), (a.payload, b.payload)):
        assert torch.equal(x, y)


def test_a_lone_chunk_without_space_is_enospc_and_the_others_are_exact(mixed):
    """A stream of one chunk keeps its own cap: one byte short and it is LINR_ENOSPC, counts 0 in the offsets, and every other
    stream - the chunked ones around it, too - is exact.  A chunked stream whose region is short of its chunks' regions is refused
    before anything is launched."""
    from linr_pcgc_amd.model_core import DeviceCoderSet
    S = 64
    m = mixed[S]
    tab = DeviceCoderSet.table(m['desc'], S)[0]
    lone = [i for i, n in enumerate(m['desc'][:, 2]) if n <= S and len(m['want'][i]) > 1]
    assert len(lone) >= 3
    tab[lone[0], 4] = len(m['want'][lone[0]]) - 1
    tab[lone[1], 4] = 0
    tab[lone[2], 4] = len(m['want'][lone[2]])              # exactly enough
    call = Call(m, S, tab)
    assert call.run() == 0
    call.check(m['want'], nospc=(lone[0], lone[1]))
    tab2 = DeviceCoderSet.table(m['desc'], S)[0]
    big = int(np.argmax(m['desc'][:, 2]))
    tab2[big, 4] -= 1
    call = Call(m, S, tab2)
    assert call.run() == -1
    assert bool((call.out == SENTINEL).all()) and bool((call.payload == SENTINEL).all())


def test_encode_streams_device_with_chunks(mixed):
    from linr_pcgc_amd import model_core
    for S in SIZES:
        assert model_core.encode_streams_device(mixed[S]['c1'], mixed[S]['sym'], mixed[S]['desc'], S) == mixed[S]['want']
    assert model_core.encode_streams_device(mixed[64]['c1'], mixed[64]['sym'], mixed[64]['desc']) == mixed[64]['plain']
    with pytest.raises(ValueError):
        model_core.encode_streams_device(mixed[64]['c1'], mixed[64]['sym'], mixed[64]['desc'], 100)


# ---- the codec path ----------------------------------------------------------------------------------------------------------

def _shell(gop, hidden=8):
    from linr_pcgc_amd import overfit
    return overfit.gen_model(gop.scale_num, 'cuda', hidden=hidden)


def _truth(gop, i):
    return torch.as_tensor(gop.infos[i]['ori']).cuda() + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32)


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _same_files(a, b):
    names = _tree(a)
    assert names == _tree(b) and len(names) > 3
    for n in names:
        assert filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False), n


@pytest.fixture(scope='module')
def shell_gop(pkg, golden_dir):
    """Three frames of the golden 128-cube shell, an untrained model of seed 8807, the plain GOP (fp32 and bf16) and the host coder's
    chunked GOPs, each computed once."""
    from linr_pcgc_amd import codec, overfit
    pts = np.load(os.path.join(golden_dir, 'octree_shell128.npz'))['points']
    gop = overfit.Gop(None, [pts, pts, pts], None, 64, 'cuda')
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807)
    plain = {prec: codec.encode_gop(model, _shell(gop), gop, 8, precision=prec) for prec in ('f32', 'bf16')}
    host = {(prec, S): codec.encode_gop(model, _shell(gop), gop, 8, precision=prec, stream_chunk=S) for prec in ('f32', 'bf16') for S in SIZES}
    return gop, model, plain, host


def test_chunked_gop_differs_where_it_should(shell_gop):
    from linr_pcgc_amd import codec
    from linr_pcgc_amd.function_utils import unpack_bitstream
    from linr_pcgc_amd.stream_chunks import chunk_count, split_chunks
    gop, model, plain, host = shell_gop
    f = gop.frames[0]
    ns = [int(f.row_off[i + 1] - f.row_off[i]) for i in range(f.n_scales)]
    assert any(n % 64 for n in ns) and max(ns) > 4 * 128 and min(ns) < 64
    for S in SIZES:
        enc, ref = host['f32', S], plain['f32']
        assert 8 * sum(chunk_count(n, S) for n in ns) >= 200
        assert enc['side_info'] == {**ref['side_info'], 'stream_chunk': S} and enc['model_bin'] == ref['model_bin']
        for i, n in enumerate(ns):
            got, want = unpack_bitstream(enc['frames'][0][i]), unpack_bitstream(ref['frames'][0][i])
            assert len(got) == 8
            if n <= S:
                assert got == want
            else:
                assert all(len(split_chunks(g, n, S)) == chunk_count(n, S) for g in got) and got != want
        points = enc['point_num']
        assert enc['bpp']['model_bpp'] * points == pytest.approx(ref['bpp']['model_bpp'] * points + 32, abs=1e-6)
        occ = lambda e: 8 * sum(len(b) for fb in e['frames'] for b in fb)                              # noqa: E731
        assert enc['bpp']['bpp_all'] * points == pytest.approx(ref['bpp']['bpp_all'] * points + 32 + occ(enc) - occ(ref), abs=1e-6)
    assert codec.EXTRA_SIDE_BITS == 40


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
@pytest.mark.parametrize('S', SIZES)
def test_chunked_gop_round_trip_is_lossless(shell_gop, tmp_path, precision, S):
    """encode_gop(stream_chunk=S) -> write_gop -> read_gop -> decode_gop: per frame with workers 1 and 2 and n_threads 1 and 4, and with
    lockstep=3; every frame is the input and what the plain GOP decodes to."""
    from linr_pcgc_amd import codec
    gop, model, plain, host = shell_gop
    codec.write_gop(host[precision, S], str(tmp_path / 'enc'))
    enc = codec.read_gop(str(tmp_path / 'enc'))
    assert enc['side_info']['stream_chunk'] == S and enc['frames'] == host[precision, S]['frames']
    ref = codec.decode_gop(_shell(gop), plain[precision], 'cuda')
    arms = [dict(workers=w, n_threads=t) for w in (1, 2) for t in (1, 4)] + [dict(lockstep=3, n_threads=4), dict()]
    for kw in arms:
        got = codec.decode_gop(_shell(gop), enc, 'cuda', **kw)
        assert len(got) == 3
        for i in range(3):
            assert torch.equal(got[i], ref[i]), (kw, i)
            assert torch.equal(got[i], _truth(gop, i)), (kw, i)


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
@pytest.mark.parametrize('group', [1, 3])
def test_the_three_coders_write_identical_files(shell_gop, tmp_path, precision, group):
    from linr_pcgc_amd import codec
    gop, model, plain, host = shell_gop
    for S in SIZES:
        ref = host[precision, S]
        codec.write_gop(ref, str(tmp_path / ('host%d' % S)))
        for name, kw in (('codes', {'device_codes': True}), ('coder', {'device_coder': True, 'coder_group': group})):
            enc = codec.encode_gop(model, _shell(gop), gop, 8, precision=precision, stream_chunk=S, **kw)
            assert enc['frames'] == ref['frames'], (S, name)
            assert enc['side_info'] == ref['side_info'] and enc['bpp'] == ref['bpp'] and enc['model_bin'] == ref['model_bin']
            codec.write_gop(enc, str(tmp_path / ('%s%d' % (name, S))))
            _same_files(str(tmp_path / ('host%d' % S)), str(tmp_path / ('%s%d' % (name, S))))


def test_zero_and_omitted_are_the_plain_gop(shell_gop, tmp_path):
    from linr_pcgc_amd import codec
    gop, model, plain, _ = shell_gop
    codec.write_gop(plain['f32'], str(tmp_path / 'omitted'))
    for kw in ({}, {'device_codes': True}, {'device_coder': True, 'coder_group': 3}):
        enc = codec.encode_gop(model, _shell(gop), gop, 8, stream_chunk=0, **kw)
        assert 'stream_chunk' not in enc['side_info'] and enc['bpp'] == plain['f32']['bpp']
        codec.write_gop(enc, str(tmp_path / 'zero'))
        _same_files(str(tmp_path / 'omitted'), str(tmp_path / 'zero'))
    assert 'stream_chunk' not in json.load(open(str(tmp_path / 'zero' / 'side_info.json')))


def test_a_chunk_size_at_or_above_the_longest_stream_changes_only_the_field(shell_gop):
    from linr_pcgc_amd import codec
    gop, model, plain, _ = shell_gop
    longest = max(int(f.row_off[i + 1] - f.row_off[i]) for f in gop.frames for i in range(f.n_scales))
    at = (longest + 63) // 64 * 64                         # the smallest valid S that holds the longest stream
    for S, kw in ((at, {}), (at, {'device_coder': True, 'coder_group': 3}), (1 << 24, {'device_codes': True})):
        enc = codec.encode_gop(model, _shell(gop), gop, 8, stream_chunk=S, **kw)
        assert enc['frames'] == plain['f32']['frames'] and enc['model_bin'] == plain['f32']['model_bin']
        assert enc['side_info'] == {**plain['f32']['side_info'], 'stream_chunk': S}
        if not kw:
            dec = codec.decode_gop(_shell(gop), enc, 'cuda', workers=2)
            assert all(torch.equal(d, _truth(gop, i)) for i, d in enumerate(dec))
    if at - 64 >= 64:                                      # one step below it the longest stream is cut
        assert codec.encode_gop(model, _shell(gop), gop, 8, stream_chunk=at - 64)['frames'] != plain['f32']['frames']


def test_bad_chunk_sizes_and_wide_models_are_refused(shell_gop):
    from linr_pcgc_amd import codec, overfit, synthetic
    gop, model, _, _ = shell_gop
    for bad in (32, 100, -64, (1 << 24) + 64):
        with pytest.raises(ValueError):
            codec.encode_gop(model, _shell(gop), gop, 8, stream_chunk=bad)
    small = overfit.Gop(None, [synthetic.sphere_shell(6, 20)], None, 64, 'cuda')
    wide = overfit.gen_model(small.scale_num, 'cuda', seed=8807, hidden=16)
    with pytest.raises(ValueError, match='hidden_channel_conv'):
        codec.encode_gop(wide, _shell(small, 16), small, 8, stream_chunk=64)
    # ... and a chunked GOP handed to a wide decoder is refused, not decoded stage-wise as if it were plain
    enc = codec.encode_gop(wide, _shell(small, 16), small, 8)
    enc['side_info'] = {**enc['side_info'], 'stream_chunk': 64}
    with pytest.raises(ValueError):
        codec.decode_gop(_shell(small, 16), enc, 'cuda')


def test_a_corrupted_chunk_header_on_disk_is_refused(shell_gop, tmp_path):
    """The first length of stage 0's stream of the finest scale of frame 1 rewritten on disk - as an unterminated varint, and as a
    length past the end of the stream: decode_gop raises LinrError (the parser's refusal, in front of the scale's first launch), per
    frame and in lock step; the untouched files decode."""
    from linr_pcgc_amd import _lib, codec
    from linr_pcgc_amd.function_utils import pack_bitstream, unpack_bitstream
    from linr_pcgc_amd.stream_chunks import leb128
    gop, model, _, host = shell_gop
    S = 64
    root = str(tmp_path / 'enc')
    codec.write_gop(host['f32', S], root)
    path = os.path.join(root, 'bins', 'frame0001_scale0.bin')
    good = open(path, 'rb').read()
    streams = unpack_bitstream(good)
    assert int(gop.frames[1].row_off[1] - gop.frames[1].row_off[0]) > S
    for what, head in (('unterminated', b'\xff' * 5), ('past the end', leb128(len(streams[0]) + 1))):
        first = 0
        while streams[0][first] & 0x80:
            first += 1
        with open(path, 'wb') as f:
            f.write(pack_bitstream([head + streams[0][first + 1:]] + streams[1:]))
        enc = codec.read_gop(root)
        for kw in ({}, {'workers': 2, 'n_threads': 4}, {'lockstep': 3}):
            with pytest.raises(_lib.LinrError, match='LINR_EINVAL'):
                codec.decode_gop(_shell(gop), enc, 'cuda', **kw)
        assert len(codec.decode_gop(_shell(gop), enc, 'cuda', frames=[0, 2])) == 2          # the other frames are fine
    with open(path, 'wb') as f:
        f.write(good)
    dec = codec.decode_gop(_shell(gop), codec.read_gop(root), 'cuda')
    assert all(torch.equal(d, _truth(gop, i)) for i, d in enumerate(dec))


# ---- the drivers -------------------------------------------------------------------------------------------------------------

def test_run_stream_chunk_decode_with_and_without_pipeline(pkg, golden_dir, tmp_path):
    """run.py --stream-chunk 128 --decode on two GOPs of two frames: lossless, the same files with --pipeline, stream_chunk in every
    side_info.json, and python -m linr_pcgc_amd.decoder in another process rebuilds every frame from the files alone."""
    from linr_pcgc_amd import custom_dataset as cd, run
    pts = np.load(os.path.join(golden_dir, 'octree_shell128.npz'))['points']
    ori = tmp_path / 'ori'
    ori.mkdir()
    for t in range(4):
        cd.write_ply_ascii(str(ori / ('frame_%04d.ply' % t)), pts + t)
    outs = []
    for flags in ([], ['--pipeline']):
        out = str(tmp_path / ('pipe' if flags else 'plain'))
        args = run.parse(['--input-glob', str(ori / 'frame_*.ply'), '--frames', '4', '--gop', '2', '--first-epoch', '1', '--others-epoch', '1',
                          '--seed', '8807', '--stream-chunk', '128', '--decode', '--out', out] + flags)
        assert args.stream_chunk == 128
        summary, _ = run.run_sequence_job(args, files=run.resolve_files(args))
        assert summary['gops'] == 2 and summary['frames'] == 4 and summary['lossless'] is True
        outs.append(os.path.join(out, 'result_enc'))
    _same_files(outs[0], outs[1])
    for g in ('gop_0_1', 'gop_2_3'):
        assert json.load(open(os.path.join(outs[0], g, 'side_info.json')))['stream_chunk'] == 128
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
    done = subprocess.run([sys.executable, '-m', 'linr_pcgc_amd.decoder', '--enc-dir', outs[1], '--dec-dir', str(tmp_path / 'dec'), '--ori-dir',
                           str(ori)], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    assert 'decoded 4 frames of 2 GOPs' in done.stdout and 'all equal to the input' in done.stdout


def test_encoder_mirror_reads_the_key(pkg, tmp_path):
    """encoder.encode with the reference's argument dict + 'stream_chunk': the files are those of codec's chunked streams - chunk by
    chunk the plain road's streams of the slices -, side_info carries S, 32 bits more are counted, and decoder.decode, unchanged,
    rebuilds every frame; without the key (or with 0) the files are the plain files."""
    from linr_pcgc_amd import custom_dataset as cd, decoder, encoder, synthetic
    from linr_pcgc_amd.function_utils import unpack_bitstream
    from linr_pcgc_amd.model_core import LINR_PCGC_Model
    from linr_pcgc_amd.stream_chunks import chunk_count, split_chunks
    ori = tmp_path / 'ori'
    ori.mkdir()
    for t in range(2):
        np.save(str(ori / ('frame_%04d.npy' % t)), synthetic.sphere_shell(7, 40 + t))
        cd.write_ply_ascii(str(ori / ('frame_%04d.ply' % t)), synthetic.sphere_shell(7, 40 + t))
    dataset = cd.MyDataset(str(ori), str(tmp_path / 'handle'), None, 'npy', stage=8)
    dataset.set_prefix_data({'offsets_ini': torch.tensor(cd.OFFSETS_INI, device='cuda'), 'min_point_num': 64})
    dataset[0]
    gen = lambda: LINR_PCGC_Model({'scale_num': dataset.scale_num, 'in_channel': 7, 'hidden_channel_conv': 8, 'block_layers': 1,
                                   'outstage': 8, 'instage': 1}).cuda()
    torch.manual_seed(8807)
    model = gen()
    out_dir = tmp_path / 'output' / 'gop_0_1'
    out_dir.mkdir(parents=True)
    torch.save({'model': model.state_dict(), 'epoch': 0, 'loss': 0.0, 'bitdepth': 8}, str(out_dir / 'model.pth'))
    test_set = cd.MytestDataset(str(ori), ori_type='ply')
    side = {}
    for name, extra in (('plain', {}), ('zero', {'stream_chunk': 0}), ('chunked', {'stream_chunk': 128})):
        enc_dir = tmp_path / name
        encoder.encode({'outputdir': str(tmp_path / 'output'), 'gop_names': ['gop_0_1'], 'Gen_Model': gen, 'dataset': dataset,
                        'encode_dir': str(enc_dir), **extra})
        decoder.decode({'gop_names': ['gop_0_1'], 'Gen_Model': gen, 'result_enc_dir': str(enc_dir), 'result_dec_dir': str(tmp_path / ('dec_' + name)),
                        'dataset': test_set, 'write_flag': False})
        side[name] = json.load(open(str(enc_dir / 'gop_0_1' / 'side_info.json')))
    _same_files(str(tmp_path / 'plain'), str(tmp_path / 'zero'))
    assert side['chunked'] == {**side['plain'], 'stream_chunk': 128}
    a = open(str(tmp_path / 'plain' / 'gop_0_1' / 'bins' / 'frame0000_scale0.bin'), 'rb').read()
    b = open(str(tmp_path / 'chunked' / 'gop_0_1' / 'bins' / 'frame0000_scale0.bin'), 'rb').read()
    n = int(dataset[0]['all_input_info'][0]['xyzqsc_t'].get_coord().shape[0])
    assert chunk_count(n, 128) > 1 and a != b
    assert all(len(split_chunks(s, n, 128)) == chunk_count(n, 128) for s in unpack_bitstream(b))
    with pytest.raises(ValueError):
        encoder.encode({'outputdir': str(tmp_path / 'output'), 'gop_names': ['gop_0_1'], 'Gen_Model': gen, 'dataset': dataset,
                        'encode_dir': str(tmp_path / 'bad'), 'stream_chunk': 100})
