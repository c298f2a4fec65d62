"""GPU: the range coder on the device (linr_rc_encode_codes, csrc/ac_device.hip: a wave per stream) and the opt-in codec path built
on it (model_core.encode_streams_device, codec.encode_gop(device_coder=True), run.py --device-coder).  The comparand is always the
host coder linr_ac_encode_binary_codes; bytes, lengths and offsets, all exact."""
import filecmp
import os

import numpy as np
import pytest
import torch

from test_device_coder_host import NS, REGIMES, draw, greedy_prefix, pack_symbols      # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def host_stream(L, c1, w, n, cap=None):
    cap = 2 * n + 64 if cap is None else cap
    out = np.empty(max(cap, 1), dtype=np.uint8)
    r = L.linr_ac_encode_binary_codes(c1.ctypes.data if n else None, w.ctypes.data if n else None, n, out.ctypes.data, cap)
    return r, out[:max(r, 0)].tobytes()


@pytest.fixture(scope='module')
def mixed(pkg):
    """Every length x regime of the host test and the long pending runs with their three endings, as ONE set of streams laid out in
    shared c1 / sym buffers: code values packed back to back (so most c1 offsets are odd, none a multiple of 64 by design), every
    stream's symbol words behind those of the one before it, both behind a non-zero lead.  The host coder's streams are computed once."""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    items = [draw(regime, n, 31 * n + r) for r, regime in enumerate(REGIMES) for n in NS]
    rng = np.random.default_rng(5)
    for steps in (16, 40):
        c1s, syms, pending = greedy_prefix(steps)
        assert pending >= 96
        items.append((np.asarray(c1s, dtype=np.uint16), np.asarray(syms, dtype=np.uint8)))
        for sym in (0, 1):
            items.append((np.asarray(c1s + [65535 if sym else 1] + rng.integers(1, 65536, 70).tolist(), dtype=np.uint16),
                          np.asarray(syms + [sym] + rng.integers(0, 2, 70).tolist(), dtype=np.uint8)))
    order = np.random.default_rng(6).permutation(len(items))          # lengths mixed, not sorted
    items = [items[i] for i in order]
    c1_all, w_all, desc = [np.full(7, 12345, dtype=np.uint16)], [np.full(3, 0xDEADBEEF, dtype=np.uint32)], []
    cb, wb = 7, 3
    for c1, s in items:
        w = pack_symbols(s)
        desc.append((cb, wb, len(c1)))
        c1_all.append(c1)
        w_all.append(w)
        cb, wb = cb + len(c1), wb + len(w)
    desc = np.asarray(desc, dtype=np.int64)
    assert (desc[:, 1] > 0).all() and (desc[desc[:, 2] > 0, 0] % 64 != 0).any() and len(set(desc[:, 2])) > 10
    want = [host_stream(L, c1, pack_symbols(s), len(c1)) for c1, s in items]
    assert all(r >= 1 for r, _ in want)
    return {'c1': torch.from_numpy(np.concatenate(c1_all)).cuda(), 'sym': torch.from_numpy(np.concatenate(w_all)).cuda(), 'desc': desc,
            'want': want}


class Call:
    """Buffers of one linr_rc_encode_codes call, all filled with the sentinel; run() launches and returns the entry's return code."""

    def __init__(self, L, c1, sym, tab, slack=0):
        from linr_pcgc_amd import _lib
        self.L, self.c1, self.sym, self.tab = L, c1, sym, np.ascontiguousarray(tab, dtype=np.int64)
        n = len(self.tab)
        self.n = n
        self.out_bytes = int((self.tab[:, 3] + self.tab[:, 4]).max()) + slack if n else 8
        total_cap = int(self.tab[:, 4].sum()) if n else 0
        fill = lambda m, dt: torch.from_numpy(np.full(m, SENTINEL, dtype=np.uint8).view(dt)).cuda()          # noqa: E731
        self.out = fill(self.out_bytes + 64, np.uint8)
        self.payload = fill(max(total_cap, 8) + 64, np.uint8)
        self.payload_bytes = max(total_cap, 8)
        self.len = fill(8 * (n + 1), np.int64)
        self.offsets = fill(8 * (n + 2), np.int64)
        self.ws_bytes = int(L.linr_rc_encode_ws_bytes(n, total_cap))
        self.ws = _lib.scratch(self.ws_bytes + 64, 'cuda')

    def args(self, **kw):
        a = dict(c1=self.c1.data_ptr(), sym=self.sym.data_ptr(), tab=self.tab.ctypes.data, n=self.n, out=self.out.data_ptr(),
                 out_bytes=self.out_bytes, len=self.len.data_ptr(), payload=self.payload.data_ptr(), payload_bytes=self.payload_bytes,
                 offsets=self.offsets.data_ptr(), ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes)
        a.update(kw)
        return [a[k] for k in ('c1', 'sym', 'tab', 'n', 'out', 'out_bytes', 'len', 'payload', 'payload_bytes', 'offsets', 'ws', 'ws_bytes')]

    def run(self, **kw):
        rc = self.L.linr_rc_encode_codes(*self.args(**kw), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        sent = int(np.frombuffer(bytes([SENTINEL]) * 8, dtype=np.int64)[0])
        return (bool((self.out == SENTINEL).all()) and bool((self.payload == SENTINEL).all()) and bool((self.len == sent).all())
                and bool((self.offsets == sent).all()))


def table(desc, caps=None):
    """Out regions one behind the other on 4-byte boundaries with a 4-byte gap between them; cap = 2 n + 64 unless given."""
    tab = np.empty((len(desc), 5), dtype=np.int64)
    tab[:, :3] = desc
    tab[:, 4] = 2 * tab[:, 2] + 64 if caps is None else caps
    size = ((tab[:, 4] + 3) & ~3) + 4
    tab[:, 3] = np.cumsum(size) - size
    return tab


def check_call(call, want, nospc=()):
    """Lengths, offsets, payload and the out regions of a finished call against the host coder's streams."""
    n, tab = call.n, call.tab
    lens = call.len.cpu().numpy()
    offs = call.offsets.cpu().numpy()
    out = call.out.cpu().numpy()
    payload = call.payload.cpu().numpy()
    counted = [0 if i in nospc else want[i][0] for i in range(n)]
    assert lens[:n].tolist() == [-2 if i in nospc else want[i][0] for i in range(n)]
    assert offs[:n + 1].tolist() == np.concatenate([[0], np.cumsum(counted)]).tolist()
    covered = np.zeros(out.size, dtype=bool)
    for i in range(n):
        o, cap = int(tab[i, 3]), int(tab[i, 4])
        covered[o:o + cap] = True
        if i in nospc:
            continue
        r, data = want[i]
        assert out[o:o + r].tobytes() == data, i
        assert payload[offs[i]:offs[i + 1]].tobytes() == data, i
    assert (out[~covered] == SENTINEL).all(), 'a byte outside every stream\'s region of cap bytes was written'
    assert (payload[offs[n]:] == SENTINEL).all()
    sent = np.frombuffer(bytes([SENTINEL]) * 8, dtype=np.int64)[0]
    assert lens[n] == sent and offs[n + 1] == sent


def test_many_streams_in_one_launch_are_the_host_coders_streams(mixed):
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    call = Call(L, mixed['c1'], mixed['sym'], table(mixed['desc']))
    assert call.run() == 0
    check_call(call, mixed['want'])
    first = (call.len.cpu(), call.offsets.cpu(), call.out.cpu(), call.payload.cpu())
    assert call.run() == 0                                  # a second call into the same buffers gives the same result
    for a, b in zip(first, (call.len.cpu(), call.offsets.cpu(), call.out.cpu(), call.payload.cpu())):
        assert torch.equal(a, b)


def test_exact_caps_fit_and_the_regions_behind_them_keep_their_sentinel(mixed):
    """cap = the host's length for every stream: each fits exactly, and check_call sees no byte behind any cap touched (the 4-byte
    gaps between the regions and the 1..3 bytes that round a cap up to the next boundary)."""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    caps = np.asarray([r for r, _ in mixed['want']], dtype=np.int64)
    assert (caps % 4 != 0).any()
    call = Call(L, mixed['c1'], mixed['sym'], table(mixed['desc'], caps))
    assert call.run() == 0
    check_call(call, mixed['want'])


def test_a_stream_without_space_is_enospc_and_the_others_are_exact(mixed):
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    want, desc = mixed['want'], mixed['desc']
    caps = 2 * desc[:, 2] + 64
    big = int(np.argmax([r for r, _ in want]))              # crosses many staging blocks before it runs out
    small = int(np.argmin([r if r > 1 else 1 << 30 for r, _ in want]))
    zero = next(i for i in range(len(want)) if i not in (big, small))
    caps[big], caps[small], caps[zero] = want[big][0] - 1, want[small][0] - 1, 0
    assert want[big][0] > 1024
    call = Call(L, mixed['c1'], mixed['sym'], table(desc, caps))
    assert call.run() == 0
    check_call(call, want, nospc=(big, small, zero))


def test_bad_arguments_launch_nothing(mixed):
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    desc = mixed['desc'][:6]
    good = table(desc)
    call = Call(L, mixed['c1'], mixed['sym'], good, slack=16)
    for name in ('c1', 'sym', 'tab', 'out', 'len', 'payload', 'offsets', 'ws'):
        assert call.run(**{name: None}) == -1, name
    assert call.run(n=-1) == -1 and call.run(out_bytes=-1) == -1 and call.run(payload_bytes=-1) == -1
    assert call.run(out_bytes=int((good[:, 3] + good[:, 4]).max()) - 1) == -1            # a region past out_bytes
    assert call.run(payload_bytes=int(good[:, 4].sum()) - 1) == -1
    assert call.run(ws_bytes=call.ws_bytes - 1) == -1                                    # a workspace one byte short

    def with_row(i, col, value):
        t = good.copy()
        t[i, col] = value
        return np.ascontiguousarray(t)
    bad = [with_row(2, 2, -1), with_row(2, 4, -1), with_row(2, 0, -1), with_row(2, 1, -1), with_row(2, 2, (1 << 27) - 1),
           with_row(3, 3, good[3, 3] + 2),                                               # an unaligned out offset
           with_row(3, 3, good[2, 3] + 4)]                                               # overlaps the region in front of it
    assert good[2, 4] > 4
    for t in bad:
        assert call.run(tab=t.ctypes.data) == -1
    assert call.run(n=0) == 0
    assert call.untouched()
    assert call.run() == 0                                  # and the good call does run
    check_call(call, mixed['want'][:6])


def test_encode_streams_device(mixed):
    from linr_pcgc_amd import model_core
    got = model_core.encode_streams_device(mixed['c1'], mixed['sym'], mixed['desc'])
    assert got == [data for _, data in mixed['want']]
    assert model_core.encode_streams_device(mixed['c1'], mixed['sym'], []) == []
    with pytest.raises(ValueError):
        model_core.encode_streams_device(mixed['c1'], mixed['sym'], [(mixed['c1'].numel() - 3, 0, 4)])


# ---- the codec path ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def shell_gop(pkg, golden_dir):
    """Three frames of the golden 128-cube shell, an untrained model of seed 8807, and the default path's result (fp32 and bf16)."""
    from linr_pcgc_amd import codec, overfit
    pts = np.load(os.path.join(golden_dir, 'octree_shell128.npz'))['points']
    gop = overfit.Gop(None, [pts, pts, pts], None, 64, 'cuda')
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807)
    ref = {prec: codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda'), gop, 8, precision=prec) for prec in ('f32', 'bf16')}
    return gop, model, ref


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
@pytest.mark.parametrize('group', [1, 2, 3])
def test_device_coder_gop_is_the_default_gop(shell_gop, precision, group, monkeypatch):
    from concurrent import futures
    from linr_pcgc_amd import codec, overfit
    gop, model, ref = shell_gop
    want = ref[precision]
    row_off = gop.frames[0].row_off
    assert any(int(r) % 32 for r in row_off[1:-1]), 'the ragged case: a scale that does not start on a word boundary'

    def no_pool(*a, **k):
        raise AssertionError('the device coder path starts no coder threads')
    monkeypatch.setattr(futures, 'ThreadPoolExecutor', no_pool)
    enc = codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda'), gop, 8, precision=precision, device_coder=True, coder_group=group)
    monkeypatch.undo()
    assert enc['frames'] == want['frames'] and len(enc['frames']) == 3 and len(enc['frames'][0]) == gop.frames[0].n_scales
    assert enc['model_bin'] == want['model_bin'] and enc['side_info'] == want['side_info']
    assert enc['low_enc_bytes'] == want['low_enc_bytes'] and enc['bpp'] == want['bpp']
    if group == 2:
        dec = codec.decode_gop(overfit.gen_model(gop.scale_num, 'cuda'), enc, 'cuda')
        for d, info, mn in zip(dec, gop.infos, gop.coord_mins):
            assert torch.equal(d, torch.as_tensor(info['ori']).cuda() + torch.tensor(mn, device='cuda', dtype=torch.int32))


def test_coder_group_out_of_range_is_refused(shell_gop):
    from linr_pcgc_amd import codec, overfit
    gop, model, _ = shell_gop
    for g in (0, 65):
        with pytest.raises(ValueError):
            codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda'), gop, 8, device_coder=True, coder_group=g)


@pytest.mark.parametrize('flags', [[], ['--pipeline', '--precision', 'bf16']], ids=['plain', 'pipeline-bf16'])
def test_run_device_coder_writes_identical_files(pkg, golden_dir, tmp_path, flags):
    """run.py --device-coder on the two-frame, one-epoch configuration of the device-codes test: every file under result_enc/ is the
    file a run without the flag writes; once more with --pipeline --precision bf16."""
    from linr_pcgc_amd import run
    pts = np.load(os.path.join(golden_dir, 'octree_shell128.npz'))['points']
    for t in range(2):
        np.save(str(tmp_path / ('frame%d.npy' % t)), pts)
    outs = []
    for flag in ([], ['--device-coder', '--coder-group', '1' if flags else '8']):
        out = str(tmp_path / ('coder' if flag else 'plain'))
        args = run.parse(['--input-glob', str(tmp_path / 'frame*.npy'), '--frames', '2', '--gop', '2', '--first-epoch', '1', '--seed', '8807',
                          '--out', out] + flags + flag)
        assert args.device_coder is bool(flag)
        summary, _ = run.run_sequence_job(args, files=run.resolve_files(args))
        assert summary['gops'] == 1 and summary['frames'] == 2
        outs.append(os.path.join(out, 'result_enc'))
    names = sorted(os.path.relpath(os.path.join(d, f), outs[0]) for d, _, fs in os.walk(outs[0]) for f in fs)
    assert names == sorted(os.path.relpath(os.path.join(d, f), outs[1]) for d, _, fs in os.walk(outs[1]) for f in fs)
    assert len(names) == 2 * 5 + 3                          # frames x scales streams, model.bin, low_enc_bytes.bin, side_info.json
    for n in names:
        assert filecmp.cmp(os.path.join(outs[0], n), os.path.join(outs[1], n), shallow=False), n
