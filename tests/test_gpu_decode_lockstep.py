"""GPU tests of the lock-step GOP decoder: one scale of many frames per call (linr_decode_scale_batch), its segmented kernel map
(linr_kmap_build_segments) and its sort-free child expansion (linr_children_segments).  Everything here is exact: lossless decode
is the strict check of the probabilities (one bit off desynchronises the range decoder), the map and the children are compared
bitwise with the per-frame entries / the torch mirror of octree_level.upper_layer."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gop_and_streams(clouds, precision='f32', hidden=8, scale_num=None):
    from linr_pcgc_amd import codec, overfit
    gop = overfit.Gop(None, clouds, scale_num, 64, 'cuda')
    gen = lambda seed=None: overfit.gen_model(gop.scale_num, 'cuda', seed=seed, hidden=hidden)
    enc = codec.encode_gop(gen(8807), gen(), gop, 8, precision=precision)
    return gop, gen, enc


def _truth(gop, i):
    return torch.as_tensor(gop.infos[i]['ori']).cuda() + torch.tensor(gop.coord_mins[i], device='cuda', dtype=torch.int32)


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_lockstep_gop_decode_equals_per_frame(pkg, precision):
    """decode_gop(lockstep=B) for B = 5 (one group), 2 (groups of 2, 2, 1) and 1 gives, frame by frame, what the per-frame decoder
    gives and what was encoded; a frame list comes back in its own order."""
    from linr_pcgc_amd import codec, synthetic
    gop, gen, enc = _gop_and_streams([synthetic.sphere_shell(7, 40 + t) for t in range(5)], precision)
    serial = codec.decode_gop(gen(), enc, 'cuda')
    for lockstep in (5, 2, 1):
        got = codec.decode_gop(gen(), enc, 'cuda', lockstep=lockstep)
        assert len(got) == 5
        for i in range(5):
            assert torch.equal(got[i], serial[i]), (lockstep, i)
            assert torch.equal(got[i], _truth(gop, i)), (lockstep, i)
    got = codec.decode_gop(gen(), enc, 'cuda', frames=[3, 1], lockstep=2)
    assert len(got) == 2 and torch.equal(got[0], serial[3]) and torch.equal(got[1], serial[1])
    # groups in flight on their own streams
    got = codec.decode_gop(gen(), enc, 'cuda', lockstep=2, workers=2)
    assert all(torch.equal(a, b) for a, b in zip(got, serial))


def test_lockstep_ragged_group(pkg):
    """One group of a shell of thousands of rows, one of a few rows and the first shell again: segment boundaries off every
    multiple of 64 and 256, and identical coordinates in two frames that must not see each other."""
    from linr_pcgc_amd import codec, synthetic
    # two scales for every frame (the small shell has no more above 64 points), so that the three share ONE group
    gop, gen, enc = _gop_and_streams([synthetic.sphere_shell(7, 45), synthetic.sphere_shell(7, 6), synthetic.sphere_shell(7, 45)], scale_num=2)
    assert [len(f) for f in enc['frames']] == [2, 2, 2]
    assert codec.lockstep_groups([0, 1, 2], {i: len(enc['frames'][i]) for i in range(3)}, 3) == [[0, 1, 2]]
    rows = [int(f.rows) for f in gop.frames]
    assert rows[1] < 256 < 4096 < rows[0] and rows[0] % 64 and (rows[0] + rows[1]) % 64
    serial = codec.decode_gop(gen(), enc, 'cuda')
    got = codec.decode_gop(gen(), enc, 'cuda', lockstep=3)
    assert len(got) == 3
    for i in range(3):
        assert torch.equal(got[i], serial[i]), i
        assert torch.equal(got[i], _truth(gop, i)), i


def _kmap(L, coords, seg):
    n = int(seg[-1])
    ld = (n + 63) // 64 * 64
    ws = torch.empty(max(L.linr_kmap_workspace_bytes(n), 8) + 8, dtype=torch.uint8, device='cuda')
    base = (ws.data_ptr() + 7) & ~7
    per = torch.full((27, ld), -1, dtype=torch.int32, device='cuda')
    for f in range(len(seg) - 1):
        a, b = int(seg[f]), int(seg[f + 1])
        assert L.linr_kmap_build(coords.data_ptr() + 12 * a, b - a, per.data_ptr(), ld, a, base, L.linr_kmap_workspace_bytes(n), _stream()) == 0
    got = torch.full((27, ld), -1, dtype=torch.int32, device='cuda')
    seg_h = np.asarray(seg, dtype=np.int64)
    assert L.linr_kmap_build_segments(coords.data_ptr(), seg_h.ctypes.data, len(seg) - 1, got.data_ptr(), ld, base,
                                      L.linr_kmap_workspace_bytes(n), _stream()) == 0
    torch.cuda.synchronize()
    return per, got


def test_segmented_kernel_map_equals_per_segment_build(pkg):
    """linr_kmap_build_segments against one linr_kmap_build(row_base = seg_off[f]) per segment, bitwise: a shell, the same shell
    again, an empty segment, a 1-row segment and a segment whose first voxel is a spatial neighbour of the previous segment's
    last.  No entry of a segment points outside it."""
    from linr_pcgc_amd import _lib, synthetic
    L = _lib.lib()
    shell = torch.as_tensor(synthetic.sphere_shell(7, 15)).to(torch.int32)          # ~2 800 rows: more than one block
    one = shell[-1:].clone()                                                         # the 1-row segment
    nxt = shell[:200].clone()
    nxt = nxt - nxt[0] + one[0] + torch.tensor([0, 0, 1], dtype=torch.int32)         # starts at the z neighbour of the row before it
    parts = [shell, shell.clone(), shell[:0], one, nxt]
    seg = np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])])
    coords = torch.cat(parts, dim=0).contiguous().cuda()
    assert bool((coords >= 0).all())
    per, got = _kmap(L, coords, seg)
    assert torch.equal(per, got)
    n = int(seg[-1])
    rows = torch.arange(n, device='cuda')
    seg_t = torch.as_tensor(seg, device='cuda')
    f = torch.searchsorted(seg_t, rows, right=True) - 1
    lo, hi = seg_t[f], seg_t[f + 1]
    live = got[:, :n]
    assert bool(((live == -1) | ((live >= lo) & (live < hi))).all())
    assert bool((live[13] == rows).all())                                            # the centre tap is the row itself
    # the two identical shells have the same map up to their row base
    a, b = int(seg[1]), int(seg[2])
    m0, m1 = got[:, :a], got[:, a:b]
    assert torch.equal(torch.where(m0 >= 0, m0 + a, m0), m1)


def _children(L, coords, occ, seg, cap=None):
    n = int(seg[-1])
    need = L.linr_children_segments_ws_bytes(n)
    ws = torch.empty(need + 256, dtype=torch.uint8, device='cuda')
    base = (ws.data_ptr() + 255) & ~255
    cap = 8 * n if cap is None else cap
    child = torch.full((max(cap, 1) + 8, 3), -7, dtype=torch.int32, device='cuda')
    seg_h = np.asarray(seg, dtype=np.int64)
    off = (ctypes.c_int64 * len(seg))()
    rc = L.linr_children_segments(coords.data_ptr(), occ.data_ptr(), seg_h.ctypes.data, len(seg) - 1, child.data_ptr(), cap, off, base,
                                  need, _stream())
    torch.cuda.synchronize()
    return rc, child, list(off)


def test_children_segments_equal_upper_layer(pkg):
    """linr_children_segments against octree_level.upper_layer per frame: segments of 0, 1, 300 and 5 000 parents (the last spans
    more than one scan tile), random occupancy with at least one child per row, rows with exactly one child and rows with all 8.
    A child buffer one short of the total is refused, and nothing is written behind it."""
    from linr_pcgc_amd import _lib
    from linr_pcgc_amd.module_utils import octree_level_obj, unique_sorted
    L = _lib.lib()
    g = torch.Generator().manual_seed(20)
    sizes = [0, 1, 300, 5000]
    parts, occs = [], []
    for m in sizes:
        # sorted unique parents in a 24^3 box: dense enough for x runs and (x, y) runs of many rows
        p = unique_sorted(torch.randint(0, 24, (3 * m, 3), generator=g, dtype=torch.int32).cuda())[:m] if m else \
            torch.zeros((0, 3), dtype=torch.int32, device='cuda')
        assert p.shape[0] == m
        o = (torch.rand((m, 8), generator=g) < 0.4).float()
        o[torch.arange(m), torch.randint(0, 8, (m,), generator=g)] = 1.0             # at least one child
        if m >= 300:
            o[::7] = 0.0
            o[torch.arange(0, m, 7), torch.randint(0, 8, (len(range(0, m, 7)),), generator=g)] = 1.0      # exactly one
            o[3::11] = 1.0                                                           # all eight
        parts.append(p)
        occs.append(o.cuda())
    seg = np.concatenate([[0], np.cumsum(sizes)])
    coords = torch.cat(parts, dim=0).contiguous()
    occ = torch.cat(occs, dim=0).contiguous()
    want = [octree_level_obj.upper_layer(p, o) if p.shape[0] else p for p, o in zip(parts, occs)]
    counts = [int(w.shape[0]) for w in want]
    assert counts == [int(o.sum()) for o in occs]
    rc, child, off = _children(L, coords, occ, seg)
    assert rc == 0
    assert off == [0] + list(np.cumsum(counts))
    total = off[-1]
    assert torch.equal(child[:total], torch.cat(want, dim=0))
    assert bool((child[total:] == -7).all())
    rc, child, off = _children(L, coords, occ, seg, cap=total - 1)
    assert rc == -2
    assert bool((child[total - 1:] == -7).all())


def test_decode_scale_batch_argument_checks(pkg):
    """linr_decode_scale_batch refuses n_frames outside 1..64, a misaligned or short workspace and NULL streams before it
    launches anything; a valid call afterwards succeeds."""
    from linr_pcgc_amd import _lib, codec, synthetic
    from linr_pcgc_amd.function_utils import unpack_bitstream
    from linr_pcgc_amd.model_codec import Model_Estimate
    from linr_pcgc_amd.module_utils import unique_sorted
    L = _lib.lib()
    gop, gen, enc = _gop_and_streams([synthetic.sphere_shell(7, 41), synthetic.sphere_shell(7, 47)])
    side = dict(enc['side_info'])
    side.pop('arith_version', None)
    side['final_bytes'] = enc['model_bin']
    m, _ = Model_Estimate().decompress_model(gen(), side)
    lows, _ = codec.dec_all_frame_low_xyz(enc['low_enc_bytes'])
    lv = [unique_sorted(torch.tensor(lows[i].astype(np.int32), device='cuda')).contiguous() for i in range(2)]
    seg = np.asarray([0, lv[0].shape[0], lv[0].shape[0] + lv[1].shape[0]], dtype=np.int64)
    n = int(seg[-1])
    coord = torch.cat(lv, dim=0).contiguous()
    streams = [np.frombuffer(b, dtype=np.uint8) for i in range(2) for b in unpack_bitstream(enc['frames'][i][-1])]
    ptrs = (ctypes.c_void_p * 16)(*[b.ctypes.data if b.size else None for b in streams])
    lens = (ctypes.c_int64 * 16)(*[int(b.size) for b in streams])
    need = L.linr_decode_scale_batch_ws_bytes(n, 2, 1, 0, -1, 0)
    assert need > 0 and L.linr_decode_scale_batch_ws_bytes(n, 0, 1, 0, -1, 0) == 0 and L.linr_decode_scale_batch_ws_bytes(n, 65, 1, 0, -1, 0) == 0
    ws = torch.empty(need + 512, dtype=torch.uint8, device='cuda')
    base = (ws.data_ptr() + 255) & ~255
    p_host, s_host = m._host_buffers(n)
    child = torch.full((8 * n, 3), -7, dtype=torch.int32, device='cuda')
    off = (ctypes.c_int64 * 66)()
    opts = _lib.LinrDecodeOpts(0, 4, 0)                                              # plain streams, 4 host threads
    torch.cuda.synchronize()

    def call(n_frames=2, ws_ptr=base, ws_bytes=need, streams_p=ptrs, seg_h=seg):
        return L.linr_decode_scale_batch(coord.data_ptr(), seg_h.ctypes.data, n_frames, gop.scale_num - 1, gop.scale_num, 1,
                                         m.flat_parameters().data_ptr(), None, 0.0, 0.0, streams_p, lens, ws_ptr, ws_bytes,
                                         p_host.data_ptr(), s_host.data_ptr(), child.data_ptr(), 8 * n, off, ctypes.byref(opts), _stream())
    seg65 = np.concatenate([seg, np.full(63, n, dtype=np.int64)])                    # 65 segments, the last 63 empty
    assert call(n_frames=0) == -1
    assert call(n_frames=65, seg_h=seg65) == -1
    assert call(ws_ptr=base + 8) == -3
    assert call(ws_bytes=need // 2) == -2
    assert call(streams_p=None) == -1
    torch.cuda.synchronize()
    assert bool((child == -7).all())                                                 # nothing ran
    assert call() == 0
    assert 0 < off[1] < off[2] <= 8 * n
    # ... and it is the next level of both frames
    for i in range(2):
        want = m.decode_scale(lv[i], gop.scale_num - 1, enc['frames'][i][-1], 8)
        assert torch.equal(child[off[i]:off[i + 1]], want)


def test_lockstep_is_ignored_for_wide_models(pkg):
    """hidden_channel_conv = 16 has no single-call decoder scale: lockstep is ignored and the GOP decodes as by default."""
    from linr_pcgc_amd import codec, synthetic
    gop, gen, enc = _gop_and_streams([synthetic.sphere_shell(6, 20), synthetic.sphere_shell(6, 22)], hidden=16)
    default = codec.decode_gop(gen(), enc, 'cuda')
    got = codec.decode_gop(gen(), enc, 'cuda', lockstep=2)
    assert len(got) == 2
    for i in range(2):
        assert torch.equal(got[i], default[i])
        assert torch.equal(got[i], _truth(gop, i))
