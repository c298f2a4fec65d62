"""GPU: linr_octree_levels (csrc/octree.hip) on clouds of 12 to 20 coordinate bits - the sparse levels (head flags, scan, rank: work and
workspace follow the rows) alone and chained with bitmap levels.  Everything is integer work: every comparison is bit-exact.  The
reference is plain numpy (np.unique of child >> 1, set membership for the occupancy) and the per-level entry (LINR_OCTREE_PER_LEVEL=1).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# the plan of include/linr_hip.h (linr_octree_levels): a level whose parents have pb bits per coordinate is a bitmap of 2^(3 pb) bits
# when pb <= 10 and the bitmap has at most 2^19 words or at most 12 words per possible row; every other level is sparse
DENSE_MAX_PB, DENSE_FLOOR_WORDS, DENSE_RATIO = 10, 1 << 19, 12
SCAN_SCRATCH = 1 << 20          # hipcub's own scratch of the scan and the alignment of the workspace's parts: under 1 MB (the header)


def _key(c):
    c = c.astype(np.int64)
    return (c[:, 0] << 40) | (c[:, 1] << 20) | c[:, 2]


def _np_levels(child, levels):
    """[(parents int32 [n,3], occ float32 [n,8])] of `levels` levels below a sorted unique child list"""
    out = []
    child = child.astype(np.int64).reshape(-1, 3)
    for _ in range(levels):
        parent = np.unique(child >> 1, axis=0)
        keys = _key(child)
        occ = np.zeros((len(parent), 8), dtype=np.float32)
        for d in range(8):
            kid = parent * 2 + np.array([d >> 2, (d >> 1) & 1, d & 1])
            occ[:, d] = np.isin(_key(kid), keys)
        out.append((parent.astype(np.int32), occ))
        child = parent
    return out


def _cloud(case, bits, rng):
    top = (1 << bits) - 1
    if case == 'random':                    # the whole cube: nearly every parent has one child
        c = rng.integers(0, 1 << bits, size=(5000, 3))
    elif case == 'corner_box':              # dense cells at the top corner: every sibling pattern, heads with dx, dy or dz = 1, key bit 3 bits - 1
        c = np.concatenate([rng.integers(top - 39, top + 1, size=(4000, 3)), [[top, top, top]]])
    elif case == 'full_cell':               # one complete 2 x 2 x 2 cell
        c = np.array([[top - 1 + (d >> 2), 6 + ((d >> 1) & 1), (1 << (bits - 1)) + (d & 1)] for d in range(8)])
    else:                                   # 'm1', 'm2', 'm3'
        c = np.array([[top, 0, 5], [top, 1, 4], [3, top, top]])[:int(case[1:])]
    return np.unique(c, axis=0).astype(np.int32)


def _check_levels(got, child, bits, max_levels=64):
    parents, occ, counts = got
    want = _np_levels(child, min(max_levels, bits - 1))
    assert counts == [len(p) for p, _ in want]
    off = 0
    for level, (p, o) in enumerate(want):
        assert np.array_equal(parents[off:off + len(p)].cpu().numpy(), p), 'coordinates of level %d' % level
        assert np.array_equal(occ[off:off + len(p)].cpu().numpy(), o), 'occupancy of level %d' % level
        off += len(p)
    assert parents.shape[0] == off and occ.shape[0] == off


@pytest.mark.parametrize('bits', [12, 16, 20])
@pytest.mark.parametrize('case', ['random', 'corner_box', 'full_cell', 'm1', 'm2', 'm3'])
def test_deep_levels_match_numpy(pkg, bits, case):
    """ops.octree_levels at coord_bits 12, 16 and 20 against numpy, level by level: coordinates, occupancy, counts."""
    from linr_pcgc_amd import _lib, ops
    assert _lib.lib().linr_octree_levels_count(bits, 64) == bits - 1
    child = _cloud(case, bits, np.random.default_rng(bits))
    if case == 'corner_box':
        assert child.max() == (1 << bits) - 1 and len(child) > 3000
    got = ops.octree_levels(torch.from_numpy(child).cuda(), bits, 64)
    assert got is not None
    _check_levels(got, child, bits)


@pytest.mark.parametrize('bits', [12, 16, 20])
def test_deep_levels_with_a_live_count_on_the_device(pkg, bits):
    """count_dev < m: the rows behind the live count are not part of the cloud."""
    from linr_pcgc_amd import ops
    child = _cloud('corner_box', bits, np.random.default_rng(bits + 1))
    live = len(child) // 2 + 1
    got = ops.octree_levels(torch.from_numpy(child).cuda(), bits, 64, count_dev=torch.tensor([live], dtype=torch.int64, device='cuda'))
    _check_levels(got, child[:live], bits)


def _raw_levels(child, m, bits, max_levels, fill):
    """linr_octree_levels through the binding with a workspace of this test's own: every byte preset to `fill`"""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    nlev = L.linr_octree_levels_count(bits, max_levels)
    cap = max(1, L.linr_octree_levels_rows(m, bits, max_levels))
    parents = torch.zeros((cap, 3), dtype=torch.int32, device='cuda')
    occ = torch.zeros((cap, 8), dtype=torch.float32, device='cuda')
    counts = torch.full((nlev,), -7, dtype=torch.int64, device='cuda')
    nbytes = L.linr_octree_levels_workspace_bytes(m, bits, max_levels)
    ws = torch.full((nbytes + 256,), fill, dtype=torch.uint8, device='cuda')
    base = (ws.data_ptr() + 255) & ~255
    rc = L.linr_octree_levels(child.data_ptr() if m else None, m, None, bits, max_levels, parents.data_ptr(), occ.data_ptr(),
                              counts.data_ptr(), base, nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return parents, occ, counts.tolist()


@pytest.mark.parametrize('bits', [12, 16, 20])
def test_deep_levels_of_an_empty_cloud(pkg, bits):
    """m = 0: every level's count is zero and nothing else is touched; the tensor wrapper has no levels to return."""
    from linr_pcgc_amd import ops
    _, _, counts = _raw_levels(None, 0, bits, 64, 0xFF)
    assert counts == [0] * (bits - 1)
    assert ops.octree_levels(torch.zeros((0, 3), dtype=torch.int32, device='cuda'), bits, 64) is None


def _mixed_cloud():
    """13 bits, 27,000 points: a 30^3 lattice of pitch 273 with a jitter of +-2 - single children on the fine levels, shared parents
    and more than one workgroup on the coarse ones"""
    rng = np.random.default_rng(13)
    g = np.arange(30) * 273
    c = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) + rng.integers(0, 5, size=(27000, 3))
    assert c.max() >= 1 << 12 and c.max() < 1 << 13
    return c[rng.permutation(len(c))].astype(np.int32)


def _frames_equal(a, b):
    assert a['point_num'] == b['point_num'] and a['scale_num'] == b['scale_num'] and a['coord_data_min'] == b['coord_data_min']
    assert torch.equal(a['ori'], b['ori'])
    for x, y in zip(a['all_input_info'], b['all_input_info']):
        assert x['scale_idx'] == y['scale_idx']
        assert torch.equal(x['coord'], y['coord']) and torch.equal(x['occ'], y['occ']) and torch.equal(x['ground_truth'], y['ground_truth'])


def test_sparse_and_bitmap_levels_in_one_chain(pkg, monkeypatch):
    """A 13-bit cloud whose fine levels are sparse and whose coarse levels are bitmaps (read off the workspace size): the chain across
    the switch equals numpy and the per-level entry, through prepare_frame."""
    from linr_pcgc_amd import _lib
    from linr_pcgc_amd.module_utils import prepare_frame
    pts = _mixed_cloud()
    m = len(np.unique(pts, axis=0))
    ws = _lib.lib().linr_octree_levels_workspace_bytes(m, 13, 64)
    assert ws < (1 << 36) // 8                              # no bitmap over the 12-bit parents of level 0: that level is sparse
    assert ws > 24 * (m + 1) + SCAN_SCRATCH                 # more than keys, flags and scan of the rows: some level holds a bitmap
    dev_pts = torch.from_numpy(pts).cuda()
    fast = prepare_frame(dev_pts, None, 64, device='cuda', with_offsets=False)
    monkeypatch.setenv('LINR_OCTREE_PER_LEVEL', '1')
    slow = prepare_frame(dev_pts, None, 64, device='cuda', with_offsets=False)
    monkeypatch.delenv('LINR_OCTREE_PER_LEVEL')
    _frames_equal(fast, slow)
    ori = np.unique(pts - pts.min(axis=0), axis=0)
    assert np.array_equal(fast['ori'].cpu().numpy(), ori) and fast['coord_data_min'] == pts.min(axis=0).tolist()
    want = _np_levels(ori, 12)
    stop = next(i for i, (p, _) in enumerate(want) if len(p) < 64)
    assert fast['scale_num'] == stop + 1 and stop >= 8        # levels of both kinds are part of the frame
    for info, (p, o) in zip(fast['all_input_info'], want):
        assert np.array_equal(info['coord'].cpu().numpy(), p) and np.array_equal(info['occ'].cpu().numpy(), o)


def _workspace_bound(m, bits, max_levels):
    """the bound of include/linr_hip.h: 24 bytes per row (two key lists, flags, scan) + the dense levels (4 bytes per bitmap word of
    each, 8 per word of the largest for its counts and scan) + the scan's scratch"""
    prev, bitmap_words, widest = m, 0, 0
    for level in range(min(max_levels, bits - 1)):
        pb = bits - level - 1
        cells = 1 << (3 * pb)
        cap, words = min(prev, cells), (cells + 31) >> 5
        if pb <= DENSE_MAX_PB and (words <= DENSE_FLOOR_WORDS or words <= DENSE_RATIO * cap):
            bitmap_words += words
            widest = max(widest, words)
        prev = cap
    return 24 * (m + 1), 4 * bitmap_words + 8 * (widest + 1) + SCAN_SCRATCH


def test_workspace_follows_the_points(pkg):
    """coord_bits 20, 100,000 rows: the workspace is what the header states - a share per row and the bitmaps of the coarse levels,
    nothing of the 2^57-cell volume of level 0 - and doubling the rows adds no more than twice the rows' share."""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    m = 100000
    per_rows, dense = _workspace_bound(m, 20, 64)
    ws = L.linr_octree_levels_workspace_bytes(m, 20, 64)
    assert 0 < ws <= per_rows + dense
    assert dense < 16 << 20                                  # (the coarse bitmaps of a 20-bit cloud are a few MB)
    ws2 = L.linr_octree_levels_workspace_bytes(2 * m, 20, 64)
    assert ws <= ws2 <= ws + 2 * per_rows
    assert L.linr_octree_levels_rows(m, 20, 64) <= 19 * m


@pytest.mark.parametrize('bits,case', [(20, 'corner_box'), (13, 'mixed')])
def test_workspace_needs_no_initialisation(pkg, bits, case):
    """A workspace preset to 0xFF bytes gives the rows of one preset to zero, and numpy's."""
    child = np.unique(_mixed_cloud(), axis=0) if case == 'mixed' else _cloud(case, bits, np.random.default_rng(4))
    dev = torch.from_numpy(child).cuda()
    a = _raw_levels(dev, len(child), bits, 64, 0xFF)
    b = _raw_levels(dev, len(child), bits, 64, 0)
    total = sum(a[2])
    assert a[2] == b[2] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _check_levels((a[0][:total], a[1][:total], a[2]), child, bits)


def test_sparse_12_bit_frame_end_to_end(pkg, monkeypatch):
    """The 8-bit sphere with its coordinates multiplied by 16 (a 12-bit span, isolated voxels): prepare_frame's one-call path equals the
    per-level path, and the frame goes through overfit.Gop, a few training steps, encode_gop and decode_gop losslessly."""
    from linr_pcgc_amd import codec, overfit, synthetic
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    from linr_pcgc_amd.module_utils import prepare_frame
    pts = (synthetic.sphere_shell(8, 100) * 16).astype(np.int32)
    dev_pts = torch.from_numpy(pts).cuda()
    fast = prepare_frame(dev_pts, None, 64, device='cuda', with_offsets=False)
    monkeypatch.setenv('LINR_OCTREE_PER_LEVEL', '1')
    slow = prepare_frame(dev_pts, None, 64, device='cuda', with_offsets=False)
    monkeypatch.delenv('LINR_OCTREE_PER_LEVEL')
    _frames_equal(fast, slow)
    assert fast['scale_num'] == 10 and fast['point_num'] == len(pts)
    gop = overfit.Gop(None, [pts], None, 64, 'cuda')
    assert gop.scale_num == 10
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=12)
    opt = FlatAdam(model, lr=1e-3)
    for _ in range(3):
        train_step(model, opt, gop.frames[0], gop.point_nums[0])
    enc = codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda'), gop, 8)
    dec = codec.decode_gop(overfit.gen_model(gop.scale_num, 'cuda'), enc, 'cuda')
    ref = torch.as_tensor(gop.infos[0]['ori']).cuda() + torch.tensor(gop.coord_mins[0], device='cuda', dtype=torch.int32)
    assert torch.equal(dec[0], ref), 'decoded geometry must be bit-exact'
