"""Op-level reference of the width-8 fp32 convolution family (csrc/fused.hip, fused_bwd.hip, wgrad.hip, occ_wgrad.hip, spconv.hip): the
clouds and inputs of every case that tests/test_gpu_conv8_ops.py runs, the float64 value of every sum the kernels form, and the criterion.
tests/test_conv8_ref.py checks this file on the CPU (no kernel); nothing here imports GPU code, and every function works on tensors of
any device (the GPU test computes the references on the GPU, from the device's own earlier outputs).

The criterion is tests/gpu_common.py::_within_rounding: every produced entry within C_ROUND 2^-24 of `absum`, the float64 sum of its own
terms taken over their absolute values - |x| (*) |W| + |b| + |res| + |old| forward, |g| (*) |W|^T + the added terms backward-data, the sum
over the rows of |x| |g| for a weight gradient, the sum of |slab| for linr_slab_reduce.  A masked entry (LINR_RELU_MASK on an exact zero)
has no term at all: its absum is 0 and the stored value must be 0.  Every sum below is written once, as a function `*_sum` that is linear
in each operand; the reference calls it with the operands in float64 and again with their absolute values.

Clouds (sorted unique voxel lists; oracle.octree.neighbour_table is the reference map):
  pair_k        two voxels, the second at the offset of tap k (k != 13): every row has the centre and exactly one other tap
  single        one voxel
  cube3, cube5  full boxes: the inner rows have all 27 taps
  isolated257   257 voxels on a pitch-3 lattice: every mask is the centre alone
  box_n         n voxels of a box at about one third occupancy; n around the 8-row groups of the transposing weight gradient, the 16-row
                quarters and 64-row tiles of the fused backward, the 256-row workgroups of the forward convolutions, and 257 / 1025 for
                several tiles per wave of the fused backward (fb_grid below)

ReLU ties: a float64 pre-activation below TIE has no defined side at fp32 resolution.  The forward cases with a ReLU redraw their weights
with the next seed, up to six times, until the float64 reference has none; tests/test_conv8_ref.py proves that every committed case finds
such a draw.  The backward masks are taken on matrices drawn here with exact zeros, so they have no ties.

Everything made here is cached and shared: do not modify what these functions return."""
import functools
import zlib

import numpy as np
import torch

from gpu_common import C_ROUND, _U, _within_rounding          # noqa: F401  (the criterion, re-exported)
from oracle import octree as ooct

TIE = 3e-7          # tests/gpu_common.py::_smallest_relu_input's threshold
DRAWS = 6

TAPS_ASC = tuple(range(27))
TAPS_LINR = tuple(k // 9 + 3 * ((k // 3) % 3) + 9 * (k % 3) for k in range(27))          # csrc/common.h: LINR_TAP
TILE8T_SPARE = 12                                                                           # csrc/common.h: LINR_TILE8T_SPARE

BOX_NS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025)
PAIR_CLOUDS = tuple('pair_%d' % k for k in range(27) if k != 13)
ENTRY_CLOUDS = tuple('box_%d' % n for n in BOX_NS) + ('cube3', 'cube5', 'single', 'isolated257')
ALL_CLOUDS = ENTRY_CLOUDS + PAIR_CLOUDS

FWD_SHAPES = ((8, 8), (8, 4), (4, 4)) + tuple((c, 8) for c in range(1, 8))
FWD_FORMS = ('none', 'relu', 'res', 'res_relu')
# (cin, cout, layout): 'out8' writes 4 channels into an 8-wide matrix, 'slice' reads channels 4..7 of an 8-wide matrix and writes 0..3 of another
FWD_LAYOUTS = tuple((ci, co, 'tight') for ci, co in FWD_SHAPES) + ((8, 4, 'out8'), (4, 4, 'slice'))
BWD_SHAPES = ((8, 8), (8, 4), (4, 4))
BWD_FORMS = ('none', 'accum', 'mask', 'accum_mask')
WGRAD_SHAPES = ((8, 8), (8, 4), (3, 8))
FUSED_NBLOCKS = (1, 2, 5, 256)
INC_NBLOCKS = (1, 3, 256)
OCC_NBLOCKS = (1, 3, 256)


# ---- clouds -------------------------------------------------------------------------------------------------------------------------------
def tap_delta(k):
    return np.array([k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1])


@functools.lru_cache(maxsize=None)
def cloud(key):
    """key in ALL_CLOUDS -> {'n', 'coord' int32 [n, 3] sorted, 'nbr' int64 [n, 27] (the oracle's neighbour table, -1 = absent)}."""
    kind, _, arg = key.partition('_')
    if kind == 'pair':
        c = np.stack([np.array([4, 4, 4]), np.array([4, 4, 4]) + tap_delta(int(arg))])
    elif key == 'single':
        c = np.array([[5, 3, 7]])
    elif key in ('cube3', 'cube5'):
        g = np.arange(int(key[4:])) + 2
        c = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    elif key == 'isolated257':
        g = 3 * np.arange(7)
        c = ooct.unique_sorted(np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3))[:257]
    else:
        n = int(arg)
        side = int(np.ceil((3.0 * n) ** (1.0 / 3.0))) + 1
        rng = np.random.default_rng(8800 + n)
        c = ooct.unique_sorted(rng.integers(0, side, size=(int(0.45 * side ** 3) + 1, 3)))
        assert len(c) >= n, (key, len(c))
        c = c[:n]
    c = ooct.unique_sorted(c)
    return {'n': len(c), 'coord': c, 'nbr': torch.from_numpy(ooct.neighbour_table(c)).long()}


def padded_ld(n):
    return (n + 63) // 64 * 64


# ---- the maps' other forms ------------------------------------------------------------------------------------------------------------------
def compress(nbr):
    """The compressed map of include/linr_hip.h from a table nbr int64 [n, 27]: (lo int64 [9, n], mask int64 [n]).  lo[q][j] = row of the first
    present neighbour of column q = (dx+1) + 3 (dy+1) (-1 here when the column is empty: the library's value there is not specified), bit
    3 q + (dz+1) of mask[j] = tap q + 9 (dz+1) present."""
    n = nbr.shape[0]
    lo = torch.full((9, n), -1, dtype=torch.int64)
    mask = torch.zeros(n, dtype=torch.int64)
    for q in range(9):
        for dz in (2, 1, 0):
            col = nbr[:, q + 9 * dz]
            lo[q] = torch.where(col >= 0, col, lo[q])
            mask |= (col >= 0).long() << (3 * q + dz)
    return lo, mask


def decode_cmap(lo, mask, ignore_b1=False):
    """(lo [9, ld], mask [ld]) -> the table [27, ld] they stand for: the dz = -1, 0, +1 neighbours of a column are consecutive rows from
    lo on.  ignore_b1: the mutant that reads the third tap at lo + b0."""
    dec = torch.full((27, lo.shape[1]), -1, dtype=lo.dtype, device=lo.device)
    for q in range(9):
        b0, b1, b2 = (mask >> (3 * q)) & 1, (mask >> (3 * q + 1)) & 1, (mask >> (3 * q + 2)) & 1
        dec[q] = torch.where(b0 == 1, lo[q], dec[q])
        dec[q + 9] = torch.where(b1 == 1, lo[q] + b0, dec[q + 9])
        dec[q + 18] = torch.where(b2 == 1, lo[q] + b0 + (0 if ignore_b1 else b1), dec[q + 18])
    return dec


def tile8t_ref(nbr_kl, n):
    """include/linr_hip.h's formula on a table nbr_kl int [27, ld] (numpy): tile8t[g][t][u][j] = nbr[tap(4 j + t)][8 g + u], -1 for position
    27, for j = 7, for rows past n and in the TILE8T_SPARE groups behind the last one.  int32 [(ceil(n / 8) + spare) * 256]."""
    groups = (n + 7) // 8 + TILE8T_SPARE
    out = np.full((groups, 4, 8, 8), -1, dtype=np.int32)
    for t in range(4):
        for j in range(7):
            p = 4 * j + t
            if p >= 27:
                continue
            for r in range(n):
                out[r // 8, t, r % 8, j] = nbr_kl[TAPS_LINR[p], r]
    return out.reshape(-1)


def fb_grid(n, nb, cus=256, waves=4):
    """csrc/fused_bwd.hip: (64-row tiles per wave, workgroups) of a fused backward launch over a slab of nb rows."""
    t64 = (n + 63) // 64
    target = max(1, min(cus, nb))
    m = max(1, -(-t64 // (waves * target)))
    return m, max(1, -(-t64 // (waves * m)))


# ---- the sums (linear in every operand; dtype and device follow the operands) -------------------------------------------------------------------
def gather(x, nbr):
    """[n, c] -> [n, 27, c]: the rows of the 27 taps, zeros where a neighbour is absent."""
    n, c = x.shape
    xp = torch.cat([x, x.new_zeros(1, c)], dim=0)
    return xp[torch.where(nbr < 0, torch.full_like(nbr, n), nbr)]


def conv_sum(x, nbr, W, b=None, order=None):
    """bias + sum_k x[nbr[k]] @ W[k]: one matrix product (order None), or tap after tap in `order` starting from the bias as the kernels do."""
    n, cin = x.shape
    cols = gather(x, nbr)
    if order is None:
        y = cols.reshape(n, 27 * cin) @ W.reshape(27 * cin, -1)
        return y if b is None else y + b.view(1, -1)
    y = x.new_zeros(n, W.shape[2]) if b is None else b.view(1, -1).expand(n, -1).clone()
    for k in order:
        y = y + cols[:, k] @ W[k]
    return y


def conv_t_sum(g, nbr, W, order=None, mirror=True):
    """sum_k g[nbr[26 - k]] @ W[k]^T (backward-data); mirror=False is the mutant that gathers tap k."""
    Wt = W.transpose(1, 2)
    return conv_sum(g, nbr, Wt.flip(0) if mirror else Wt, None, order)


def wgrad_sum(x, g, nbr, rows=None, bias_rows=None):
    """[gW (27 cin cout) | gb (cout)] flat, gW[k] = sum_j x[nbr[k][j]]^T g[j], gb = sum_j g[j]; rows / bias_rows: index tensors of the rows that
    take part (the mutants drop some)."""
    cols = gather(x, nbr).reshape(x.shape[0], -1)
    gw_rows = slice(None) if rows is None else rows
    gb_rows = gw_rows if bias_rows is None else bias_rows
    return torch.cat([(cols[gw_rows].t() @ g[gw_rows]).reshape(-1), g[gb_rows].sum(0)])


def _d(t):
    return None if t is None else t.double()


def _a(t):
    return None if t is None else t.double().abs()


# ---- float64 references: (exact, absum[, pre-activation]) -------------------------------------------------------------------------------------
def fwd_ref(x, nbr, W, b, res=None, relu=False):
    y, a = conv_sum(_d(x), nbr, _d(W), _d(b)), conv_sum(_a(x), nbr, _a(W), _a(b))
    if res is not None:
        y, a = y + _d(res), a + _a(res)
    return (torch.relu(y) if relu else y), a, y


def bwd_ref(g, nbr, W, old=None, act=None, extra=()):
    """(conv_t + extra terms + old) * (act > 0); extra: already formed float64 (value, absum) pairs of the sums added in front of the mask."""
    y, a = conv_t_sum(_d(g), nbr, _d(W)), conv_t_sum(_a(g), nbr, _a(W))
    for v, av in extra:
        y, a = y + v, a + av
    if old is not None:
        y, a = y + _d(old), a + _a(old)
    if act is not None:
        m = (act > 0).double()
        y, a = y * m, a * m
    return y, a


def wgrad_ref(x, g, nbr):
    return wgrad_sum(_d(x), _d(g), nbr), wgrad_sum(_a(x), _a(g), nbr)


def slab_ref(slab):
    """Sum of the slab rows: (float64 sum, sum of |slab|)."""
    return slab.double().sum(0), slab.double().abs().sum(0)


def inception_H_ref(x, nbr, w):
    y0, a0, _ = fwd_ref(x, nbr, w['w00'], w['b00'])
    y1 = _d(x) @ _d(w['w10']) + _d(w['b10']).view(1, -1)
    a1 = _a(x) @ _a(w['w10']) + _a(w['b10']).view(1, -1)
    pre = torch.cat([y0, y1], dim=1)
    return torch.relu(pre), torch.cat([a0, a1], dim=1), pre


def inception_M_ref(H, nbr, w):
    return fwd_ref(H[:, 4:8], nbr, w['w11'], w['b11'], relu=True)


def inception_I_ref(x, H, M, nbr, w):
    y0, a0, _ = fwd_ref(H[:, 0:4], nbr, w['w01'], w['b01'], res=x[:, 0:4])
    y1 = _d(M) @ _d(w['w12']) + _d(w['b12']).view(1, -1) + _d(x[:, 4:8])
    a1 = _a(M) @ _a(w['w12']) + _a(w['b12']).view(1, -1) + _a(x[:, 4:8])
    return torch.cat([y0, y1], dim=1), torch.cat([a0, a1], dim=1)


def inception_gM_ref(gI, M, w):
    m = (M > 0).double()
    return (_d(gI[:, 4:8]) @ _d(w['w12']).t()) * m, (_a(gI[:, 4:8]) @ _a(w['w12']).t()) * m


def inception_gH_ref(gI, gM, H, nbr, w):
    y0, a0 = bwd_ref(gI[:, 0:4], nbr, w['w01'], act=H[:, 0:4])
    y1, a1 = bwd_ref(gM, nbr, w['w11'], act=H[:, 4:8])
    return torch.cat([y0, y1], dim=1), torch.cat([a0, a1], dim=1)


def inception_gX_ref(gI, gH, x, nbr, w, old=None, mask=False):
    side = (_d(gH[:, 4:8]) @ _d(w['w10']).t() + _d(gI), _a(gH[:, 4:8]) @ _a(w['w10']).t() + _a(gI))
    return bwd_ref(gH[:, 0:4], nbr, w['w00'], old=old, act=x if mask else None, extra=(side,))


def inception_slab_ref(gI, gM, gH, x, H, nbr):
    """[W00 864 | b00 4 | W01 432 | b01 4 | W11 432 | b11 4 | W10 32 | b10 4] of linr_inception_bwd_fused: (exact, absum)."""
    out = []
    for f in (_d, _a):
        gh1 = f(gH[:, 4:8])
        out.append(torch.cat([wgrad_sum(f(x), f(gH[:, 0:4]), nbr), wgrad_sum(f(H[:, 0:4]), f(gI[:, 0:4]), nbr),
                              wgrad_sum(f(H[:, 4:8]), f(gM), nbr), (f(x).t() @ gh1).reshape(-1), gh1.sum(0)]))
    return out[0], out[1]


def dual44_ref(H, g0, g1, nbr):
    """[gW01 432 | gb01 4 | gW11 432 | gb11 4] of linr_spconv_wgrad_dual44."""
    e0, a0 = wgrad_ref(H[:, 0:4], g0, nbr)
    e1, a1 = wgrad_ref(H[:, 4:8], g1, nbr)
    return torch.cat([e0, e1]), torch.cat([a0, a1])


def occ_wgrad7_ref(occ, gouts, nbr):
    """for b = 1..7: kernel [27][b][8] then bias [8] (6104 elements)."""
    parts = [wgrad_ref(occ[:, :b], gouts[b - 1], nbr) for b in range(1, 8)]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------
def _gen(*what):
    return torch.Generator().manual_seed(zlib.crc32(repr(what).encode()))


def _relu_zeros(gen, n, c):
    """A ReLU output: about half of its entries are exact zeros."""
    return torch.relu(torch.randn(n, c, generator=gen))


def _tie_free(pres):
    return all(p.numel() == 0 or float(p.abs().min()) >= TIE for p in pres)


@functools.lru_cache(maxsize=None)
def fwd_case(key, cin, cout):
    """x [n, cin], res [n, cout] and, redrawn until neither ReLU form ('relu', 'res_relu') has a tie, W [27, cin, cout], b [cout];
    'other' [n, 4]: what the channels of an 8-wide matrix hold that a 4-channel slice does not name."""
    c = cloud(key)
    gen = _gen('fwd', key, cin, cout)
    t = {'x': torch.randn(c['n'], cin, generator=gen), 'res': torch.randn(c['n'], cout, generator=gen),
         'other': torch.randn(c['n'], 4, generator=gen)}
    for attempt in range(DRAWS):
        gw = _gen('fwd-w', key, cin, cout, attempt)
        t['W'], t['b'] = torch.randn(27, cin, cout, generator=gw) * 0.2, torch.randn(cout, generator=gw) * 0.1
        if _tie_free([fwd_ref(t['x'], c['nbr'], t['W'], t['b'])[2], fwd_ref(t['x'], c['nbr'], t['W'], t['b'], res=t['res'])[2]]):
            t['attempt'] = attempt
            return t
    raise AssertionError('forward %d -> %d on %s: %d draws in a row with a pre-activation below %.0e' % (cin, cout, key, DRAWS, TIE))


@functools.lru_cache(maxsize=None)
def bwd_case(key, cin, cout):
    """g [n, cout] (the gathered output gradient), W, old [n, cin], act [n, cin] with exact zeros."""
    n = cloud(key)['n']
    gen = _gen('bwd', key, cin, cout)
    return {'g': torch.randn(n, cout, generator=gen), 'W': torch.randn(27, cin, cout, generator=gen) * 0.2,
            'old': torch.randn(n, cin, generator=gen), 'act': _relu_zeros(gen, n, cin)}


@functools.lru_cache(maxsize=None)
def wgrad_case(key, cin, cout):
    n = cloud(key)['n']
    gen = _gen('wgrad', key, cin, cout)
    return {'x': torch.randn(n, cin, generator=gen), 'g': torch.randn(n, cout, generator=gen)}


@functools.lru_cache(maxsize=None)
def fused_case(key):
    """linr_spconv_bwd_fused: g (gathered), x (the convolution's input), W [27, 8, 8]."""
    n = cloud(key)['n']
    gen = _gen('fused', key)
    return {'g': torch.randn(n, 8, generator=gen), 'x': torch.randn(n, 8, generator=gen), 'W': torch.randn(27, 8, 8, generator=gen) * 0.2}


INC_SHAPES = {'w00': (27, 8, 4), 'b00': (4,), 'w01': (27, 4, 4), 'b01': (4,), 'w10': (8, 4), 'b10': (4,), 'w11': (27, 4, 4), 'b11': (4,),
              'w12': (4, 4), 'b12': (4,)}


def _inc_weights(gen):
    return {k: torch.randn(*s, generator=gen) * (0.2 if k[0] == 'w' else 0.1) for k, s in INC_SHAPES.items()}


@functools.lru_cache(maxsize=None)
def inception_case(key):
    """Forward: x (a ReLU output, as in make_block) and the ten weights, redrawn until H and M have no tie.  Backward (its masks are
    taken on matrices with exact zeros, drawn here, not on the forward's outputs): Hb [n, 8], Mb [n, 4], gI [n, 8], old [n, 8]."""
    c = cloud(key)
    n, nbr = c['n'], c['nbr']
    gen = _gen('inception', key)
    t = {'x': _relu_zeros(gen, n, 8), 'Hb': _relu_zeros(gen, n, 8), 'Mb': _relu_zeros(gen, n, 4), 'gI': torch.randn(n, 8, generator=gen),
         'old': torch.randn(n, 8, generator=gen)}
    for attempt in range(DRAWS):
        t['w'] = _inc_weights(_gen('inception-w', key, attempt))
        H, _, preH = inception_H_ref(t['x'], nbr, t['w'])
        if _tie_free([preH, inception_M_ref(H, nbr, t['w'])[2]]):
            t['attempt'] = attempt
            return t
    raise AssertionError('inception forward on %s: %d draws in a row with a pre-activation below %.0e' % (key, DRAWS, TIE))


@functools.lru_cache(maxsize=None)
def occ_case(key):
    """occ [n, 8] of 0 / 1, the seven gradients [n, 8] and, redrawn until none of the seven outputs has a tie, the kernels [27][g + 1][8]
    and biases [8] of linr_occ_conv7."""
    c = cloud(key)
    n, nbr = c['n'], c['nbr']
    gen = _gen('occ', key)
    t = {'occ': (torch.rand(n, 8, generator=gen) < 0.5).float(), 'gouts': [torch.randn(n, 8, generator=gen) for _ in range(7)]}
    for attempt in range(DRAWS):
        gw = _gen('occ-w', key, attempt)
        t['ws'] = [torch.randn(27, g + 1, 8, generator=gw) * 0.3 for g in range(7)]
        t['bs'] = [torch.randn(8, generator=gw) * 0.1 for g in range(7)]
        if _tie_free([fwd_ref(t['occ'][:, :g + 1], nbr, t['ws'][g], t['bs'][g])[2] for g in range(7)]):
            t['attempt'] = attempt
            return t
    raise AssertionError('occ_conv7 on %s: %d draws in a row with a pre-activation below %.0e' % (key, DRAWS, TIE))


def occ_params(t, base=5):
    """The seven kernels and biases as one flat buffer that starts at a non-zero base offset: (params, w_off, b_off)."""
    w_off, b_off, cur, chunks = [], [], base, [torch.zeros(base)]
    for g in range(7):
        w_off.append(cur); chunks.append(t['ws'][g].reshape(-1)); cur += t['ws'][g].numel()
        b_off.append(cur); chunks.append(t['bs'][g]); cur += 8
    return torch.cat(chunks), w_off, b_off


# ---- fp32 emulations, with mutants (tests/test_conv8_ref.py: the criterion tells right from wrong) ------------------------------------------------
MUTANTS = ('taps_swapped', 'bwd_not_mirrored', 'third_tap_ignores_b1', 'wgrad_last_group_dropped', 'wgrad_wave_tile_dropped',
           'bias_grad_short', 'accum_ignored', 'mask_on_wrong_matrix')


def _table(key, mut):
    """The table the emulation gathers with: what the compressed map decodes to (the mutant decodes it wrongly)."""
    nbr = cloud(key)['nbr']
    lo, mask = compress(nbr)
    dec = decode_cmap(lo, mask, ignore_b1=mut == 'third_tap_ignores_b1').t().contiguous()
    assert mut == 'third_tap_ignores_b1' or torch.equal(dec, nbr)
    return dec


def emu_fwd(key, cin, cout, form, order, mut=None):
    t = fwd_case(key, cin, cout)
    W = t['W'].clone()
    if mut == 'taps_swapped':
        W[[3, 17]] = W[[17, 3]]
    y = conv_sum(t['x'], _table(key, mut), W, t['b'], order)
    if 'res' in form:
        y = y + t['res']
    return torch.relu(y) if 'relu' in form else y


def emu_bwd(key, cin, cout, form, order, mut=None):
    t = bwd_case(key, cin, cout)
    y = conv_t_sum(t['g'], _table(key, mut), t['W'], order, mirror=mut != 'bwd_not_mirrored')
    if 'accum' in form and mut != 'accum_ignored':
        y = y + t['old']
    if 'mask' in form:
        y = y * ((t['old'] if mut == 'mask_on_wrong_matrix' else t['act']) > 0).float()
    return y


def emu_wgrad(key, cin, cout, mut=None, nblocks=1):
    """Row by row in fp32 (groups of 8 rows summed first, as the transposing kernel walks them)."""
    t, n = wgrad_case(key, cin, cout), cloud(key)['n']
    rows = torch.arange(n)
    bias_rows = None
    if mut == 'wgrad_last_group_dropped':
        rows = rows[:(n - 1) // 8 * 8]
    if mut == 'wgrad_wave_tile_dropped':          # the last tile of wave 0 of block 0
        tpw, _ = fb_grid(n, nblocks)
        rows = torch.cat([rows[:64 * (tpw - 1)], rows[64 * tpw:]])
    if mut == 'bias_grad_short':
        bias_rows = rows[:n - 1]
    tab = _table(key, mut)
    tot = torch.zeros((27 * cin + 1) * cout)
    for a in range(0, n, 8):
        grp = rows[(rows >= a) & (rows < a + 8)]
        bgrp = grp if bias_rows is None else bias_rows[(bias_rows >= a) & (bias_rows < a + 8)]
        tot = tot + wgrad_sum(t['x'], t['g'], tab, grp, bgrp)
    return tot


def emu_inception_fwd(key, order):
    t, nbr = inception_case(key), _table(key, None)
    w, x = t['w'], t['x']
    H = torch.relu(torch.cat([conv_sum(x, nbr, w['w00'], w['b00'], order), x @ w['w10'] + w['b10']], dim=1))
    M = torch.relu(conv_sum(H[:, 4:8].contiguous(), nbr, w['w11'], w['b11'], order))
    I = torch.cat([conv_sum(H[:, 0:4].contiguous(), nbr, w['w01'], w['b01'], order), M @ w['w12'] + w['b12']], dim=1) + x
    return H, M, I


def emu_inception_bwd(key, order, flags):
    """gM, gH, gX of linr_inception_bwd_data in fp32; flags: 0 or LINR_RELU_MASK | LINR_ACCUM (6)."""
    t, nbr = inception_case(key), _table(key, None)
    w, x, H, M, gI = t['w'], t['x'], t['Hb'], t['Mb'], t['gI']
    gM = (gI[:, 4:8] @ w['w12'].t()) * (M > 0).float()
    gH = torch.cat([conv_t_sum(gI[:, 0:4].contiguous(), nbr, w['w01'], order), conv_t_sum(gM, nbr, w['w11'], order)], dim=1) * (H > 0).float()
    gX = conv_t_sum(gH[:, 0:4].contiguous(), nbr, w['w00'], order) + gI
    if flags:
        gX = gX + t['old']
    gX = gX + gH[:, 4:8] @ w['w10'].t()
    if flags:
        gX = gX * (x > 0).float()
    return gM, gH, gX


def emu_occ_conv7(key, order):
    t, nbr = occ_case(key), _table(key, None)
    return [torch.relu(conv_sum(t['occ'][:, :g + 1].contiguous(), nbr, t['ws'][g], t['bs'][g], order)) for g in range(7)]
