"""Op-level reference of the wide bf16 / uint8-weight inference executor (csrc/wide_bf16.hip): the inputs of every case that
tests/test_gpu_wide_bf16_ops.py runs, the float64 value of every fp32 sum the kernels form, and - because every output is STORED as bf16 -
the interval of bf16 values a correct kernel can store.  tests/test_wide_bf16_ops_ref.py checks this file on the CPU (no kernel).

The criterion.  The operands are exact: inputs are bf16 values, a 3x3x3 kernel is rb(de-quantised weight), biases and the pointwise / head
/ scale-context weights are the de-quantised fp32 values.  So the float64 sum y is what exact arithmetic would give, and the kernel's fp32
value v satisfies |v - y| <= eps = C_ROUND 2^-24 a, a = the same sum over the absolute values of its terms (tests/gpu_common.py).  ReLU, an
fp32 add and the rounding to bf16 are monotone, so with f = the entry's own chain of such steps the stored value lies in
[f(y - eps), f(y + eps)].  Where both ends are the same bf16 value the stored bits are determined; the other entries are AMBIGUOUS
(AMBIGUOUS_CAP of a case's entries at most - a case above it gets other inputs, not a higher cap).  Values are compared as numbers: +0 and
-0 count as the same stored value.

rb64 rounds a float64 to bf16 (RNE) by integer arithmetic on its bits - no float32 in between, so no double rounding narrows an interval.

The chains (WE_* of csrc/wide_bf16.hip):
  WE_PLAIN  y = conv + bias (+ res, its stored bf16 value);  f(v) = rb(relu?(v));  with the extra skip res2: f(v) = rb(fl32(rb(v) + r2))
  WE_PW1    blocks 0 .. CO/8 - 1: rb(relu(conv0_0));  blocks CO/8 ..: rb(relu(b10 + x_row . W10)) on the row's own input
  WE_PW2    M in [rb(relu(y11 - eps)), rb(relu(y11 + eps))] = [m_lo, m_hi]; carried through conv1_2 as centre m_c and radius m_r:
            o = m_c . W12 + b12 + x_hi,  bound = C_ROUND 2^-24 (m_hi . |W12| + |b12| + |x_hi|) + m_r . |W12|;  stored in
            [rb(o - bound), rb(o + bound)], then the res2 chain.  An ambiguous M widens the interval, it excludes no row.
  scale context  hid in [relu(hpre - eps_h), relu(hpre + eps_h)] (fp32, never stored), carried through the second layer the same way
  head      c (the prune convolution, never rounded) -> z64 = head_ref.head_logits in float64;  the logit recovered from the stored fp32 p
            within 1e-4 + 1e-4 |z64| where |z64| < 12, p within 1e-6 of head_ref.sigmoid32(z64) elsewhere;  partial[b] within 1e-5
            relative of the float64 sum over block b's live rows of head_ref.nats(p_stored, t)

The inputs: clouds of n in NS voxels of a box at about half occupancy (tests/test_gpu_multi_tile.py::occ7_inputs' draw) and the full
6 x 6 x 6 cube; ONE flat uint8 code buffer (`bank()`) that holds every layer of LAYERS, de-quantised with QRANGE; bf16 inputs N(0, 1).
Everything here is made on the CPU, cached and shared: do not modify what these functions return."""
import functools

import numpy as np
import torch

import head_ref
from gpu_common import C_ROUND, _U
from oracle import network as onet
from oracle import octree as ooct

NS = (1, 2, 63, 64, 65, 255, 256, 257, 1025)
CLOUDS = NS + ('cube6',)
QRANGE = (-0.31, 0.27)
AMBIGUOUS_CAP = 0.10
TAP_SHARE = 0.15          # for n >= 257: every one of the 27 taps present in at least this share of the rows
WE_PLAIN, WE_PW1, WE_PW2, WE_HEAD = 0, 1, 2, 3
_EPI_NAME = {WE_PLAIN: 'WE_PLAIN', WE_PW1: 'WE_PW1', WE_PW2: 'WE_PW2', WE_HEAD: 'WE_HEAD'}

# one layer per instantiation of wdispatch: (epilogue, cin, cout); NBI = ceil(cin / 8).  3 -> 8 and 7 -> 16 have 27 * nc = 108 / 216
# combos, no multiple of 16 (a zero-filled tail in the image); cin = 3, 7, 13, 29 leave pad channels in the last input block.
# (WE_PLAIN, 2, 8), (2, 32) and (4, 16) are the three instantiations no network schedule launches.
LAYERS = [(WE_PLAIN, 3, 8), (WE_PLAIN, 7, 16), (WE_PLAIN, 8, 32), (WE_PLAIN, 16, 16), (WE_PLAIN, 32, 32),
          (WE_PLAIN, 16, 8), (WE_PLAIN, 13, 32), (WE_PLAIN, 29, 16),
          (WE_PW1, 16, 8), (WE_PW1, 32, 16), (WE_PW2, 8, 8), (WE_PW2, 16, 16), (WE_HEAD, 16, 16), (WE_HEAD, 32, 32)]
PLAIN_FORMS = ('bare', 'res_relu', 'res2', 'res_relu_res2')
PW_FORMS = ('bare', 'res2')


def layer_id(layer):
    epi, cin, co = layer
    return '%s-%d-%d' % (_EPI_NAME[epi], (cin + 7) // 8, co)


def forms_of(layer):
    return PLAIN_FORMS if layer[0] == WE_PLAIN else PW_FORMS


# ---- bf16 ---------------------------------------------------------------------------------------------------------------------------------
_MAG = 0x7FFFFFFFFFFFFFFF
_BF16_MAX = float.fromhex('0x1.fep127')
_BF16_MIN_NORMAL = 2.0 ** -126


def rb64(v):
    """float64 -> the nearest bf16 value (ties to even), as float64.  bf16 keeps 7 of the 52 fraction bits: add half of the dropped 45
    (one less on an even kept part) to the magnitude's bit pattern and clear them - a carry walks into the exponent by itself.  Below
    2^-126 the spacing is fixed at 2^-133; above the largest bf16 the result is +-inf; NaN stays NaN."""
    v = v.to(torch.float64).contiguous()
    bits = v.view(torch.int64)
    mag = bits & _MAG
    sign = bits ^ mag
    r = mag + ((1 << 44) - 1) + ((mag >> 45) & 1)
    r = r & ~((1 << 45) - 1)
    out = (r | sign).view(torch.float64)
    out = torch.where(out.abs() > _BF16_MAX, torch.copysign(torch.full_like(out, float('inf')), v), out)
    sub = torch.round(v * 2.0 ** 133) * 2.0 ** -133                 # torch.round: halves to even; the scaling is exact
    out = torch.where(v.abs() < _BF16_MIN_NORMAL, sub, out)
    return torch.where(torch.isnan(v), v, out)


def rb32(t):
    """fp32 -> bf16 -> fp32 as torch (and v_cvt_pk_bf16_f32) rounds: RNE."""
    return t.to(torch.bfloat16).to(torch.float32)


def trunc32(t):
    """fp32 -> bf16 by dropping the low 16 bits: the wrong rounding, for the mutants of tests/test_wide_bf16_ops_ref.py."""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def fl32(v):
    """float64 -> fp32 (RNE) -> float64: the fp32 add of two bf16 values, whose float64 sum is exact."""
    return v.to(torch.float32).to(torch.float64)


# ---- clouds -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cloud(key):
    """key in CLOUDS -> {'n', 'coord' int32 [n, 3] sorted, 'nbr' int64 [n, 27] (the oracle's neighbour table, -1 = absent)}."""
    if key == 'cube6':
        g = np.arange(6)
        c = ooct.unique_sorted(np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3))
    else:
        side = int(np.ceil((2.0 * key) ** (1.0 / 3.0))) + 1
        rng = np.random.default_rng(4200 + key)
        c = ooct.unique_sorted(rng.integers(0, side, size=(int(0.8 * side ** 3), 3)))[:key]
        assert len(c) == key
    return {'n': len(c), 'coord': c, 'nbr': torch.from_numpy(ooct.neighbour_table(c)).long()}


def tap_shares(key):
    """Per tap, the share of the cloud's rows that have it."""
    return (cloud(key)['nbr'] >= 0).double().mean(0)


# ---- the parameter bank ---------------------------------------------------------------------------------------------------------------------
def image_elems(cin, co):
    """uint2 elements of a convolution's A-operand image (linr_wide_bf16_image_elems)."""
    nc = 2 * ((cin + 7) // 8) * (co // 4)
    return (27 * nc + 15) // 16 * 64


def dequant32(codes):
    """w = q / 255 * range + min, every step one fp32 operation, range an fp32 subtraction (quant_uniform2's reconstruction;
    tests/test_gpu_bf16.py::test_dequantisation_is_bit_exact)."""
    lo, hi = torch.tensor(QRANGE[0], dtype=torch.float32), torch.tensor(QRANGE[1], dtype=torch.float32)
    rng = hi - lo
    return codes.to(torch.float32) / 255.0 * rng + lo


@functools.lru_cache(maxsize=None)
def bank():
    """The flat code buffer of every layer: {'codes' uint8 [P], 'pf' fp32 [P] = dequant32(codes), 'off': {(layer, name): (offset, shape)},
    'convs': [(kernel offset, cin, co, image offset)] in LAYERS order, 'n_img'}.  A layer's tensors: 'kernel' [27][cin][co], 'bias' [co];
    WE_PW1 'pw_w' [cin][co], 'pw_b' [co]; WE_PW2 'pw_w' [co][co], 'pw_b' [co]; WE_HEAD 'w1' [24][C], 'b1' [24], 'w2' [24], 'b2' [1].
    Eight codes lead the buffer, so that no kernel starts at offset 0."""
    off, cur, convs, img = {}, 8, [], 0
    for layer in LAYERS:
        epi, cin, co = layer
        shapes = [('kernel', (27, cin, co)), ('bias', (co,))]
        if epi == WE_PW1:
            shapes += [('pw_w', (cin, co)), ('pw_b', (co,))]
        elif epi == WE_PW2:
            shapes += [('pw_w', (co, co)), ('pw_b', (co,))]
        elif epi == WE_HEAD:
            shapes += [('w1', (24, co)), ('b1', (24,)), ('w2', (24,)), ('b2', (1,))]
        for name, shape in shapes:
            off[(layer, name)] = (cur, shape)
            if name == 'kernel':
                convs.append((cur, cin, co, img))
                img += image_elems(cin, co)
            cur += int(np.prod(shape))
    codes = torch.from_numpy(np.random.default_rng(20260).integers(0, 256, size=cur, dtype=np.uint8))
    assert sum(1 for c in convs if (27 * 2 * ((c[1] + 7) // 8) * (c[2] // 4)) % 16) >= 1          # a zero-filled tail exists
    return {'codes': codes, 'pf': dequant32(codes), 'off': off, 'convs': convs, 'n_img': img}


def param(layer, name, pf=None):
    """A layer's tensor as a view of pf (default: the bank's own fp32 copy)."""
    b = bank()
    o, shape = b['off'][(layer, name)]
    return (b['pf'] if pf is None else pf)[o:o + int(np.prod(shape))].view(shape)


# ---- a case: inputs, exact sums, intervals ------------------------------------------------------------------------------------------------------
def _seed(layer, key):
    return 100000 * (LAYERS.index(layer) + 1) + (6 if key == 'cube6' else key)


def _draw(layer, key, attempt):
    epi, cin, co = layer
    n = cloud(key)['n']
    gen = torch.Generator().manual_seed(_seed(layer, key) + 1000 * attempt)
    t = {'x': rb32(torch.randn(n, cin, generator=gen)), 'res': rb32(torch.randn(n, co, generator=gen)),
         'res2': rb32(torch.randn(n, co, generator=gen)), 'x_hi': rb32(torch.randn(n, co, generator=gen))}
    if epi == WE_HEAD:
        t['target'] = (torch.rand(n, 8, generator=gen) < 0.5).float()
    return t


@functools.lru_cache(maxsize=None)
def inputs(layer, key):
    """bf16-valued fp32 inputs of a layer on a cloud: x [n, cin], res / res2 [n, co], WE_PW2 also x_hi [n, co]; WE_HEAD a random 0 / 1
    target [n, 8].  A draw that puts more than AMBIGUOUS_CAP of a form's entries next to a rounding boundary (at n = 1 one entry of 8 is
    12.5 %) is replaced by the next one - decided by the float64 reference alone; eight such draws in a row are an error."""
    if layer[0] == WE_HEAD:
        return _draw(layer, key, 0)
    for attempt in range(8):
        t = _draw(layer, key, attempt)
        if all(ambiguous_share(_intervals(layer, key, form, t)) <= AMBIGUOUS_CAP for form in forms_of(layer)):
            return t
    raise AssertionError('no draw of %s on cloud %s under the ambiguity cap' % (layer_id(layer), key))


def conv64(layer, key, x):
    """(y, a): the float64 convolution conv + bias of the exact operands and the same sum over absolute values."""
    nbr = cloud(key)['nbr']
    x = x.double()
    W, b = rb32(param(layer, 'kernel')).double(), param(layer, 'bias').double().view(1, -1)
    return onet.conv3(x, nbr, W, b), onet.conv3(x.abs(), nbr, W.abs(), b.abs())


def _res2_chain(lo, hi, r2):
    return rb64(fl32(lo + r2)), rb64(fl32(hi + r2))


@functools.lru_cache(maxsize=None)
def intervals(layer, key, form):
    """{'lo', 'hi' (float64 bf16 values, [n, width]), 'nom' (the chain applied to the exact sum itself); without res2 also 'pre', 'eps'
    (nom before its rounding to bf16, and the bound of the last fp32 sum)} of a convolution entry; 'stat': None, or for WE_PW2 the entries
    of the rows whose whole M is determined (elsewhere nom is the image of an M between two bf16 values: nothing a kernel can store).
    WE_PW1's width is 2 co: [conv0_0 | conv1_0]; its extra skip reaches the first half only (the second is stored in front of it)."""
    return _intervals(layer, key, form, inputs(layer, key))


def _intervals(layer, key, form, t):
    epi, cin, co = layer
    cu = C_ROUND * _U
    stat = None
    y, a = conv64(layer, key, t['x'])
    if epi == WE_PLAIN:
        relu = form in ('res_relu', 'res_relu_res2')
        if relu:
            y, a = y + t['res'].double(), a + t['res'].double().abs()
        eps = cu * a
        lo, hi = y - eps, y + eps
        nom = y
        if relu:
            lo, hi, nom = torch.relu(lo), torch.relu(hi), torch.relu(y)
    elif epi == WE_PW1:
        x, W10, b10 = t['x'].double(), param(layer, 'pw_w').double(), param(layer, 'pw_b').double()
        y = torch.cat([y, x @ W10 + b10], dim=1)
        a = torch.cat([a, x.abs() @ W10.abs() + b10.abs()], dim=1)
        eps = cu * a
        lo, hi, nom = torch.relu(y - eps), torch.relu(y + eps), torch.relu(y)
    else:
        W12, b12, xh = param(layer, 'pw_w').double(), param(layer, 'pw_b').double(), t['x_hi'].double()
        e11 = cu * a
        m_lo, m_hi = rb64(torch.relu(y - e11)), rb64(torch.relu(y + e11))
        m_c, m_r = (m_lo + m_hi) / 2, (m_hi - m_lo) / 2
        y = m_c @ W12 + b12 + xh          # m_c is rb(relu(y11)) wherever M is determined
        nom, stat = y, (m_r == 0).all(dim=1, keepdim=True).expand_as(y)
        eps = cu * (m_hi @ W12.abs() + b12.abs() + xh.abs()) + m_r @ W12.abs()
        lo, hi = y - eps, y + eps
    pre = nom
    lo, hi, nom = rb64(lo), rb64(hi), rb64(nom)
    if form in ('res2', 'res_relu_res2'):
        l2, h2 = _res2_chain(lo[:, :co], hi[:, :co], t['res2'].double())
        lo, hi = torch.cat([l2, lo[:, co:]], dim=1), torch.cat([h2, hi[:, co:]], dim=1)
        nom = torch.cat([_res2_chain(nom[:, :co], nom[:, :co], t['res2'].double())[0], nom[:, co:]], dim=1)
        return {'lo': lo, 'hi': hi, 'nom': nom, 'stat': stat}
    return {'lo': lo, 'hi': hi, 'nom': nom, 'stat': stat, 'pre': pre, 'eps': eps}


def ambiguous_share(iv):
    return float((iv['lo'] != iv['hi']).double().mean())


def check_interval(got, iv, what):
    """Every entry of `got` (the stored values, any float type) inside its interval; returns (ambiguous share, share of the entries whose
    stored value is not iv['nom'], worst visible error / eps) - the last two are printed, not asserted.  |got - y| itself holds the
    store's own rounding (2^-9 |y| against eps ~ 2^-18 a), so the error of the kernel's fp32 value shows only where it moved the stored
    value off nom: there it is at least the distance from the exact value to the rounding boundary between nom and got,
    |(nom + got) / 2 - pre|, and that distance is what the ratio reports (0 where got == nom; NaN for the res2 chains, whose second
    rounding has no single boundary).  Both figures leave out the entries outside iv['stat']."""
    got = got.detach().double().cpu()
    assert got.shape == iv['lo'].shape, (what, got.shape, iv['lo'].shape)
    assert bool(torch.isfinite(got).all()), '%s: %d entries never written (NaN)' % (what, int((~torch.isfinite(got)).sum()))
    bad = (got < iv['lo']) | (got > iv['hi'])
    if bool(bad.any()):
        i = torch.nonzero(bad)[0].tolist()
        amb = iv['lo'] != iv['hi']
        raise AssertionError('%s: %d of %d entries outside their interval (%d of them where the bits are determined); first at %s: got '
                             '%r, interval [%r, %r]' % (what, int(bad.sum()), bad.numel(), int((bad & ~amb).sum()), i,
                                                        float(got[tuple(i)]), float(iv['lo'][tuple(i)]), float(iv['hi'][tuple(i)])))
    moved = got != iv['nom']
    if iv.get('stat') is not None:
        moved = moved & iv['stat']
    ratio = float('nan')
    if 'pre' in iv:
        need = ((iv['nom'] + got) / 2 - iv['pre']).abs() / iv['eps'].clamp(min=1e-300)
        ratio = float(torch.where(moved, need, torch.zeros_like(need)).max())
    return ambiguous_share(iv), float(moved.double().mean()), ratio


# ---- head ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def head64(layer, key):
    """{'c' (float64 prune convolution, never rounded), 'z64'} of a WE_HEAD layer."""
    c, _ = conv64(layer, key, inputs(layer, key)['x'])
    z = head_ref.head_logits(c, param(layer, 'w1').double(), param(layer, 'b1').double(), param(layer, 'w2').double(),
                             param(layer, 'b2').double())
    return {'c': c, 'z64': z}


def check_head_p(p, layer, key, what):
    """The stored fp32 probabilities against z64; returns the worst logit error as a share of its tolerance."""
    p = p.detach().cpu()
    assert p.dtype == torch.float32 and bool(torch.isfinite(p).all()), '%s: p never written' % what
    z64 = head64(layer, key)['z64']
    mid = z64.abs() < 12
    pd = p.double()
    z = torch.log(pd) - torch.log1p(-pd)
    ratio = ((z - z64).abs() / (1e-4 + 1e-4 * z64.abs()))[mid]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    assert worst <= 1.0, '%s: a logit at %.3g x its tolerance 1e-4 + 1e-4 |z|' % (what, worst)
    far = (pd - head_ref.sigmoid32(z64).double()).abs()[~mid]
    assert far.numel() == 0 or float(far.max()) <= 1e-6, '%s: a saturated p off by %.3g' % (what, float(far.max()))
    return worst


def partial64(p, t_col_values):
    """float64 sums over each 256-row block's live rows of head_ref.nats(p_stored, t): [ceil(n / 256)]."""
    nats = head_ref.nats(p.detach().cpu(), t_col_values)
    n = nats.shape[0]
    nb = (n + 255) // 256
    padded = torch.zeros(nb * 256, dtype=torch.float64)
    padded[:n] = nats
    return padded.view(nb, 256).sum(1)


def check_partial(partial, p, t_col_values, what):
    ref = partial64(p, t_col_values)
    got = partial.detach().double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), '%s: partial never written' % what
    rel = float(((got - ref).abs() / ref.abs().clamp(min=1e-300)).max())
    assert rel <= 1e-5, '%s: a block partial off by %.3g relative' % (what, rel)
    return rel


# ---- scale context ----------------------------------------------------------------------------------------------------------------------------------
def sce_intervals(ref):
    """tests/sce_ref.py::reference's float64 result -> the interval of the stored bf16 x0.  hid = relu(hpre) stays fp32 in the kernel:
    within eps_h = C_ROUND 2^-24 hid_abs of it it lies in [relu(hid - eps_h), hid + eps_h] (for hpre < 0 that is wider than
    [0, relu(hpre + eps_h)], never narrower); the second layer then carries centre and radius like WE_PW2 carries M.  Needs the W2, b2 rows
    of every row: ref['W2'] [R, 8, 16], ref['b2'] [R, 8] (sce_case adds them)."""
    cu = C_ROUND * _U
    e_h = cu * ref['hid_abs']
    h_lo, h_hi = torch.relu(ref['hid'] - e_h), ref['hid'] + e_h
    h_c, h_r = (h_lo + h_hi) / 2, (h_hi - h_lo) / 2
    W2, b2 = ref['W2'], ref['b2']
    y = torch.einsum('rk,rok->ro', h_c, W2) + b2
    eps = cu * (torch.einsum('rk,rok->ro', h_hi, W2.abs()) + b2.abs()) + torch.einsum('rk,rok->ro', h_r, W2.abs())
    pre = torch.einsum('rk,rok->ro', ref['hid'], W2) + b2
    return {'lo': rb64(y - eps), 'hi': rb64(y + eps), 'nom': rb64(pre), 'pre': pre, 'eps': eps}


SCE_CASES = {'257-0-65': (3, ((0, 257), (1, 0), (2, 65))), '1': (2, ((1, 1),))}


@functools.lru_cache(maxsize=None)
def sce_case(name):
    """{'S', 'row_off', 'sidx', 'off' fp32 [R, 7], 'flat' fp32 parameters, 'iv'} of a scale-context frame (tests/sce_ref.py).  The
    parameters are redrawn while more than AMBIGUOUS_CAP of the entries are ambiguous (one row has 8 entries), as inputs() does."""
    import sce_ref as sr
    S, ranges = SCE_CASES[name]
    row_off, sidx, off, _ = sr.draw_frame(list(ranges), 31 + len(ranges))
    R = int(row_off[-1])
    for attempt in range(8):
        flat = sr.draw_params(S, 57 + len(ranges) + 1000 * attempt)
        ref = sr.reference(flat, S, row_off, sidx, off)
        p = sr.unpack(flat.double(), S)
        ref['W2'], ref['b2'] = torch.zeros(R, 8, 16, dtype=torch.float64), torch.zeros(R, 8, dtype=torch.float64)
        for j, si in enumerate(int(s) for s in sidx):
            a, b = int(row_off[j]), int(row_off[j + 1])
            ref['W2'][a:b], ref['b2'][a:b] = p[si][2], p[si][3]
        iv = sce_intervals(ref)
        if ambiguous_share(iv) <= AMBIGUOUS_CAP:
            return {'S': S, 'row_off': row_off, 'sidx': sidx, 'off': off, 'flat': flat, 'iv': iv}
    raise AssertionError('no draw of the scale context %s under the ambiguity cap' % name)


# ---- fp32 emulations of the chains, with mutants (tests/test_wide_bf16_ops_ref.py: the criterion has teeth) --------------------------------------
MUTANTS = ('truncate_store', 'm_unrounded', 'res2_before_rounding', 'head_rounded_c', 'taps_swapped', 'quad_zeroed', 'pad_not_ignored',
           'dead_lane_counted')


def _emu_conv(layer, key, mut):
    """fp32 conv + bias in torch (its own summation order); the weight and pad-channel mutants live here."""
    epi, cin, co = layer
    nbr = cloud(key)['nbr']
    x, W, b = inputs(layer, key)['x'], rb32(param(layer, 'kernel')).clone(), param(layer, 'bias').view(1, -1)
    if mut == 'taps_swapped':
        W[[3, 17]] = W[[17, 3]]
    if mut == 'quad_zeroed':
        W[5, 0:4, 4:8] = 0.0
    if mut == 'pad_not_ignored':
        pad = -cin % 8
        assert pad, 'the layer has no pad channel'
        x = torch.cat([x, torch.full((x.shape[0], pad), 7.0)], dim=1)
        W = torch.cat([W, W[:, torch.arange(pad) % cin]], dim=1)          # the pad channels meet some non-zero weights
    return onet.conv3(x, nbr, W, b)


def emulate(layer, key, form, mut=None):
    """The stored values of a convolution entry ([n, width] fp32 holding bf16 values) as fp32 arithmetic gives them; `mut` in MUTANTS
    breaks one step."""
    epi, cin, co = layer
    t = inputs(layer, key)
    store = trunc32 if mut == 'truncate_store' else rb32
    o = _emu_conv(layer, key, mut)
    if epi == WE_PLAIN:
        if form in ('res_relu', 'res_relu_res2'):
            o = torch.relu(o + t['res'])
    elif epi == WE_PW1:
        h1 = t['x'] @ param(layer, 'pw_w') + param(layer, 'pw_b')
        o = torch.relu(torch.cat([o, h1], dim=1))
    else:
        m = torch.relu(o)
        if mut != 'm_unrounded':
            m = rb32(m)
        o = (m @ param(layer, 'pw_w') + param(layer, 'pw_b')) + t['x_hi']
    if form in ('res2', 'res_relu_res2'):
        o = torch.cat([(o[:, :co] if mut == 'res2_before_rounding' else rb32(o[:, :co])) + t['res2'], o[:, co:]], dim=1)
    return store(o)


def emulate_head(layer, key, t_col, mut=None):
    """(p fp32 [n], partial float64 [blocks]) of the head in fp32 arithmetic."""
    c = _emu_conv(layer, key, mut)
    if mut == 'head_rounded_c':
        c = rb32(c)
    z = head_ref.head_logits(c, param(layer, 'w1'), param(layer, 'b1'), param(layer, 'w2'), param(layer, 'b2'))
    p = head_ref.sigmoid32(z)
    part = partial64(p, inputs(layer, key)['target'][:, t_col])
    if mut == 'dead_lane_counted':
        part = part.clone()
        part[-1] += head_ref.nats(p[-1:], inputs(layer, key)['target'][-1:, t_col])[0]
    return p, part
