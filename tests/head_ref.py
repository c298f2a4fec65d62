"""Reference of the occupancy heads on SATURATED logits (tests/test_head_ref.py checks it on the CPU, tests/test_gpu_heads_saturated.py
uses it against the kernels): a plain restatement of the operation AS THE REFERENCE DEFINES IT - torch's BCELoss(sum) on an fp32
sigmoid (models/upsample.py:160, models/model_core.py:72-81) - not of the true sigmoid loss.  Where the two differ the semantics are
piecewise, and every piece is spelled out here once:

  p    = 1 / (1 + exp(-z))                                    formed in float32 from the float32-rounded logit: exactly 1 from
                                                              z ~ 16.6 .. 17.4 on, accurate down to z ~ -87, exactly 0 below ~ -104
  nats = -t max(log p, -100) - (1 - t) max(log(1 - p), -100)  `1 - p` formed in float32, everything else float64 (recent torch
                                                              CPU builds take log1p(-p): at most half an ulp of 1 per row away)
  gz   = gscale (p - t) / max((1 - p) p, 1e-12) * ((1 - p) p) float64 on the fp32 p it is GIVEN (the backward entries take p as an
                                                              input): BCELoss's backward times the sigmoid's
and a head on top of it, c -> relu(W1 c + b1) -> w2 . + b2 -> z, with its explicit backward (gc and the gradients of W1, b1, w2, b2).
Every function takes a dtype: float64 is the reference, float32 the "fp32 oracle" of the criterion of tests/gpu_common.py
    err_hip(f64) <= max(3 err_oracle32(f64), 1e-4 max|g_tensor|).

choose_targets() makes every row well conditioned BY CONSTRUCTION (no masking afterwards):
  z in (8, 20)    -> t = 1.  There 1 - p has only a few bits and p rounds to 1 somewhere between 16.6 and 17.4, so with t = 0 two correct
                     fp32 evaluations of the same row differ by up to 83 nats (17 against 100): the question is never asked (this
                     project's ReLU-tie situation).  The bf16 executors' logits are ~2e-2 from their emulating oracle's: (6, 24) there.
  z < -80         -> t = 0.  p leaves the normal range at z ~ -87.3 (log p loses its bits) and the clamp at -100 nats sits behind it.
  everything else -> ~30 % of the rows contradicted (t against the sign of z), the classes being
                     contradicted high  z >= 20, t = 0: p == 1.0f, exactly 100 nats, gz == 0
                     contradicted low   -80 <= z <= -20, t = 1: -z nats; gz crosses the 1e-12 switch at z ~ -27.6
                     agreeing saturated |z| >= 20 and t on the side of z
                     ordinary           -20 < z <= 8
Final ranges: as above, nothing had to be narrowed - on the inputs of saturated_case() the fp32 oracle (oracle/network.py pieces) stays
within 1e-5 relative of this file's float64 bits at every n and width (tests/test_head_ref.py asserts it).
"""
import functools
import math

import numpy as np
import torch

LN2 = math.log(2.0)
BAND = (8.0, 20.0)               # fp32 executors: logits within 1e-4 + 1e-4 |z| of the float64 ones
BAND_BF16 = (6.0, 24.0)          # bf16 executors: logits within 2e-2 of the emulating oracle's
CLASSES = ('contradicted_high', 'contradicted_low', 'agreeing_saturated', 'ordinary')


def sigmoid32(z):
    """p as the kernels and torch's fp32 sigmoid form it: float32 arithmetic on the float32-rounded logit (exp(-z) may overflow to inf:
    p = 0)."""
    z32 = torch.as_tensor(z).to(torch.float32)
    return 1.0 / (1.0 + torch.exp(-z32))


def nats(p32, t, dtype=torch.float64):
    """Per-row BCELoss terms on an fp32 probability: the two logs clamped at -100, `1 - p` in float32."""
    assert p32.dtype == torch.float32
    q32 = 1.0 - p32
    t = t.to(dtype)
    lp = torch.clamp(torch.log(p32.to(dtype)), min=-100.0)
    lq = torch.clamp(torch.log(q32.to(dtype)), min=-100.0)
    return -t * lp - (1.0 - t) * lq


def bits(p32, t, dtype=torch.float64):
    return nats(p32, t, dtype).sum() / LN2


def gz_of(p32, t, gscale, dtype=torch.float64):
    """d (gscale * nats) / dz on the fp32 p it is given: BCELoss's backward (quotient clamped at 1e-12) times the sigmoid's."""
    assert p32.dtype == torch.float32
    p, t = p32.to(dtype), t.to(dtype)
    q = (1.0 - p) * p
    return gscale * (p - t) / torch.clamp(q, min=1e-12) * q


def head_logits(c, w1, b1, w2, b2):
    """PointwiseMLP([C, 24, 1]) (models/upsample.py:73-76): w1 [24, C], b1 [24], w2 [24], b2 [1] -> z [n]."""
    return torch.relu(c @ w1.t() + b1) @ w2.reshape(-1) + b2.reshape(())


def head_backward(c, p32, t, w1, b1, w2, gscale, dtype=torch.float64):
    """The backward entries' contract: from c, the STORED fp32 probability and the target to gc [n, C] and the gradients of W1, b1, w2, b2
    (of gscale * nats summed over the rows), all in `dtype`.  The hidden layer is recomputed from c."""
    c, w1, b1, w2 = (x.to(dtype) for x in (c, w1, b1, w2.reshape(-1)))
    gz = gz_of(p32, t, gscale, dtype)
    hpre = c @ w1.t() + b1
    gh = gz[:, None] * w2[None, :] * (hpre > 0).to(dtype)
    return {'gz': gz, 'gc': gh @ w1, 'gw1': gh.t() @ c, 'gb1': gh.sum(0), 'gw2': (gz[:, None] * torch.relu(hpre)).sum(0),
            'gb2': gz.sum().reshape(1)}


def choose_targets(z64, rng, band=BAND):
    """Targets for float64 logits z64 [n] (see the module docstring) and the per-class row counts (CLASSES, plus 'band' and
    'forced_low')."""
    z = np.asarray(z64, dtype=np.float64).reshape(-1)
    agree = (z > 0).astype(np.float32)
    flip = rng.random(z.shape[0]) < 0.3
    in_band = (z > band[0]) & (z < band[1])
    low = z < -80.0
    flip &= ~in_band & ~low
    t = np.where(flip, 1.0 - agree, agree).astype(np.float32)
    sat_hi, sat_lo = z >= band[1], (z <= -band[1]) & ~low
    counts = {'contradicted_high': int((sat_hi & flip).sum()), 'contradicted_low': int((sat_lo & flip).sum()),
              'agreeing_saturated': int(((sat_hi | sat_lo | low) & ~flip).sum()),
              'ordinary': int(((z > -band[1]) & (z <= band[0])).sum()), 'band': int(in_band.sum()), 'forced_low': int(low.sum())}
    assert bool((t[in_band] == 1).all()) and bool((t[low] == 0).all())
    return t, counts


# ---- the inputs of the op-level forward tests ---------------------------------------------------------------------------------------------
NS = (1, 63, 64, 65, 257, 1025)


def raw_case(n, C):
    """Layers as the existing head tests draw them - the SAME layers at every n (drawn first) - and n rows of input.  C = 8: the fp32
    executor's head INCLUDING its prune convolution (prior, kernel map); C = 16 / 32: the wide head on c itself."""
    from oracle import network as onet
    from oracle import octree as ooct
    gen = torch.Generator().manual_seed(1000 * C)
    s = 0.5 if C == 8 else 0.3
    case = {'n': n, 'C': C, 'w1': torch.randn(24, C, generator=gen) * s, 'b1': torch.randn(24, generator=gen) * 0.1,
            'w2': torch.randn(24, generator=gen) * s, 'b2': torch.randn(1, generator=gen) * 0.1}
    if C == 8:
        case.update(Wp=torch.randn(27, 8, 8, generator=gen) * 0.15, bp=torch.randn(8, generator=gen) * 0.1)
        side = max(6, int(round((3 * n) ** (1 / 3))) + 2)
        rng = np.random.default_rng(n + C)
        coord = ooct.unique_sorted(rng.integers(0, side, size=(4 * n, 3)))[:n]
        assert len(coord) == n
        case.update(coord=coord, nbr=torch.from_numpy(ooct.neighbour_table(coord)).long(), prior=torch.randn(n, 8, generator=gen))
        case['c64'] = onet.conv3(case['prior'].double(), case['nbr'], case['Wp'].double(), case['bp'].double().view(1, -1))
    else:
        case['c'] = torch.randn(n, C, generator=gen)
        case['c64'] = case['c'].double()
    return case


@functools.lru_cache(maxsize=None)
def _calibrated_output_layer(C):
    """w2 and b2 scaled so that the float64 logits have a standard deviation near 40, b2 then shifted so that they straddle zero (their
    median on the 1025-row case: relu(.) . w2 has a mean of its own, and a head whose logits are all of one sign draws no contradicted
    rows on the other side).  One output layer per width, the same at every n."""
    k = raw_case(1025, C)
    z = head_logits(k['c64'], k['w1'].double(), k['b1'].double(), k['w2'].double(), k['b2'].double())
    sc = 40.0 / float(z.std())
    w2, b2 = (k['w2'] * sc).contiguous(), k['b2'] * sc
    z = head_logits(k['c64'], k['w1'].double(), k['b1'].double(), w2.double(), b2.double())
    return w2, (b2 - float(z.median())).float().contiguous()


@functools.lru_cache(maxsize=None)
def saturated_case(n, C):
    """One forward case: fp32 inputs, the float64 logits of those fp32 inputs, targets by choose_targets and their class counts, the
    reference's fp32 p and float64 bits.  Cached and shared: do not modify."""
    k = raw_case(n, C)
    k['w2'], k['b2'] = _calibrated_output_layer(C)
    k['z64'] = head_logits(k['c64'], k['w1'].double(), k['b1'].double(), k['w2'].double(), k['b2'].double())
    t, k['counts'] = choose_targets(k['z64'].numpy(), np.random.default_rng(7 * n + C))
    k['t'] = torch.from_numpy(t)
    k['p32'] = sigmoid32(k['z64'])
    k['bits64'] = float(bits(k['p32'], k['t']))
    return k


def oracle32_bits(k):
    """The fp32 oracle of a saturated_case: oracle/network.py pieces + torch's own fp32 sigmoid and binary_cross_entropy, as in
    tests/test_gpu_fused_ops.py::test_head_forward_backward."""
    import torch.nn.functional as F
    from oracle import network as onet
    c = onet.conv3(k['prior'], k['nbr'], k['Wp'], k['bp'].view(1, -1)) if k['C'] == 8 else k['c']
    z = F.linear(F.relu(F.linear(c, k['w1'], k['b1'])), k['w2'].view(1, -1), k['b2'])
    return float(F.binary_cross_entropy(torch.sigmoid(z), k['t'].view(-1, 1), reduction='sum').double() / LN2)


# ---- the inputs of the op-level backward tests: probabilities supplied directly -------------------------------------------------------------
def supplied_probabilities():
    """fp32 probabilities around every piece of the backward: 0, 1, the smallest denormal, the smallest normal, both sides of the 1e-12
    switch in (1 - p) p (none within 10 % of it), ordinary values, and the two largest p below 1 that matter."""
    one = np.float32(1.0)
    vals = [np.float32(0.0), one, np.nextafter(np.float32(0.0), one), np.float32(1.18e-38), np.float32(1e-13), np.float32(5e-13),
            np.float32(2e-12), np.float32(1e-6), np.float32(0.5), one - np.float32(2.0 ** -24), one - np.float32(1e-3)]
    q = np.array([(1.0 - float(v)) * float(v) for v in vals])
    assert not bool(((q > 0.9e-12) & (q < 1.1e-12)).any())
    return np.array(vals, dtype=np.float32)


def supplied_rows(n):
    """(p32 [n], t [n]): the 11 probabilities x {t = 0, t = 1} in a cycle; row n - 1 always holds p = 1e-6 against t = 1 (|gz| = gscale to
    1e-6: no row of the cloud has a larger one)."""
    vals = supplied_probabilities()
    i = np.arange(n)
    p = vals[(i // 2) % len(vals)].copy()
    t = (i % 2).astype(np.float32)
    p[n - 1], t[n - 1] = np.float32(1e-6), 1.0
    return torch.from_numpy(p), torch.from_numpy(t)
