"""Float64 reference of the scale context (models/model_core.py:48-53) on a frame descriptor (row_off, scale_idx, offset_feat) and the
FLAT parameters as the library lays them out (csrc/layout.h: scale_emb [S][8], then per scale 0.weight [16][15], 0.bias [16], 2.weight
[8][16], 2.bias [8]) - tests/test_sce_ref.py checks it on the CPU against oracle.network.scale_context + float64 autograd,
tests/test_gpu_multi_tile.py holds linr_sce_fwd / linr_sce_bwd / linr_sce_bwd_params to it.  Per row r of a range of scale s:
    x    = [emb_s | offset_feat[r]]                      hpre = W1_s x + b1_s        hid = relu(hpre)        x0 = W2_s hid + b2_s
    ghid = (gx0[r] W2_s) * (hid > 0)
and the gradients of sum_r gx0[r] . x0[r] in the layout linr_sce_bwd_params writes (the flat layout above):
    g 0.weight = sum_r ghid[r] (x) x[r]     g 0.bias = sum_r ghid[r]     g 2.weight = sum_r gx0[r] (x) hid[r]     g 2.bias = sum_r gx0[r]
    g scale_emb[s] = (g 0.bias) W1_s[:, :8]
Scales the frame does not name, and scales it names with zero rows, get exact zeros (their embedding rows included).  Two row ranges of
one scale are summed here (the library refuses such a frame).
Beside every value goes the same expression over the absolute values of all its inputs, the ReLU mask kept (`*_abs`): what
tests/gpu_common.py::_within_rounding scales its bound with.  It is nested - hid_abs = |W1| |x| + |b1|, x0_abs = |W2| hid_abs + |b2|,
g 2.weight_abs = sum_r |gx0[r]| (x) hid_abs[r], ... - so the rounding of an intermediate the kernels form in fp32 is covered too.
`min_pre` is the smallest |hpre| over all rows: below ~3e-7 (tests/gpu_common.py::_smallest_relu_input) the side of that ReLU is decided
by fp32 rounding order and no two fp32 evaluations need agree.
Everything runs on the device of `offset_feat` (CPU in tests/test_sce_ref.py, the GPU at 300 k rows)."""
import numpy as np
import torch

PER_SCALE = 16 * 15 + 16 + 8 * 16 + 8          # 392


def param_count(S):
    return S * 8 + S * PER_SCALE


def names(S):
    """state_dict names in the order of the flat layout"""
    return ['scale_emb.weight'] + ['scale_mlp.%d.%d.%s' % (si, l, w) for si in range(S) for l in (0, 2) for w in ('weight', 'bias')]


def unpack(flat, S):
    """flat [param_count(S)] -> {'emb': [S, 8], si: (W1 [16, 15], b1 [16], W2 [8, 16], b2 [8])} (views)"""
    assert flat.numel() >= param_count(S)
    out = {'emb': flat[:8 * S].view(S, 8)}
    for si in range(S):
        o = 8 * S + PER_SCALE * si
        out[si] = (flat[o:o + 240].view(16, 15), flat[o + 240:o + 256], flat[o + 256:o + 384].view(8, 16), flat[o + 384:o + 392])
    return out


def state_dict_of(flat, S):
    """the flat parameters under the reference's names (for oracle.network.scale_context)"""
    p = unpack(flat, S)
    sd = {'scale_emb.weight': p['emb']}
    for si in range(S):
        for key, v in zip(('0.weight', '0.bias', '2.weight', '2.bias'), p[si]):
            sd['scale_mlp.%d.%s' % (si, key)] = v
    return sd


def draw_params(S, seed):
    """fp32 flat parameters: embedding N(0, 1) as nn.Embedding draws it, weights N(0, 0.3^2), biases N(0, 0.1^2)"""
    gen = torch.Generator().manual_seed(seed)
    flat = torch.empty(param_count(S))
    p = unpack(flat, S)
    p['emb'].copy_(torch.randn(S, 8, generator=gen))
    for si in range(S):
        for v, sc in zip(p[si], (0.3, 0.1, 0.3, 0.1)):
            v.copy_(torch.randn(v.shape, generator=gen) * sc)
    return flat


def draw_frame(ranges, seed):
    """ranges: [(scale_idx, rows), ...] in frame order -> row_off int64 [n + 1], scale_idx int32 [n], offset_feat fp32 [R, 7] of random
    bits, gx0 fp32 [R, 8] normal."""
    gen = torch.Generator().manual_seed(seed)
    row_off = np.zeros(len(ranges) + 1, dtype=np.int64)
    row_off[1:] = np.cumsum([n for _, n in ranges])
    R = int(row_off[-1])
    off = (torch.rand(R, 7, generator=gen) < 0.5).float()
    gx0 = torch.randn(R, 8, generator=gen)
    return row_off, np.asarray([s for s, _ in ranges], dtype=np.int32), off, gx0


def reference(flat, S, row_off, scale_idx, offset_feat, gx0=None):
    """See the module docstring.  flat, offset_feat [R, 7], gx0 [R, 8] (optional) of any float type; float64 results on offset_feat's
    device: x0, hid, min_pre (+ ghid, grads with gx0), each with its `_abs` companion."""
    dev = offset_feat.device
    p = unpack(flat.detach().to(device=dev, dtype=torch.float64), S)
    off = offset_feat.detach().to(torch.float64)
    R = off.shape[0]
    assert int(row_off[0]) == 0 and int(row_off[-1]) == R and len(row_off) == len(scale_idx) + 1
    z = lambda c: torch.zeros((R, c), dtype=torch.float64, device=dev)
    out = {'x0': z(8), 'x0_abs': z(8), 'hid': z(16), 'hid_abs': z(16), 'min_pre': float('inf')}
    if gx0 is not None:
        g = gx0.detach().to(device=dev, dtype=torch.float64)
        out.update(ghid=z(16), ghid_abs=z(16), grads=torch.zeros(param_count(S), dtype=torch.float64, device=dev),
                   grads_abs=torch.zeros(param_count(S), dtype=torch.float64, device=dev))
        gp, gpa = unpack(out['grads'], S), unpack(out['grads_abs'], S)
    for j, si in enumerate(int(s) for s in scale_idx):
        a, b = int(row_off[j]), int(row_off[j + 1])
        assert 0 <= si < S and a <= b
        if a == b:
            continue
        W1, b1, W2, b2 = p[si]
        x = torch.cat([p['emb'][si].unsqueeze(0).expand(b - a, -1), off[a:b]], dim=1)
        hpre = x @ W1.t() + b1
        out['min_pre'] = min(out['min_pre'], float(hpre.abs().min()))
        hid = torch.relu(hpre)
        hid_abs = x.abs() @ W1.abs().t() + b1.abs()
        out['hid'][a:b], out['hid_abs'][a:b] = hid, hid_abs
        out['x0'][a:b] = hid @ W2.t() + b2
        out['x0_abs'][a:b] = hid_abs @ W2.abs().t() + b2.abs()
        if gx0 is None:
            continue
        mask = (hpre > 0).to(torch.float64)
        gj, gja = g[a:b], g[a:b].abs()
        ghid, ghid_abs = (gj @ W2) * mask, (gja @ W2.abs()) * mask
        out['ghid'][a:b], out['ghid_abs'][a:b] = ghid, ghid_abs
        for dst, parts in ((gp, (ghid.t() @ x, ghid.sum(0), gj.t() @ hid, gj.sum(0), W1)),
                           (gpa, (ghid_abs.t() @ x.abs(), ghid_abs.sum(0), gja.t() @ hid_abs, gja.sum(0), W1.abs()))):
            gW1, gb1, gW2, gb2, w = parts
            for t, v in zip(dst[si], (gW1, gb1, gW2, gb2)):
                t += v
            dst['emb'][si] += gb1 @ w[:, :8]
    return out
