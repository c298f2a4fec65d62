"""Helpers shared by the GPU parity tests (tests/test_gpu_*.py); the fixtures `pkg` and `shell` live in conftest.py.

Tolerances (the reference states none): fp32 HIP vs fp32 oracle
  logits  |d| <= 1e-4 + 1e-4 |x|     bits  rel <= 1e-5
  gradients, per tensor against ITS OWN largest entry: the HIP gradient must be as close to the float64 oracle as the fp32
  oracle itself is, err_hip(f64) <= max(3 * err_oracle32(f64), 1e-4 * max|g_tensor|); the direct fp32-vs-fp32 difference
  (two summation orders of sums with heavy cancellation) is only sanity-bounded: 1e-3 * max|g_tensor| at block_layers 1, 3e-3 for the deeper block_in variants
Integer / index / byte work (kernel map, streams, decoded geometry) is bit-exact.
"""
import numpy as np
import torch

from oracle import network as onet


def _dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


def _close(a, b, rtol, atol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    assert bool((err <= tol).all()), '%s: max err %.3e (tol %.3e at worst)' % (what, float(err.max()), float(tol.min()))


# ---- whole network --------------------------------------------------------------------------------------------------------
def _model_and_oracle(pkg, scale_num, seed=8807, block_layers=1):
    from linr_pcgc_amd.model_core import LINR_PCGC_Model
    torch.manual_seed(seed)
    model = LINR_PCGC_Model({'scale_num': scale_num, 'in_channel': 7, 'hidden_channel_conv': 8, 'block_layers': block_layers,
                             'outstage': 8, 'instage': 1})
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return model.cuda(), sd


def _grad_or_zero(leaf):
    """A leaf's gradient as float64 on the host; a leaf the loss never reached (grad None: the scale MLP of a scale the frame does not
    hold) has a zero gradient, which the executor must then give exactly (within the floor)."""
    if leaf.grad is None:
        return torch.zeros(leaf.shape, dtype=torch.float64)
    return leaf.grad.detach().double().cpu()


def _grads_close_per_tensor(grads, sdo, rtol=1e-3, floor=1e-9, sd64=None, slack=None, report=None):
    """Every tensor against ITS OWN largest gradient (a tensor whose gradients are orders of magnitude below the model's
    largest one must still be right).  A gradient entry is a sum over all rows with heavy cancellation (bias gradients
    most of all), so two fp32 evaluations in different summation orders (the oracle adds the taps in ascending order, the
    kernels column by column: common.h LINR_TAP) differ by up to ~2e-3 of the tensor's largest entry at block_layers 3
    (measured worst: 2.07e-3 on a bias gradient of 5e-4): the direct fp32-vs-fp32 bound (rtol) is only a sanity check.  The criterion proper needs sd64, the
    same leaves evaluated by the oracle in float64: the HIP gradient must be as accurate as the fp32 oracle is,
        err_hip(f64) <= max(3 * err_oracle32(f64), 1e-4 * max|g_tensor|).
    grads: the executor's flat gradient in the order of sdo; sdo / sd64: leaves on any device.  slack (_relu_tie_slack): per tensor, what
    the ReLU inputs at fp32 resolution of a fixed cloud can move the gradient by, added to the float64-anchored bound.  report: a list
    that receives (name, err_hip, err_oracle32, own max) of every tensor checked against sd64, before its assertion."""
    off, worst = 0, (0.0, '')
    for name, v in sdo.items():
        n = v.numel()
        mine = grads[off:off + n].view(v.shape).detach().double().cpu()
        ref = _grad_or_zero(v)
        gmax = float(ref.abs().max())
        err = float((mine - ref).abs().max())
        assert err <= rtol * gmax + floor, 'grad %s: max err %.3e vs tolerance %.3e (own max %.3e)' % (name, err, rtol * gmax + floor, gmax)
        if sd64 is not None:
            truth = _grad_or_zero(sd64[name])
            e_hip, e_o32 = float((mine - truth).abs().max()), float((ref - truth).abs().max())
            tie = slack[name] if slack else 0.0
            if report is not None:
                report.append((name, e_hip, e_o32, gmax))
            assert e_hip <= max(3.0 * e_o32, 1e-4 * gmax) + tie + floor, \
                'grad %s vs float64: HIP %.3e, fp32 oracle %.3e (own max %.3e, ReLU-tie slack %.3e)' % (name, e_hip, e_o32, gmax, tie)
        if gmax > 0 and err / gmax > worst[0]:
            worst = (err / gmax, name)
        off += n
    return worst


def _smallest_relu_input(sd, sc):
    """Smallest |x| any ReLU of the network sees on this scale, from the oracle in float64.  Below ~3e-7 (inputs are O(1)) the sign of x - and with
    it a whole term of the gradient - is decided by fp32 rounding order, so no two fp32 implementations need agree there."""
    import types
    seen = []

    def relu(x):
        if x.numel():
            seen.append(float(x.detach().abs().min()))
        return torch.relu(x)
    shim = types.SimpleNamespace(relu=relu, linear=torch.nn.functional.linear,
                                 binary_cross_entropy=torch.nn.functional.binary_cross_entropy)
    keep, onet.F = onet.F, shim
    try:
        with torch.no_grad():
            onet.forward_scale({k: v.double() for k, v in sd.items()}, onet.to_torch_scales([sc], torch.float64)[0])
    finally:
        onet.F = keep
    return min(seen)


def _relu_tie_slack(sd, scales, gscale=1.0, thresh=3e-7):
    """For clouds that cannot be redrawn: every ReLU input with |x| < thresh (float64 oracle) is a tie at fp32 resolution - its side, and
    with it a whole term of the gradient, is decided by rounding order.  Per tensor, the sum over those inputs of how far the float64
    oracle's gradient of gscale * bits moves (max abs) when that one input is put on the other side: what two correct fp32 evaluations
    may differ by beyond rounding.  Zero when there is no tie.  scales: numpy scale dicts."""
    import types
    slack = {k: 0.0 for k in sd}

    def grads_of(sc, flip=None, ties=None):
        cnt = [0]

        def relu(x):
            i = cnt[0]
            cnt[0] += 1
            if ties is not None:
                ties.extend((i, int(j)) for j in torch.nonzero(x.detach().abs().reshape(-1) < thresh).reshape(-1))
            if flip is None or flip[0] != i:
                return torch.relu(x)
            mask = (x.detach() > 0).to(x.dtype).reshape(-1).clone()
            mask[flip[1]] = 1.0 - mask[flip[1]]
            return x * mask.reshape(x.shape)
        shim = types.SimpleNamespace(relu=relu, linear=torch.nn.functional.linear,
                                     binary_cross_entropy=torch.nn.functional.binary_cross_entropy)
        keep, onet.F = onet.F, shim
        try:
            leaves = {k: v.double().clone().requires_grad_() for k, v in sd.items()}
            (onet.forward_scale(leaves, onet.to_torch_scales([sc], torch.float64)[0])['bits'] * gscale).backward()
        finally:
            onet.F = keep
        return {k: v.grad for k, v in leaves.items() if v.grad is not None}

    for sc in scales:
        ties = []
        base = grads_of(sc, ties=ties)
        for t in ties:
            moved = grads_of(sc, flip=t)
            for k, g in moved.items():
                slack[k] += float((g - base[k]).abs().max())
    return slack


# ---- per-entry rounding bounds (tests/test_gpu_wide.py, tests/test_gpu_multi_tile.py) --------------------------------------------
# Op level at the multi-tile size: per-entry bounds against float64.  A relative-to-max bound loses its sharpness at 1e5 rows (one lost
# 256-row tile moves a weight-gradient entry by ~1e-3 of its largest), so every entry gets the rounding bound of its own sum,
#     |got - exact| <= C_ROUND * 2^-24 * (the same sum over the absolute values of its terms)
# (forward: |x| (*) |W| + |b| + |res|; backward-data: |g| (*) |W|^T; weight gradients: sum over rows of |x| |g|), computed by the same
# float64 oracle.  A recursive fp32 sum of m terms errs by at most ~m 2^-24 of that; the kernels' sums are blocked (depth < 200 at 157 k
# rows) and rounding errors cancel, so C_ROUND = 64 is far above what any summation order gives in practice and far below what a skipped
# tile or 8-row group costs (16 of a typical term per 256 rows, against 64 2^-24 157 k = 0.6 of one).  Measured on the MI355X: worst
# entries at 0.12 of the bound (forward), 0.1 (backward-data), 1.4e-3 (weight gradients); a weight-gradient kernel that drops the last
# 8-row group lands at 17-43 x.  Every output is pre-filled with NaN, so a tile that is never written fails instead of reading stale memory.
C_ROUND = 64.0
_U = 2.0 ** -24


def _within_rounding(got, exact, absum, what):
    got = got.double()
    tol = C_ROUND * _U * absum
    ratio = (got - exact).abs() / tol.clamp(min=1e-300)
    assert bool(torch.isfinite(got).all()), '%s: %d entries never written (NaN)' % (what, int((~torch.isfinite(got)).sum()))
    worst = float(ratio.max())
    assert bool(((got - exact).abs() <= tol).all()), '%s: worst entry at %.3g x its bound' % (what, worst)
    return worst


# Adam's arguments as they reach a fused training step (one linr_step_args) and FlatAdam.step (positional scalars of linr_adam_step):
# the defaults every other test uses, and a set of pairwise distinct non-default values, with a loss scale that is not
# 1 / point_num (ADAM_DISTINCT_GSCALE_DIV times smaller) - a field of the struct that is dropped or swapped with a neighbour changes
# the fused path alone
ADAM_DEFAULT = dict(lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
ADAM_DISTINCT = dict(lr=2e-3, betas=(0.7, 0.95), eps=1e-5, weight_decay=3e-3)
ADAM_DISTINCT_GSCALE_DIV = 1.7
