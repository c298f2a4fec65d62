"""Executor for ``hidden_channel_conv`` = 16 / 32 (main.py:520; models/upsample.py:38-76 ``channels=``, models/resnet.py:12-51
``channels // 2``): the same network with wider feature rows, on CHANNEL-BLOCKED activations.

Every C-wide activation is kept as C / 8 separate [rows + 1][8] matrices (zero row in front, what the kernels gather from).  Every
layer is ONE launch of a kernel of csrc/wide.hip: a convolution Ci -> Co ``linr_spconv_wide`` (every input block of a row gathered
once per tap, the weights of a tap as an A-operand image in LDS, all output channels from that one gather; the same for
backward-data at the mirrored taps; the Inception layer's pointwise convolutions conv1_0 / conv1_2 and their backward-data passes ride
in its epilogue: its ``pw`` argument), its weight gradient ``linr_spconv_wgrad_wide`` (one gather per input block for all gradient
blocks; conv0_1 and conv1_1 together: ``linr_spconv_wgrad_wide2``), the pointwise weight gradients ``linr_linear_wgrad_wide``, a stage's
head ``linr_head_wide_fwd`` and the backward of all 8 heads ``linr_head_wide_bwd``; the scale context (width-independent) runs on the
8-wide network's kernels (``linr_sce_fwd``, ``linr_sce_bwd_params``).  The ~64 slab reductions of a backward pass are deferred into
two launches (``linr_wide_reduce_many``).  Concatenations are free; the padded block buffers of a training step come from a pool.
Deterministic (fixed launch order, no atomics); the forward is the same launches in training, encoding and stage-by-stage decoding,
so streams decode losslessly.

The schedule below is Python (~190 launches per step; GPU-bound on the BASELINE-sized frames, launch-bound on small ones): 5.9 / 18.1 ms
per training step at widths 16 / 32 on the loot-like frame (profiles/r04_wide.txt; ~3.7x / ~14x the convolution work of width 8).  The
8-wide model (every BASELINE config, the reference's default and its shipped checkpoint) never comes here.

Opt-in (WideNet.c_step, LINR_WIDE_C_STEP=1): model_core.train_step sends the whole step - the forward with its tape, the backward, Adam,
and with qat_bitdepth the fake quantisation in front - to ONE C call (csrc/wide_train.hip: linr_net_train_step_wide), which makes the
same launches with the same arguments on an arena of its own (step_arena below: per model, no pool, no lock), so the bits, the moments
and the parameters are those of this schedule bit for bit (tests/test_gpu_wide_step.py; profiles/wide_step.txt).  Without it
forward(keep=True) / backward / FlatAdam.step run as ever; they, the _Pool and the autograd surface are the C call's cross-check.

The full-range inference forward (frame_probs, the encoder) does not run this schedule by default: WideNet.c_forward sends it to the
same launches scheduled in C (csrc/wide_fwd.hip: forward_c), and the decoder's scales are C calls on that forward
(model.decode_scale -> linr_decode_scale_wide).  Stage ranges (model.decode's stage loop, the cross-check of those entries) and the
training passes of the autograd surface stay here; the bits are the same on either schedule.

train_precision 'bf16-mul' (opt-in): a training forward (keep=True) and its backward run the same launches with LINR_MUL_BF16 - the
products of the 3x3x3 convolutions on bf16 matrix instructions, operands rounded at the multiply, everything else fp32 (csrc/wide_mul.hip;
_Pass.mul below; 5.31 / 13.8 ms per step, profiles/wide_bf16_mul.txt).  Every other forward multiplies in fp32.

What a running pass needs beyond its inputs - the frame's tables, the buffer pool, the list of deferred reductions, the precision of the
products - travels in a _Pass that forward / backward build per call and hand to every layer method: nothing is kept per thread or on
the executor, so passes of several models and frames interleave freely (the model's lock guards its pool, _build and the bf16 state).

forward_bf16 is the inference forward of --precision bf16 (BASELINE config[4]'s numerics) on csrc/wide_bf16.hip: the uint8 weight codes
as the model, bf16 channel-blocked activations, fp32 accumulation, one launch per layer in the same schedule (profiles/r07_wide_bf16.txt).
"""
import ctypes
import os
import threading

import torch

from . import _lib, ops
from ._lib import LINR_ACCUM, LINR_NO_BIAS, LINR_RELU, LINR_RELU_MASK, check

B = 8


def _stream():
    return _lib.current_stream_handle()


class _Pool:
    """Zero-padded block buffers reused from step to step (train_step's schedule asks for the same sequence every time): the kernels
    never write a block's row 0, so it is cleared once when the buffer is made instead of once per request (88 fill launches per step at
    width 16).  A buffer is [nb][cap + 1][8]; a request for fewer rows gets views of its first rows."""

    def __init__(self):
        self.bufs, self.i = [], 0

    def reset(self):
        self.i = 0

    def take(self, n, nb, dev):
        i = self.i
        self.i += 1
        if i < len(self.bufs):
            b = self.bufs[i]
            want = dev.index if dev.index is not None else (torch.cuda.current_device() if dev.type == 'cuda' else None)
            if b.shape[0] == nb and b.shape[1] > n and b.device.type == dev.type and want == b.device.index:
                return [b[j, 1:n + 1] for j in range(nb)]
        b = torch.empty((nb, n + 1, B), dtype=torch.float32, device=dev)
        b[:, 0].zero_()
        if i < len(self.bufs):
            self.bufs[i] = b
        else:
            self.bufs.append(b)
        return [b[j, 1:] for j in range(nb)]


class _Pass:
    """What ONE WideNet.forward / backward call runs on, handed to every layer method that launches: the frame's tables and row count,
    `pool` = the model's _Pool (train_step) or None for fresh buffers, `defer` = the backward's list of deferred weight-gradient
    reductions (one launch per 32 at its end) or None in a forward, `mul` = what the 3x3x3 convolutions multiply in ('bf16' in the
    training passes of a train_precision 'bf16-mul' model, else 'f32': every codec, decoder and probability forward), `fuse_pw` = the
    pointwise layers of an Inception layer in the convolutions' epilogues.  Nothing of a pass is kept on the executor or the thread."""
    __slots__ = ('lo', 'mask', 'nbr', 'tile8t', 'n', 'dev', 'pool', 'defer', 'mul', 'fuse_pw')

    def __init__(self, frame, pool, defer, mul, fuse_pw):
        self.lo, self.mask, self.nbr, self.tile8t = frame.nbr_lo, frame.nbr_mask, frame.nbr, frame.nbr8t
        self.n, self.dev = frame.rows, frame.occ.device          # (the device WITH its index: what the blocks and _ZW are keyed by)
        self.pool, self.defer, self.mul, self.fuse_pw = pool, defer, mul, fuse_pw

    def blocks(self, nb):
        """nb zero-padded [n, 8] matrices (views buf[1:] of [n + 1, 8] buffers whose row 0 is zero)."""
        if self.pool is not None:
            return self.pool.take(self.n, nb, self.dev)
        buf = torch.empty((nb, self.n + 1, B), dtype=torch.float32, device=self.dev)
        buf[:, 0].zero_()
        return [buf[i, 1:] for i in range(nb)]


def _lin_bwd_data(gout, w, w_off, ws_ci, ws_co, cin, cout, out, act=None, accumulate=False):
    n = gout.shape[0]
    flags = (LINR_ACCUM if accumulate else 0) | (LINR_RELU_MASK if act is not None else 0)
    check(_lib.lib().linr_linear_bwd_data(gout.data_ptr(), gout.stride(0), n, w.data_ptr() + 4 * w_off, ws_ci, ws_co, cin, cout,
                                          0 if act is None else act.data_ptr(), 0 if act is None else act.stride(0),
                                          out.data_ptr(), out.stride(0), flags, _stream()), 'linr_linear_bwd_data')


def _axpy(src, dst, accumulate=True):
    check(_lib.lib().linr_axpy(src.data_ptr(), src.numel(), dst.data_ptr(), 1 if accumulate else 0, _stream()), 'linr_axpy')


class _Conv:
    """A 3x3x3 convolution Ci -> Co on blocked activations.  xs: Ci / 8 blocks (or one block with Ci < 8 live channels)."""

    def __init__(self, mod):
        self.mod = mod
        self.ci, self.co = mod.kernel.shape[1], mod.kernel.shape[2]
        self.nbi, self.nbo = (self.ci + B - 1) // B, self.co // B

    def fwd(self, ps, xs, relu=False, res=None, pw=None):
        """ONE launch (linr_spconv_wide): every input block of a row is gathered once per tap and feeds all output channels.
        pw: a pointwise layer fused into the epilogue (ops.spconv_wide)."""
        outs = ps.blocks(self.nbo)
        ops.spconv_wide(xs[:self.nbi], ps.lo, ps.mask, ps.n, self.mod.kernel, self.mod.bias.reshape(-1), res=res, relu=relu, outs=outs,
                        pw=pw, mul=ps.mul)
        return outs

    def bwd(self, ps, xs, gouts, act=None, need_input_grad=True, res=None, pw=None, wgrad=True, into=None, accumulate=False):
        """Parameter gradients into .grad; the input gradient (+ res, masked by act > 0: the ReLU that produced xs) written to (or,
        accumulate, added to) the blocks `into`, or to fresh blocks.  Returns the input gradient's blocks."""
        # weight gradients: all (input block, gradient block) pairs as groups of grouped launches of the transposing 8-wide kernel, ONE
        # fixed-order reduction straight into the parameter gradients (views of the flat gradient)
        if wgrad:
            ops.spconv_wgrad_wide(xs[:self.nbi], gouts[:self.nbo], ps.nbr, ps.tile8t, ps.n, self.ci, self.co,
                                  gw=self.mod.kernel.grad, gb=self.mod.bias.grad.reshape(-1), defer=ps.defer, mul=ps.mul)
        if not need_input_grad:
            return None
        gins = ps.blocks(self.nbi) if into is None else into
        # backward-data in one launch: the output gradient's blocks gathered once per (mirrored) tap for all input channels
        ops.spconv_wide(gouts[:self.nbo], ps.lo, ps.mask, ps.n, self.mod.kernel, None, bwd=True, act=act, res=res, outs=gins,
                        accumulate=accumulate, pw=pw, mul=ps.mul)
        return gins


class _Pointwise:
    """A 1x1 convolution (ME layout [Cin][Cout]) or an nn.Linear (torch layout [Cout][Cin]) on blocked inputs as ONE launch
    (linr_linear_wide); the output is blocked when cout is a multiple of 8, else one dense [n, cout] matrix."""

    def __init__(self, weight, bias, cin, cout, layout, blocked_out=True):
        self.w, self.b, self.cin, self.cout, self.layout = weight, bias, cin, cout, layout
        self.nbi = cin // B
        self.blocked_out = blocked_out and cout % B == 0
        self.nbo = cout // B if self.blocked_out else 1
        self.cw = B if self.blocked_out else cout
        self.ws = (cout, 1) if layout == 'me' else (1, cin)          # element (ci, co) at ci ws[0] + co ws[1]

    def fwd(self, ps, xs, relu=False, res=None, padded=True):
        outs = ps.blocks(self.nbo) if (self.blocked_out and padded) else \
            [torch.empty((ps.n, self.cw), dtype=torch.float32, device=ps.dev) for _ in range(self.nbo)]
        return ops.linear_wide(xs[:self.nbi], self.cin, self.w, self.ws[0], self.ws[1], self.b.reshape(-1), self.cout, outs,
                               out_blocked=self.blocked_out, res=res, relu=relu)

    def wgrad(self, ps, xs, gouts):
        """Parameter gradients into .grad (one grouped launch + one reduction); alone where the backward-data pass rides in a
        convolution's epilogue."""
        ops.linear_wgrad_wide(xs[:self.nbi], self.cin, gouts[:self.nbo], self.cout, self.w.grad, self.ws[0], self.ws[1],
                              self.b.grad.reshape(-1), g_blocked=self.blocked_out, defer=ps.defer)

    def bwd(self, ps, xs, gouts, act=None, into=None, accumulate=False):
        """wgrad(), then the input gradient (masked by act > 0) written to (or, accumulate, added to) the blocks `into`, or to fresh
        blocks.  Returns the input gradient's blocks."""
        self.wgrad(ps, xs, gouts)
        gins = ps.blocks(self.nbi) if into is None else into
        # backward-data: the same kernel with the roles of cin / cout and the weight strides swapped
        ops.linear_wide(gouts[:self.nbo], self.cout, self.w, self.ws[1], self.ws[0], None, self.cin, gins, in_blocked=self.blocked_out,
                        act=act, accumulate=accumulate)
        return gins


class _Block:
    """make_block (models/upsample.py:88-97): conv3 -> ReLU -> ResNetBlock (Inception layers) -> conv3."""

    def __init__(self, seq, C):
        self.C, self.h = C, C // 2
        self.first, self.tail = _Conv(seq[0]), _Conv(seq[3])
        self.layers = []
        for lay in seq[2].layers:
            h = self.h
            self.layers.append({'c00': _Conv(lay.conv0_0), 'c01': _Conv(lay.conv0_1),
                                'c10': _Pointwise(lay.conv1_0.kernel, lay.conv1_0.bias, C, h, 'me'), 'c11': _Conv(lay.conv1_1),
                                'c12': _Pointwise(lay.conv1_2.kernel, lay.conv1_2.bias, h, h, 'me')})

    def fwd(self, ps, xs, res=None):
        nh = self.h // B
        a = self.first.fwd(ps, xs, relu=True)
        tape = {'in': xs, 'a': a, 'layers': []}
        x = a
        for q in self.layers:
            # conv1_0 rides in conv0_0's launch (it reads the row itself: the centre tap), conv1_2 + the residual in conv1_1's: the
            # fmaf chains of the stand-alone pointwise kernel, so the bits are those of the five-launch form (fuse_pw False)
            if ps.fuse_pw:
                h1 = ps.blocks(nh)
                h0 = q['c00'].fwd(ps, x, relu=True, pw=(1, q['c10'].w, q['c10'].b.reshape(-1), None, h1))
            else:
                h0 = q['c00'].fwd(ps, x, relu=True)
                h1 = q['c10'].fwd(ps, x, relu=True)
            i_lo = q['c01'].fwd(ps, h0, res=x[:nh])
            if ps.fuse_pw:
                i_hi = ps.blocks(nh)
                m = q['c11'].fwd(ps, h1, relu=True, pw=(2, q['c12'].w, q['c12'].b.reshape(-1), x[nh:], i_hi))
            else:
                m = q['c11'].fwd(ps, h1, relu=True)
                i_hi = q['c12'].fwd(ps, m, res=x[nh:])
            tape['layers'].append({'x': x, 'h0': h0, 'h1': h1, 'm': m})
            x = i_lo + i_hi
        if len(self.layers) > 1:           # ResNetBlock.forward: out += x (models/resnet.py:160-161)
            for blk, ab in zip(x, a):
                _axpy(ab, blk)
        tape['il'] = x
        return self.tail.fwd(ps, x, res=res), tape

    def bwd(self, ps, tape, g_out, need_input_grad):
        """g_out: gradient blocks of the block output.  Returns the input gradient blocks (or None)."""
        nh = self.h // B
        nl = len(self.layers)
        fuse = ps.fuse_pw
        g_m_last = None
        if fuse:
            # gM of the LAST Inception layer (backward of conv1_2 and of M's ReLU) rides in the tail convolution's backward-data launch
            lastq, lastt = self.layers[-1], tape['layers'][-1]
            g_m_last = ps.blocks(nh)
            g_il = self.tail.bwd(ps, tape['il'], g_out, pw=(3, lastq['c12'].w, None, lastt['m'], g_m_last))
        else:
            g_il = self.tail.bwd(ps, tape['il'], g_out)
        g_a = None
        if len(self.layers) > 1:           # the extra skip: a receives g_il as well
            g_a = ps.blocks(self.C // B)
            for s, d in zip(g_il, g_a):
                _axpy(s, d, accumulate=False)
        g_i = g_il
        for li, (q, t) in enumerate(zip(reversed(self.layers), reversed(tape['layers']))):
            x = t['x']
            if fuse and li == 0:
                g_m = g_m_last
                q['c12'].wgrad(ps, t['m'], g_i[nh:])
            else:
                g_m = q['c12'].bwd(ps, t['m'], g_i[nh:], act=t['m'])
            # the weight gradients of conv0_1 and conv1_1 (same shape, independent) as ONE launch: alone each is one wave per SIMD
            pair = fuse and ps.defer is not None and ps.tile8t is not None and ps.n > 0
            g_h1 = q['c11'].bwd(ps, t['h1'], g_m, act=t['h1'], wgrad=not pair)
            g_h0 = q['c01'].bwd(ps, t['h0'], g_i[:nh], act=t['h0'], wgrad=not pair)
            if pair:
                c01, c11 = q['c01'].mod, q['c11'].mod
                ops.spconv_wgrad_wide2(t['h0'], g_i[:nh], c01.kernel.grad, c01.bias.grad.reshape(-1), t['h1'], g_m, c11.kernel.grad,
                                       c11.bias.grad.reshape(-1), ps.tile8t, ps.n, ps.defer, mul=ps.mul)
            # the layer's input gradient: the residual's share g_i rides in conv0_0's backward-data epilogue (+ res), conv1_0's share
            # is added last - and with it, for the block's first layer of a one-layer block, the ReLU mask of a = relu(first conv)
            last_mask = tape['a'] if (nl == 1 and li == nl - 1) else None
            if fuse:
                q['c10'].wgrad(ps, x, g_h1)
                g_x = q['c00'].bwd(ps, x, g_h0, res=g_i, act=last_mask, pw=(4, q['c10'].w, None, g_h1, None))
            else:
                g_x = q['c00'].bwd(ps, x, g_h0, res=g_i)
                q['c10'].bwd(ps, x, g_h1, act=last_mask, into=g_x, accumulate=True)
            g_i = g_x
        if g_a is not None:
            for s, d in zip(g_a, g_i):
                _axpy(s, d)
        if nl != 1:
            # g_i is the gradient of a = relu(first conv): mask it
            for g, ab in zip(g_i, tape['a']):
                _mask_inplace(ps, g, ab)
        return self.first.bwd(ps, tape['in'], g_i, need_input_grad=need_input_grad)


def _mask_inplace(ps, g, act):
    """g *= (act > 0) through the pointwise kernel's ReLU-mask epilogue on an identity-free path: g = 0 * W + g masked."""
    # linr_linear_bwd_data with cin = cout = 8, a zero weight block, accumulate and mask: out = (0 + old) * (act > 0)
    z = _zeros_w(ps.dev)
    _lin_bwd_data(g, z, 0, 8, 1, B, B, g, act=act, accumulate=True)


_ZW = {}


def _zeros_w(dev):
    key = str(dev)
    if key not in _ZW:
        _ZW[key] = torch.zeros(64, dtype=torch.float32, device=dev)
    return _ZW[key]


class WideNet:
    # the pointwise layers of an Inception layer in the convolutions' epilogues; False (LINR_WIDE_FUSE_PW=0, or set on an executor): one
    # launch per pointwise layer, the same bits
    fuse_pw = os.environ.get('LINR_WIDE_FUSE_PW', '1') != '0'
    # the full-range inference forward (stages 0..8, no tape) as one C call (csrc/wide_fwd.hip: forward_c below); False
    # (LINR_WIDE_C_FORWARD=0, or set on an executor): the Python schedule, the same launches and the same bits
    c_forward = os.environ.get('LINR_WIDE_C_FORWARD', '1') != '0'
    # opt-in (LINR_WIDE_C_STEP=1, or set on an executor): the training step (forward with the tape, backward, Adam) as one C call
    # (csrc/wide_train.hip: model_core.train_step) - the same launches and bits as forward(keep=True) / backward / FlatAdam.step below,
    # which stay the default; quantisation-aware steps exist on the C call only
    c_step = os.environ.get('LINR_WIDE_C_STEP', '0') == '1'

    def __init__(self, model, hidden):
        if hidden % 16 != 0 or hidden > 32:
            raise ValueError('hidden_channel_conv must be 8 (the tuned kernels) or 16 / 32 (channel-blocked executor), got %d' % hidden)
        self.model, self.C = model, hidden
        self._built = False
        self._pool = None
        self._step_arena = None            # the arena of the C training step: grows to the largest frame seen, follows the device
        # one thread at a time per model: the pool, _build() and the bf16 state are per-model state (train_step holds it across forward,
        # backward and the optimiser step)
        self.lock = threading.RLock()

    def _build(self):
        up = self.model.upsampler
        C = self.C
        self.block_in = _Block(up.block_in, C)
        self.outter = [_Block(b, C) for b in up.outter_blocks]
        self.prune = [_Conv(p[0].conv) for p in up.prune_blocks]
        self.heads = [(mlp[0][0], mlp[0][2]) for mlp in up.inner_mlps]          # PointwiseMLP([C, 24, 1]) = Linear, ReLU, Linear
        self._bf = None                    # the bf16 executor's state addresses the parameters by their offsets: rebuilt with them
        self._built = True

    # ---- shared pieces ------------------------------------------------------------------------------------------------
    def _train_mul(self):
        """The products of a training pass: bf16 for train_precision 'bf16-mul' (csrc/wide_mul.hip), else fp32."""
        return 'bf16' if getattr(self.model, 'train_precision', 'f32') == 'bf16-mul' else 'f32'

    def _pass(self, frame, training, pool, defer=None):
        """The pass object of one call: a training pass (forward(keep=True), backward) multiplies as the model's train_precision says,
        every other forward in fp32."""
        return _Pass(frame, self._pool if pool else None, defer, self._train_mul() if training else 'f32', self.fuse_pw)

    def _scale_context(self, ps, frame, keep):
        """x0 [rows, 8] (one block): PointwiseMLP([15, 16, 8]) of the rows' scale on [emb | offset features] (model_core.py:48-53) - all
        scales in ONE launch of the library's scale-context kernel (linr_sce_fwd: the parameters of the scale context lead the flat
        parameter order whatever the width of the rest of the network); the hidden layer is kept for the backward pass."""
        x0 = ps.blocks(1)
        hid = torch.empty((frame.rows, 16), dtype=torch.float32, device=frame.device)
        check(_lib.lib().linr_sce_fwd(self.model.flat_parameters().data_ptr(), frame.cref(), None, hid.data_ptr(), x0[0].data_ptr(),
                                      _stream()), 'linr_sce_fwd')
        return x0, (hid if keep else None)

    def _occ_block(self, frame):
        return [frame.occ]                     # [rows, 8] view of a buffer with the zero row in front (engine.Frame)

    def _head(self, ps, k, prior, frame, p, partial):
        """Stage k behind `prior`: the prune convolution, then the head MLP + sigmoid (+ the stage's bits partials) as one launch."""
        c = self.prune[k].fwd(ps, prior)
        lin0, lin2 = self.heads[k]
        ops.head_wide_fwd(c, lin0.weight, lin0.bias, lin2.weight, lin2.bias, frame.occ[:, k] if partial is not None else None, p,
                          partial=partial)
        return c

    # ---- forward ---------------------------------------------------------------------------------------------------------
    def forward(self, frame, k0, k1, probs, bits, keep=False, pool=False):
        """Stages [k0, k1) teacher-forced on frame.occ (decoder: the columns decoded so far): probs [8, rows] rows k0..k1-1, bits
        (float64[1]) += their cost.  keep: record the activations for backward (k0 = 0, k1 = 8).  pool: the padded block buffers
        come from this executor's pool, i.e. they are valid until the NEXT pooled forward (train_step: forward, backward, done)."""
        with self.lock:
            if not self._built:
                self._build()
            if frame.rows == 0:
                return None
            if pool:
                if self._pool is None:
                    self._pool = _Pool()
                self._pool.reset()
            return self._forward(self._pass(frame, keep, pool), frame, k0, k1, probs, bits, keep)

    def _forward(self, ps, frame, k0, k1, probs, bits, keep):
        x0, sce_tape = self._scale_context(ps, frame, keep)
        xg, bin_tape = self.block_in.fwd(ps, x0)
        tape = {'sce': sce_tape, 'bin': bin_tape, 'xg': xg, 'stages': []} if keep else None
        nb = (frame.rows + 255) // 256                      # per-block bits partials of a stage (linr_head_wide_workspace_bytes / 8)
        parts = torch.empty(((k1 - k0) * nb,), dtype=torch.float64, device=frame.device) if bits is not None else None
        for k in range(k0, k1):
            blk_tape = None
            if k == 0:
                prior = xg
            else:
                occ = self._occ_block(frame)
                prior, blk_tape = self.outter[k - 1].fwd(ps, occ, res=xg)
            p = probs[k] if probs is not None else torch.empty((frame.rows,), dtype=torch.float32, device=frame.device)
            c = self._head(ps, k, prior, frame, p, None if parts is None else parts[(k - k0) * nb:(k - k0 + 1) * nb])
            if keep:
                tape['stages'].append({'prior': prior, 'c': c, 'p': p, 'blk': blk_tape})
        if parts is not None:
            ops.bits_finish(parts, (k1 - k0) * nb, bits)          # all stages' partials in one fixed-order pass
        return tape

    def forward_c(self, frame, probs, bits, bf16=False):
        """All 8 stages of forward() (keep=False) or forward_bf16() as ONE call into the library (linr_net_forward_wide[_bf16]): the
        same launches with the same arguments from a C schedule, on an arena of per-role blocks from _lib.scratch.  Nothing is kept on
        the executor and no lock is taken: calls of several threads, frames and models interleave freely."""
        if frame.rows == 0:
            return
        L, m = _lib.lib(), self.model
        need = int(L.linr_net_wide_arena_bytes(frame.rows, self.C, m.block_layers, 1 if bf16 else 0))
        ws = _lib.scratch(need + 64, frame.device)
        base = (ws.data_ptr() + 63) & ~63
        p, b = (0 if probs is None else probs.data_ptr()), (0 if bits is None else bits.data_ptr())
        if bf16:
            check(L.linr_net_forward_wide_bf16(frame.cref(), m._qcodes.data_ptr(), float(m._qrange[0]), float(m._qrange[1]), self.C, base,
                                               need, 0, 8, p, b, _stream()), 'linr_net_forward_wide_bf16')
        else:
            check(L.linr_net_forward_wide(frame.cref(), m.flat_parameters().data_ptr(), self.C, base, need, 0, 8, p, b, _stream()),
                  'linr_net_forward_wide')

    def step_arena(self, frame):
        """The arena of linr_net_train_step_wide for `frame`: one buffer per model (the steps of one model follow each other on its
        stream), re-made when a frame needs more than the largest so far or lives on another device."""
        need = int(_lib.lib().linr_net_wide_train_arena_bytes(frame.rows, self.C, self.model.block_layers)) + 64
        a = self._step_arena
        if a is None or a.numel() < need or a.device != frame.device:
            a = self._step_arena = _lib.scratch(need, frame.device)
        return a

    # ---- backward --------------------------------------------------------------------------------------------------------
    def backward(self, frame, tape, gscale, pool=False):
        """d (gscale * bits) / d params into the parameters' .grad (model._ensure_grad_views(): views of the flat gradient).
        pool: continue in the pool of the forward that made `tape`."""
        with self.lock:
            if not self._built:
                self._build()
            ps = self._pass(frame, True, pool, defer=[])
            self._backward(ps, frame, tape, gscale)
            ops.wide_reduce_many(ps.defer)          # the ~64 slab reductions of the pass, 32 per launch

    def _backward(self, ps, frame, tape, gscale):
        self.model._ensure_grad_views()
        C = self.C
        # the loss scale is a float, as it crosses the C-ABI as one (linr_step_args.gscale, linr_net_backward_wide): this schedule and
        # the C one differentiate the same loss.  d(bits)/d(nats) = 1 / ln 2, multiplied in double and rounded once by the call
        gz_scale = ctypes.c_float(float(gscale)).value * 1.4426950408889634
        g_xg = ps.blocks(C // B)
        # all 8 heads first, as one grouped launch (their inputs - c, p, the occupancy columns - exist once the forward has run): the
        # gradients of the prune convolutions' outputs and the heads' parameter gradients, straight into the flat gradient
        stages = tape['stages']
        g_cs = [ps.blocks(C // B) for _ in range(8)]
        first = self.heads[0][0].weight.grad
        per = 24 * C + 49
        for k, (lin0, lin2) in enumerate(self.heads):           # the reference's parameter order: the 8 inner_mlps back to back
            assert lin0.weight.grad.data_ptr() == first.data_ptr() + 4 * k * per and lin2.bias.grad.data_ptr() == \
                first.data_ptr() + 4 * (k * per + per - 1)
        off0 = (first.data_ptr() - self.model._flat_grad.data_ptr()) // 4
        ops.head_wide_bwd([st['c'] for st in stages], [st['p'] for st in stages], [frame.occ[:, k] for k in range(8)],
                          [h[0].weight for h in self.heads], [h[0].bias for h in self.heads], [h[1].weight for h in self.heads],
                          gz_scale, g_cs, self.model._flat_grad[off0:off0 + 8 * per])
        g_priors = []
        for k in range(7, -1, -1):
            st = stages[k]
            g_c = g_cs[k]
            if k == 0:
                self.prune[k].bwd(ps, st['prior'], g_c, into=g_xg, accumulate=False)
            else:
                g_prior = self.prune[k].bwd(ps, st['prior'], g_c)
                g_priors.append(g_prior)                            # prior_k = x_glob + block output: both receive g_prior
                self.outter[k - 1].bwd(ps, st['blk'], g_prior, need_input_grad=False)
        # x_glob's gradient: stage 0's (in g_xg) + the seven priors' - one pass per block instead of a read-modify-write pass per stage
        for b, dst in enumerate(g_xg):
            check(_lib.lib().linr_sum_many(ops._ptr_array([gp[b] for gp in g_priors]), len(g_priors), dst.numel(), dst.data_ptr(), 1,
                                           _stream()), 'linr_sum_many')
        g_x0 = self.block_in.bwd(ps, tape['bin'], g_xg, need_input_grad=True)[0]
        # scale context: ghid, the four parameter gradients of every scale's MLP and the embedding rows in one call, straight into the
        # flat gradient (its leading linr_sce_param_count floats)
        L = _lib.lib()
        m = self.model
        slab = _lib.scratch(L.linr_sce_bwd_params_slab_bytes(m.scale_num), frame.device)
        check(L.linr_sce_bwd_params(m.flat_parameters().data_ptr(), frame.cref(), g_x0.data_ptr(), tape['sce'].data_ptr(), slab.data_ptr(),
                                    slab.numel(), m._flat_grad.data_ptr(), _stream()), 'linr_sce_bwd_params')

    # ---- bf16 / uint8-weight inference forward (csrc/wide_bf16.hip) ----------------------------------------------------------
    def forward_bf16(self, frame, k0, k1, probs, bits):
        """_forward's schedule on the bf16 executor: the model is its uint8 codes (model._qcodes / _qrange), de-quantised by one prologue
        launch per call; bf16 channel-blocked activations from a pool of per-role buffers; no tape.  Stages [k0, k1) as in forward():
        the decoder's one-stage calls run the same launches as the encoder's [0, 8), so their probabilities are bit-identical."""
        with self.lock:
            if frame.rows == 0:
                return
            m = self.model
            st = self._bf16_state(frame.device)
            ops.wide_bf16_prep(m._qcodes, m._qrange, st['tab'], st['n_conv'], st['n_img'], st['pf'], st['img'])
            n, dev, L = frame.rows, frame.device, _lib.lib()
            x0 = st['pool'].take('x0', n, 1, dev)
            ops.sce_fwd_bf16(st['pf'], frame, x0[0] - 16)
            occ = st['pool'].take('occ', n, 1, dev)         # converted on every call: the decoder fills frame.occ column by column
            check(L.linr_occ_to_bf16(frame.occ.data_ptr(), n, occ[0] - 16, _stream()), 'linr_occ_to_bf16')
            xg = self._block_bf16(frame, st, st['blocks'][0], x0, 'bin', None)
            nb = (n + 255) // 256
            parts = torch.empty(((k1 - k0) * nb,), dtype=torch.float64, device=dev) if bits is not None else None
            for k in range(k0, k1):
                prior = xg if k == 0 else self._block_bf16(frame, st, st['blocks'][k], occ, 'out', xg)
                p = probs[k] if probs is not None else torch.empty((n,), dtype=torch.float32, device=dev)
                h = st['heads'][k]
                ops.head_wide_bf16(prior, self.C, frame.nbr_lo, frame.nbr_mask, n, h['img'], h['bias'], h['w1'], h['b1'], h['w2'], h['b2'],
                                   frame.occ.data_ptr(), k, p, None if parts is None else parts[(k - k0) * nb:(k - k0 + 1) * nb])
            if parts is not None:
                ops.bits_finish(parts, (k1 - k0) * nb, bits)

    def _block_bf16(self, frame, st, bd, xin, tag, res):
        """make_block on bf16 blocks: conv3 -> ReLU -> Inception layers (conv1_0 in conv0_0's epilogue, conv1_2 + the residual in conv1_1's,
        the extra skip of models/resnet.py:160-161 in the last layer's two launches) -> conv3 (+ res: x_glob)."""
        n, dev, C = frame.rows, self.model._flat.device, self.C
        lo, mask = frame.nbr_lo, frame.nbr_mask
        nbC, nh, h = C // B, C // (2 * B), C // 2
        pool = st['pool']
        conv = ops.spconv_wide_bf16
        a = pool.take(tag + 'a', n, nbC, dev)
        conv(0, xin, bd['cin'], lo, mask, n, bd['first'][0], bd['first'][1], C, a, relu=True)
        x, nl = a, len(bd['layers'])
        for li, q in enumerate(bd['layers']):
            skip = a if (nl > 1 and li == nl - 1) else None
            H = pool.take(tag + 'h%d' % li, n, nbC, dev)
            I = pool.take(tag + 'i%d' % li, n, nbC, dev)
            conv(1, x, C, lo, mask, n, q['c00'][0], q['c00'][1], h, H, pw=q['c10'])
            conv(0, H, h, lo, mask, n, q['c01'][0], q['c01'][1], h, I, res=x, res2=skip)
            conv(2, _sub(H, nh), h, lo, mask, n, q['c11'][0], q['c11'][1], h, _sub(I, nh), res=_sub(x, nh),
                 res2=None if skip is None else _sub(skip, nh), pw=q['c12'])
            x = I
        o = pool.take(tag + 'o', n, nbC, dev)
        conv(0, x, C, lo, mask, n, bd['tail'][0], bd['tail'][1], C, o, res=res)
        return o

    def _bf16_state(self, dev):
        """Per model and device: the convolution table of the prologue, the de-quantised fp32 parameters, the bf16 weight images and the
        activation pool.  Every parameter is addressed in the fp32 copy at its offset in the flat buffer (the codes follow that order)."""
        if not self._built:
            self._build()
        st = getattr(self, '_bf', None)
        if st is not None and st['dev'] == dev:
            return st
        L = _lib.lib()
        flat = self.model._flat
        pf = _lib.scratch(4 * flat.numel(), dev).view(torch.float32)
        convs = []

        def off(t):
            return (t.data_ptr() - flat.data_ptr()) // 4

        def pfv(t):
            return pf[off(t):off(t) + t.numel()]

        def cv(mod):
            convs.append((off(mod.kernel), mod.kernel.shape[1], mod.kernel.shape[2]))
            return [len(convs) - 1, pfv(mod.bias)]

        def blk(b):
            return {'cin': b.first.ci, 'first': cv(b.first.mod), 'tail': cv(b.tail.mod),
                    'layers': [{'c00': cv(q['c00'].mod), 'c01': cv(q['c01'].mod), 'c11': cv(q['c11'].mod),
                                'c10': (pfv(q['c10'].w), pfv(q['c10'].b)), 'c12': (pfv(q['c12'].w), pfv(q['c12'].b))} for q in b.layers]}

        blocks = [blk(self.block_in)] + [blk(b) for b in self.outter]
        heads = [{'conv': cv(self.prune[k].mod), 'w1': pfv(l0.weight), 'b1': pfv(l0.bias), 'w2': pfv(l2.weight), 'b2': pfv(l2.bias)}
                 for k, (l0, l2) in enumerate(self.heads)]
        starts, tot = [], 0
        for _, ci, co in convs:
            starts.append(tot)
            tot += int(L.linr_wide_bf16_image_elems(ci, co))
        img = _lib.scratch(8 * tot, dev)
        tab = torch.tensor([[w, ci, co, s] for (w, ci, co), s in zip(convs, starts)], dtype=torch.int64).to(dev)

        def fix(c):                                         # [conv index, bias] -> (image pointer, bias)
            return (img.data_ptr() + 8 * starts[c[0]], c[1])

        for b in blocks:
            b['first'], b['tail'] = fix(b['first']), fix(b['tail'])
            for q in b['layers']:
                q['c00'], q['c01'], q['c11'] = fix(q['c00']), fix(q['c01']), fix(q['c11'])
        for hd in heads:
            hd['img'], hd['bias'] = fix(hd.pop('conv'))
        self._bf = {'dev': dev, 'pf': pf, 'img': img, 'tab': tab, 'n_conv': len(convs), 'n_img': tot, 'blocks': blocks, 'heads': heads,
                    'pool': _Bf16Pool()}
        return self._bf


def _sub(t, j):
    """Blocks j.. of a blocked bf16 matrix given as (pointer of block 0's first row, block stride in elements)."""
    return (t[0] + 2 * j * t[1], t[1])


class _Bf16Pool:
    """The bf16 activation buffers of forward_bf16, one per role ('bin' / 'out' block slots, x0, occ), reused from call to call (all
    launches are on one stream, in order).  A buffer is [nb][cap + 1][8] bf16 whose row 0 is cleared once when it is made; a role is
    handed out as (pointer of block 0's first row, block stride)."""

    def __init__(self):
        self.bufs = {}

    def take(self, key, n, nb, dev):
        b = self.bufs.get(key)
        if b is None or b.shape[0] != nb or b.shape[1] < n + 1 or b.device != dev:
            b = torch.empty((nb, n + 1, B), dtype=torch.int16, device=dev)
            if os.environ.get('LINR_DEBUG_POISON'):
                b.fill_(-1)
            b[:, 0].zero_()
            self.bufs[key] = b
        return (b[0, 1].data_ptr(), b.stride(0))
