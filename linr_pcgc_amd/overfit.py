"""Per-GOP overfitting on the fast path: mirror of main.overfit_one_gop's hot loop (main.py:297-437).

The reference re-reads a pickle from disk, rebuilds ~60 coordinate maps per scale and synchronises with the host
~20 times per scale-step.  Here every frame of the GOP is resident in HBM (kernel map, features,
occupancy), a step is one stream-ordered launch sequence (forward, backward, fused Adam) and the host reads the loss
once per epoch.
"""
import os

import torch

from .model_core import LINR_PCGC_Model, train_step
from .module_utils import prepare_frame


def gen_model(scale_num, device='cuda', seed=None, block_layers=1, hidden=8):
    """Gen_Model of main.py:97,218 (hidden = --hidden_channel_conv, main.py:520: 8 on the tuned kernels, 16 / 32 channel-blocked)."""
    if seed is not None:
        torch.manual_seed(seed)
    m = LINR_PCGC_Model({'scale_num': scale_num, 'in_channel': 7, 'hidden_channel_conv': hidden, 'block_layers': block_layers,
                         'outstage': 8, 'instage': 1})
    return m.to(device)


class Gop:
    """A group of pictures resident on one GPU: per frame the batched multi-scale Frame + side data."""

    def __init__(self, model, clouds, scale_num=None, min_point_num=64, device='cuda', block_layers=None):
        self.frames, self.point_nums, self.coord_mins, self.low_xyz, self.infos = [], [], [], [], []
        self.scale_num = scale_num
        for pts in clouds:
            fr = prepare_frame(pts, self.scale_num, min_point_num, device=device, with_offsets=False)
            if self.scale_num is None:
                self.scale_num = fr['scale_num']             # frozen from frame 0 (main.py:77-78)
            self.infos.append(fr)
        self.model_scale_num = model.scale_num if model is not None else self.scale_num
        if block_layers is None:
            block_layers = model.block_layers if model is not None else 1
        self.block_layers = int(block_layers)
        max_rows = 0
        from . import engine
        for fr in self.infos:
            f = engine.Frame(fr['all_input_info'], self.model_scale_num, device, validate=True, with_arena=False,
                             block_layers=self.block_layers)
            for i, sinfo in enumerate(fr['all_input_info']):      # the reference's per-scale dicts carry 'offset_tensor'
                sinfo['offset_tensor'] = f.offset_feat[f.scale_slice(i)]
                sinfo['xyzqsc_t'].offset_tensor = sinfo['offset_tensor']
            self.frames.append(f)
            self.point_nums.append(fr['point_num'])
            self.coord_mins.append(fr['coord_data_min'])
            self.low_xyz.append(fr['all_input_info'][-1]['coord'])
            max_rows = max(max_rows, f.rows)
        # one activation arena shared by all frames of the GOP (a step finishes before the next begins)
        from . import _lib
        arena = _lib.scratch(_lib.lib().linr_net_arena_bytes(max_rows, self.block_layers), device)
        for f in self.frames:
            f.arena = arena

    def share_train_bf16_arena(self, deep=False):
        """One arena of the bf16 training executor for all frames of the GOP (a step finishes before the next begins).  deep: the
        caller accepts block_layers 2..4 (Frame.train_bf16_arena); without it a deeper GOP is refused before any library call."""
        from . import _lib
        if self.block_layers > 1 and not deep:
            raise _lib.LinrError("the bf16 training executor supports block_layers=1 only (train_precision 'bf16-deep': 1..4)")
        if all(getattr(f, 'arena_train_bf16', None) is not None for f in self.frames):
            return
        nbytes = _lib.lib().linr_net_train_bf16_arena_bytes(max(f.rows for f in self.frames), self.block_layers)
        if nbytes == 0:
            raise _lib.LinrError('the bf16 training executor supports block_layers 1..4 through its deep entries only')
        arena = _lib.scratch(nbytes + 64, self.frames[0].device)
        for f in self.frames:
            f.arena_train_bf16 = arena

    def __len__(self):
        return len(self.frames)

    def subset(self, n):
        """A view of the first n frames (shares every buffer): warm-up runs, spot checks."""
        import copy
        g = copy.copy(self)
        g.frames, g.point_nums, g.coord_mins = self.frames[:n], self.point_nums[:n], self.coord_mins[:n]
        g.low_xyz, g.infos = self.low_xyz[:n], self.infos[:n]
        return g


def staging_split(config, frame_ids, device='cuda', scale_num=None, min_point_num=64):
    """Milliseconds per frame of the three staging steps, each timed synchronously on the given synthetic frames: the generator
    (stands in for file input), the octree levels (parents, child occupancy: module_utils.prepare_frame) and the kernel maps
    (engine.Frame: neighbour search, compressed map, tiled copy, 7-neighbour features).  Measurement aid of bench.py / tools."""
    import time
    from . import engine, synthetic
    t = {'generator': 0.0, 'octree': 0.0, 'kernel_map': 0.0}
    n = 0
    for i in frame_ids:
        torch.cuda.synchronize()
        t0 = time.time()
        pts = synthetic.sequence_frame_device(config, i, device)
        torch.cuda.synchronize()
        t1 = time.time()
        fr = prepare_frame(pts, scale_num, min_point_num, device=device, with_offsets=False)
        torch.cuda.synchronize()
        t2 = time.time()
        f = engine.Frame(fr['all_input_info'], fr['scale_num'], device, validate=True, with_arena=False)
        torch.cuda.synchronize()
        t3 = time.time()
        t['generator'] += t1 - t0
        t['octree'] += t2 - t1
        t['kernel_map'] += t3 - t2
        n += 1
        del f, fr, pts
    out = {k: round(v * 1e3 / max(n, 1), 3) for k, v in t.items()}
    out['total_without_generator'] = round(out['octree'] + out['kernel_map'], 3)
    out['frames'] = n
    return out


class BestState:
    """Device-side snapshot of (parameters, Adam moments, counters, lr) of the best epoch so far - what the reference keeps in
    model.pth: it saves the checkpoint only when the epoch's mean loss improves (main.py:413-426,440-451), so the encoder codes
    with, and the GOPs >= 1 warm-start from, the BEST epoch of an overfit, not the last one.  One D2D copy of 3 x n_params floats."""

    def __init__(self, model, opt):
        self.model, self.opt = model, opt
        self.params = torch.empty_like(model.flat_parameters())
        self.exp_avg, self.exp_avg_sq = torch.empty_like(opt.exp_avg), torch.empty_like(opt.exp_avg_sq)
        self.epoch, self.loss, self.meta = -1, float('inf'), None

    def offer(self, epoch, loss):
        """Called at the end of an epoch, BEFORE the lr clamp (the reference saves first, main.py:413-437)."""
        if not loss < self.loss:
            return False
        self.params.copy_(self.model.flat_parameters())
        self.exp_avg.copy_(self.opt.exp_avg)
        self.exp_avg_sq.copy_(self.opt.exp_avg_sq)
        self.epoch, self.loss = epoch, loss
        self.meta = (self.opt.t, self.opt.t_scale.copy(), self.opt.lr, self.opt.sched_steps)
        return True

    def restore(self):
        if self.meta is None:
            return
        self.model.flat_parameters().copy_(self.params)
        self.opt.exp_avg.copy_(self.exp_avg)
        self.opt.exp_avg_sq.copy_(self.exp_avg_sq)
        self.opt.t, self.opt.t_scale, self.opt.lr, self.opt.sched_steps = self.meta[0], self.meta[1].copy(), self.meta[2], self.meta[3]


def qat_first_epoch(epochs, qat_epochs):
    """The first quantisation-aware epoch of an overfit of `epochs` epochs whose last min(qat_epochs, epochs) are; `epochs` (no
    such epoch) when qat_epochs is 0."""
    if qat_epochs < 0:
        raise ValueError('qat_epochs must be >= 0, got %d' % qat_epochs)
    return max(0, int(epochs) - int(qat_epochs))


AVG_MAX_DECAYS = 4            # LINR_AVG_MAX of csrc/params_avg.h: the rows of one linr_params_average call


def avg_weights(decays):
    """The update weights of the averaged iterates (overfit_gop avg_decays=): for every decay d in [0, 1) the fp32 weight
    w = (float)(1 - d) of  avg += w * (params - avg);  at most AVG_MAX_DECAYS of them.  Returns a float32 array; the decay that is
    really applied is 1 - (double)w (avg_debias_scales uses that one).  None or no decay: an empty array."""
    import numpy as np
    d = [] if decays is None else [float(x) for x in decays]
    if len(d) > AVG_MAX_DECAYS:
        raise ValueError('at most %d averaging decays, got %d' % (AVG_MAX_DECAYS, len(d)))
    w = np.asarray([1.0 - x for x in d], dtype=np.float32)
    for x, wk in zip(d, w):
        if not (0.0 <= x < 1.0) or not (0.0 < float(wk) <= 1.0):
            raise ValueError('an averaging decay must be in [0, 1) (and 1 - decay a positive float32), got %r' % (x,))
    return w


def avg_debias_scales(weights, steps):
    """The scales that turn exponential averages accumulated from zero over `steps` updates into averages whose weights sum to one:
    (float)(1 / (1 - d^steps)) with d = 1 - (double)w, formed in double, applied as ONE fp32 multiply per element."""
    import numpy as np
    if steps < 1:
        raise ValueError('a debiased average needs one update or more, got %d' % steps)
    return np.asarray([1.0 / (1.0 - (1.0 - float(w)) ** int(steps)) for w in weights], dtype=np.float32)


def _averages_info(decays, weights, rows, n, steps):
    """info['averages'] of overfit_gop: the debiased averages as a device [K][n] tensor (torch's elementwise multiply is one IEEE fp32
    multiply per element); no update at all (0 epochs): the zero rows."""
    import numpy as np
    scales = torch.from_numpy(avg_debias_scales(weights, steps) if steps > 0 else np.ones(len(weights), np.float32)).to(rows.device)
    return {'decays': [float(d) for d in decays], 'steps': int(steps), 'params': rows[:, :n] * scales[:, None]}


# opt-in (LINR_C_OVERFIT=1, or overfit_gop(c_loop=True)): the whole overfit of a GOP as ONE C call (csrc/overfit.hip: linr_overfit_gop)
C_OVERFIT = os.environ.get('LINR_C_OVERFIT', '0') == '1'


def _overfit_gop_c(model, opt, gop, epochs, min_lr, keep, info, qat_epochs, qat_from, qat_bitdepth, avg=None):
    """overfit_gop's loop as one call of linr_overfit_gop: the same launches and the same host doubles, one synchronisation."""
    import math
    from . import _lib, engine
    from .model_core import TRAIN_PRECISIONS
    tp = model.train_precision
    if tp not in TRAIN_PRECISIONS:
        raise ValueError('train_precision must be one of ' + ', '.join(repr(p) for p in TRAIN_PRECISIONS))
    if model._wide is not None and tp in ('bf16', 'bf16-deep'):
        raise _lib.LinrError('the bf16 training executor exists for hidden_channel_conv=8 only')
    if model._wide is None and tp == 'bf16-mul':
        raise _lib.LinrError("train_precision 'bf16-mul' exists for hidden_channel_conv 16 / 32 only: width 8 has the bf16 training executor")
    big = max(gop.frames, key=lambda f: f.rows)
    extra = {}
    if model._wide is not None:          # whatever WideNet.c_step says: the C step is what the call runs
        w = model._wide
        a = w.step_arena(big)
        base = (a.data_ptr() + 63) & ~63
        nbytes = a.numel() - (base - a.data_ptr())
        executor = _lib.LINR_OVERFIT_WIDE
        extra = {'hidden': w.C, 'flags': _lib.LINR_MUL_BF16 if w._train_mul() == 'bf16' else 0}
    elif tp == 'f32':
        arenas = {f.arena.data_ptr() for f in gop.frames if f.arena is not None}
        if len(arenas) != 1 or any(f.arena is None for f in gop.frames):
            raise _lib.LinrError('overfit_gop(c_loop=True) needs the frames of the GOP to share one arena (overfit.Gop)')
        base, nbytes, executor = big.arena.data_ptr(), min(f.arena.numel() for f in gop.frames), _lib.LINR_OVERFIT_F32
    else:
        base, nbytes = big.train_bf16_arena(tp == 'bf16-deep')          # the GOP's shared one (share_train_bf16_arena)
        executor = _lib.LINR_OVERFIT_BF16
        extra = {'occ_bf16': [f.occ_bf16() for f in gop.frames]}
    if qat_epochs:
        extra.update(qparams=model.qat_parameters(), qat_from=qat_from, bitdepth=int(qat_bitdepth))
    if avg is not None:          # (weights, rows): linr_overfit_gop_avg zeroes the rows and updates them behind every step
        extra['avg'] = avg
    losses, best_epoch, best_loss, t, sched, lr, t_scale = engine.overfit_gop(
        gop.frames, gop.point_nums, executor, model.flat_parameters(), opt.exp_avg, opt.exp_avg_sq, base, nbytes, epochs, opt.lr, min_lr,
        opt.gamma, opt.step_size, opt.t, opt.sched_steps, opt.t_scale, opt.betas[0], opt.betas[1], opt.eps, opt.weight_decay,
        keep_best=keep == 'best', **extra)
    opt.t, opt.sched_steps, opt.lr = t, sched, lr
    opt.t_scale = t_scale.astype(opt.t_scale.dtype)
    losses = [float(x) for x in losses]
    if (keep == 'best' and best_epoch < 0 and losses) or (keep != 'best' and losses and not math.isfinite(losses[-1])):
        err = FloatingPointError('the overfit diverged: epoch losses %s (no finite epoch to keep; learning rate %g)'
                                 % (['%.4g' % x for x in losses], opt.lr))
        err.losses = losses          # (run.py writes the epochs' records from them: no on_epoch has seen them)
        raise err
    if info is not None:
        info['coded_epoch'] = best_epoch if keep == 'best' else epochs - 1
        info['coded_loss'] = best_loss if keep == 'best' else (losses[-1] if losses else None)
        if qat_epochs:
            info['qat_from'] = qat_from
    return losses


def overfit_gop(model, opt, gop, epochs, min_lr=4e-4, on_epoch=None, keep='best', info=None, qat_epochs=0, qat_bitdepth=8, c_loop=None,
                avg_decays=None):
    """main.py:297-437: frames in fixed order, one optimiser + StepLR step per frame, lr clamp after each epoch.
    keep='best' (the reference's policy, main.py:413-426,440-451): model and optimiser are left in the state at the end of the epoch
    with the lowest mean loss; keep='last': in the state after the last epoch.  Returns the per-epoch mean loss (bits per point),
    like the reference logs; `info` (a dict) receives 'coded_epoch' and 'coded_loss'.
    qat_epochs > 0 (opt-in; 0 is the plain overfit, untouched): the last min(qat_epochs, epochs) epochs are quantisation-aware
    (train_step qat_bitdepth=): their loss is the rate of the weights encode_gop will code with at `qat_bitdepth` bits.  With
    keep='best' only those epochs compete - the loss of a plain epoch belongs to weights that are never coded.  The state left
    behind is the fp32 master either way; `info` also receives 'qat_from', the first quantisation-aware epoch.
    c_loop (opt-in; None: LINR_C_OVERFIT=1, read once): the loop below as ONE C call (linr_overfit_gop) that queues every step of
    every epoch and synchronises once - the same launches and the same host doubles, so parameters, moments and counters are those of
    the loop; the returned losses are summed in frame order instead of torch's reduction order (a few ulp).  Wide models then run
    their one-call step whatever WideNet.c_step says.  Epochs cannot be observed from outside the call: on_epoch is refused.
    avg_decays (opt-in; None or empty: today's launches and no others): up to 4 decays d in [0, 1).  For each an exponential average of
    the iterates is kept on the device - a zeroed [K][stride] buffer when the overfit starts, ONE linr_params_average launch queued
    behind every train_step, on model.flat_parameters() (the fp32 master of every executor) - and `info` receives
    'averages' = {'decays', 'steps' (the updates made), 'params' (device [K][n]: the debiased averages at the end of the last epoch,
    whatever epoch is kept)}: candidates for codec.encode_gop(avg=).  Training is untouched, bit for bit; c_loop=True runs
    linr_overfit_gop_avg and returns the same averages."""
    if c_loop is None:
        c_loop = C_OVERFIT
    if c_loop and on_epoch is not None:
        raise ValueError('overfit_gop(c_loop=True) runs all epochs in one call: on_epoch cannot be served')
    if keep not in ('best', 'last'):
        raise ValueError("keep must be 'best' or 'last'")
    qat_from = qat_first_epoch(epochs, qat_epochs)
    if qat_epochs and not 2 <= int(qat_bitdepth) <= 16:
        raise ValueError('qat_bitdepth must be in 2..16, got %r' % (qat_bitdepth,))
    if getattr(model, 'train_precision', 'f32') in ('bf16', 'bf16-deep'):
        gop.share_train_bf16_arena(deep=model.train_precision == 'bf16-deep')
    avg_w = avg_weights(avg_decays)
    avg_rows, n_params = None, model.flat_parameters().numel()
    if len(avg_w):
        avg_rows = torch.zeros((len(avg_w), (n_params + 3) & ~3), dtype=torch.float32, device=model.flat_parameters().device)
    if c_loop:
        losses = _overfit_gop_c(model, opt, gop, epochs, min_lr, keep, info, qat_epochs, qat_from, qat_bitdepth,
                                None if avg_rows is None else (avg_w, avg_rows))
        if avg_rows is not None and info is not None:
            info['averages'] = _averages_info(avg_decays, avg_w, avg_rows, n_params, epochs * len(gop))
        return losses
    from . import engine
    losses = []
    dev = gop.frames[0].device
    bits = torch.zeros(len(gop), dtype=torch.float64, device=dev)         # one slot per frame: no per-step torch kernels
    pns = torch.tensor([float(pn) for pn in gop.point_nums], dtype=torch.float64, device=dev)
    best = BestState(model, opt) if keep == 'best' else None
    for epoch in range(epochs):
        bits.zero_()
        for j, (f, pn) in enumerate(zip(gop.frames, gop.point_nums)):
            if epoch >= qat_from:
                train_step(model, opt, f, pn, out=bits[j:j + 1], qat_bitdepth=qat_bitdepth)
            else:
                train_step(model, opt, f, pn, out=bits[j:j + 1])
            if avg_rows is not None:
                engine.params_average(model.flat_parameters(), avg_w, avg_rows)
        # the only host sync of the epoch.  Non-finite parameters make the epoch count as diverged (loss = inf): the loss itself
        # would not show them - BCELoss's clamp at -100 (models/model_core.py:76-81) turns a NaN probability into 100 nats
        val = (bits / pns).sum() / len(gop)
        loss_mean = float(torch.where(torch.isfinite(model.flat_parameters()).all(), val, torch.full_like(val, float('inf'))))
        if best is not None and (not qat_epochs or epoch >= qat_from):
            best.offer(epoch, loss_mean)
        opt.clamp_lr(min_lr)
        losses.append(loss_mean)
        if on_epoch is not None:
            on_epoch(epoch, loss_mean)
    import math
    if (best is not None and best.meta is None and losses) or (best is None and losses and not math.isfinite(losses[-1])):
        raise FloatingPointError('the overfit diverged: epoch losses %s (no finite epoch to keep; learning rate %g)'
                                 % (['%.4g' % x for x in losses], opt.lr))
    if best is not None:
        best.restore()          # also when the last epoch is the best: the checkpoint holds the lr from before the clamp
    if info is not None:
        info['coded_epoch'] = best.epoch if best is not None else epochs - 1
        info['coded_loss'] = best.loss if best is not None else (losses[-1] if losses else None)
        if qat_epochs:
            info['qat_from'] = qat_from
        if avg_rows is not None:
            info['averages'] = _averages_info(avg_decays, avg_w, avg_rows, n_params, epochs * len(gop))
    return losses


def checkpoint(model, opt, epoch, loss, bitdepth=8):
    """main.py:365-374 checkpoint dict (same keys, torch.optim.Adam state format)."""
    return {'model': {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, 'epoch': epoch,
            'optimizer_state_dict': opt.state_dict(), 'loss': loss, 'bitdepth': bitdepth}


def warm_start(model, opt, ckpt):
    """main.py:241-248: GOPs >= 1 start from GOP 0's model AND optimiser state."""
    model.load_state_dict(ckpt['model'])
    opt.load_state_dict(ckpt['optimizer_state_dict'])
