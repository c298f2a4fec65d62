"""The headline leg of bench.py: the timed fp32 overfit of BASELINE config[1]'s GOP (ramp, warm-up, K timed steps, the rest of the
overfit)."""
import ctypes   # noqa: F401
import json     # noqa: F401
import os
import sys      # noqa: F401
import time     # noqa: F401

import numpy as np   # noqa: F401
import torch

from .common import EPOCHS, PROF_EVERY, TABLE_STEPS, log, steps_done_so_far
from .roofline import KERNEL_CLASSES, _read_prof, kernel_roofline

class Headline:
    """The timed region: K steps of the per-GOP overfit (main.py:297-321) on this rank's GOP, then the rest of the complete overfit.
    Holds everything the timed loop touches (created before the ramp): the loss accumulators, the per-step events, the device-side
    best-epoch snapshot (the reference codes with the epoch of the lowest mean loss, main.py:413-426,440-451; tracked on the device
    so that the loop never waits for the host)."""

    def __init__(self, args, rank, L, _lib):
        from linr_pcgc_amd import overfit, synthetic
        from linr_pcgc_amd.model_core import FlatAdam, train_step
        self.args, self.L, self._lib, self.train_step = args, L, _lib, train_step
        # rank r owns GOP r of the sequence: frames [gop*r, gop*(r+1))  (GOPs are independent: no collective)
        t_setup = time.time()
        clouds = [synthetic.sequence_frame_device(args.config, rank * args.gop + t, 'cuda') for t in range(args.gop)]
        self.gop = gop = overfit.Gop(None, clouds, None, 64, 'cuda')
        del clouds
        self.model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807)
        self.init_sd = {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}
        self.init_flat = self.model.flat_parameters().detach().clone()           # device copy: the reset before t0 is one D2D copy
        self.setup_s = time.time() - t_setup
        log('setup done: %d frames, frame0 %d points / %d rows, %d scales' % (len(gop), gop.point_nums[0], gop.frames[0].rows,
            gop.scale_num))
        self.opt = FlatAdam(self.model)
        self.total_steps = EPOCHS * len(gop)
        self.prof_every = 1 if args.steps <= 32 else PROF_EVERY
        L.linr_prof_mask(3)                                       # timed region: the dominant kernel and the forward conv only
        _lib.check(L.linr_prof_enable(1), 'linr_prof_enable')     # creates the event pairs ...
        L.linr_prof_enable(0)                                     # ... and stops; sampled steps switch it on (mode 2)
        self.acc = torch.zeros(len(gop), dtype=torch.float64, device='cuda')
        self.acc_done = torch.zeros_like(self.acc)               # the previous epoch's per-frame bits (swapped with acc at an epoch end)
        self.pns = torch.tensor([float(pn) for pn in gop.point_nums], dtype=torch.float64, device='cuda')
        epoch_end = (self.acc / self.pns).sum()                   # loads the torch kernels the epoch end uses
        del epoch_end
        self.step_ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        self.epoch_loss = []
        self.flat = self.model.flat_parameters()
        self.best = {'loss': torch.full((), float('inf'), dtype=torch.float64, device='cuda'),
                     'epoch': torch.full((), -1, dtype=torch.int64, device='cuda'), 'p': self.flat.detach().clone(),
                     'm': self.opt.exp_avg.clone(), 'v': self.opt.exp_avg_sq.clone(), 'meta': []}

    def best_reset(self):
        self.best['loss'].fill_(float('inf'))
        self.best['epoch'].fill_(-1)
        self.best['meta'].clear()

    def best_offer(self, l):
        best, opt = self.best, self.opt
        better = l < best['loss']
        torch.where(better, self.flat.detach(), best['p'], out=best['p'])
        torch.where(better, opt.exp_avg, best['m'], out=best['m'])
        torch.where(better, opt.exp_avg_sq, best['v'], out=best['v'])
        best['epoch'].copy_(torch.where(better, torch.full_like(best['epoch'], len(best['meta'])), best['epoch']))
        best['loss'].copy_(torch.minimum(best['loss'], l))
        best['meta'].append((opt.t, opt.t_scale.copy(), opt.lr, opt.sched_steps))

    def body(self, i, sample):
        """One iteration of the timed loop - warm-up and ramp run exactly this."""
        gop = self.gop
        j = i % len(gop)
        if sample:
            self.L.linr_prof_enable(2)
        self.train_step(self.model, self.opt, gop.frames[j], gop.point_nums[j],
            out=self.acc[j:j + 1])      # bits of frame j into its own slot
        if sample:
            self.L.linr_prof_enable(0)
        if j == len(gop) - 1:
            l = (self.acc / self.pns).sum()                 # like overfit.overfit_gop: per-epoch loss, no per-step torch kernels
            self.best_offer(l)                              # before the clamp, as the reference saves (main.py:413-437)
            self.opt.clamp_lr(4e-4)
            self.epoch_loss.append(l)
            self.acc, self.acc_done = self.acc_done, self.acc
            self.acc.zero_()

    def run(self, barrier, dist):
        """Ramp + W warm-up steps, reset in place, the K timed steps, then the rest of the complete overfit (second timed region)."""
        args, L = self.args, self.L
        # a fresh box starts at idle clocks (sclk level 1): ramp the device with ~1 s of the same steps before the W warm-up
        # steps, otherwise the first few hundred timed steps run ~10 % slow (measured: 3.22 vs 2.92 ms/step)
        t_ramp, i_ramp = time.time(), 0
        while time.time() - t_ramp < args.ramp_s:
            for _ in range(32):
                self.body(i_ramp, i_ramp % self.prof_every == 0)
                i_ramp += 1
            torch.cuda.synchronize()
        for i in range(args.warmup):
            self.body(i, i % self.prof_every == 0)
        # reset to the seeded initialisation IN PLACE (one D2D copy + three memsets on the stream; nothing is allocated and
        # the host does not wait), drop the warm-up's samples
        self.model.flat_parameters().copy_(self.init_flat)
        self.opt.reset()
        self.acc.zero_()
        self.epoch_loss.clear()
        self.best_reset()
        barrier()
        L.linr_prof_enable(1)                                     # clears the records (the events are reused, none is created)
        L.linr_prof_enable(0)
        log('warm-up done (%d ramp + %d warm-up steps)' % (i_ramp, args.warmup))
        barrier()
        t0 = time.time()
        self.step_ev[0].record()
        for i in range(args.steps):
            self.body(i, i % self.prof_every == 0)
            self.step_ev[i + 1].record()
        barrier()
        elapsed = time.time() - t0
        per_step_ms = [self.step_ev[i].elapsed_time(self.step_ev[i + 1]) for i in range(args.steps)]
        self.live = _read_prof(L, self._lib)
        self.last_step = None
        if args.dump_outputs:
            # what the caller of the last timed step received (between the two timed regions): the bits of its frame and the
            # parameters / Adam moments it left behind
            j = (args.steps - 1) % len(self.gop)
            bits = (self.acc_done if j == len(self.gop) - 1 else self.acc)[j:j + 1]
            self.last_step = {'bits': bits.clone(), 'parameters': self.flat.detach().clone(),
                              'adam_exp_avg': self.opt.exp_avg.clone(), 'adam_exp_avg_sq': self.opt.exp_avg_sq.clone()}
        # carry the overfit on to its full length (second timed region) so that bits/point and value describe one training
        rest = max(0, self.total_steps - args.steps)
        barrier()
        t1 = time.time()
        for i in range(args.steps, args.steps + rest):
            self.body(i, False)
        # leave model and optimiser in the state of the best epoch (what the reference's model.pth holds) - inside the timed region
        best, opt = self.best, self.opt
        self.coded_epoch = int(best['epoch'])
        if 0 <= self.coded_epoch < len(best['meta']) and steps_done_so_far(args.steps, rest, self.total_steps):
            self.flat.detach().copy_(best['p'])
            opt.exp_avg.copy_(best['m'])
            opt.exp_avg_sq.copy_(best['v'])
            opt.t, opt.t_scale, opt.lr, opt.sched_steps = (best['meta'][self.coded_epoch][0], best['meta'][self.coded_epoch][1].copy(),
                                                           best['meta'][self.coded_epoch][2], best['meta'][self.coded_epoch][3])
        barrier()
        rest_s = time.time() - t1
        if dist is not None:
            t = torch.tensor([elapsed, rest_s], dtype=torch.float64, device='cuda')
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed, rest_s = float(t[0]), float(t[1])
        self.elapsed, self.rest_s = elapsed, rest_s
        self.ms_per_step = elapsed * 1e3 / args.steps
        self.steps_done = args.steps + rest
        # steps > total: scaled back to one overfit
        self.full_overfit_s = (elapsed + rest_s) * (self.total_steps / float(self.steps_done))
        self.losses = [float(x) / len(self.gop) for x in self.epoch_loss]
        srt = sorted(per_step_ms)
        self.step_stats = {'min': round(srt[0], 4), 'median': round(srt[len(srt) // 2], 4), 'max': round(srt[-1], 4),
                           'first8': [round(x, 3) for x in per_step_ms[:8]], 'sum_over_wall': round(sum(per_step_ms) / (elapsed * 1e3), 4)}
        log('timed %d steps: %.3f ms/step (events: min %.3f median %.3f max %.3f); full overfit %d steps %.3f s; epoch losses %s'
            % (args.steps, self.ms_per_step, srt[0], srt[len(srt) // 2], srt[-1], self.steps_done, elapsed + rest_s,
               ['%.4f' % x for x in self.losses]))

    def kernel_table_leg(self):
        """Per-kernel table: TABLE_STEPS more steps with every launch of a step bracketed by an event pair (outside every timed region;
        parameters and optimiser state are saved and put back, so the codec leg codes the model of the complete overfit)."""
        L, opt = self.L, self.opt
        snap = (self.model.flat_parameters().detach().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.t, opt.t_scale.copy(),
                opt.lr, opt.sched_steps)
        n_loss = len(self.epoch_loss)
        L.linr_prof_mask(0xFFFFFFFF)
        L.linr_prof_enable(1)
        for i in range(TABLE_STEPS):
            self.body(i, False)
        L.linr_prof_enable(0)
        torch.cuda.synchronize()
        table_prof = _read_prof(L, self._lib)
        L.linr_prof_mask(3)
        self.model.flat_parameters().copy_(snap[0])
        opt.exp_avg.copy_(snap[1])
        opt.exp_avg_sq.copy_(snap[2])
        opt.t, opt.t_scale, opt.lr, opt.sched_steps = snap[3], snap[4], snap[5], snap[6]
        self.acc.zero_()
        del self.epoch_loss[n_loss:]
        torch.cuda.synchronize()
        return table_prof
