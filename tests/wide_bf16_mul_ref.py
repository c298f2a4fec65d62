"""Emulation of train_precision 'bf16-mul' on the oracle (test infrastructure): oracle.network.conv3 with the operands of every PRODUCT
rounded to bf16 and everything else as it is -
    forward        out = bias + sum rb(x) rb(W)
    backward       gx = sum rb(g) rb(W)      gW = sum_rows rb(x) rb(g)      gb = sum g        (rb: round to nearest even to bf16)
as an autograd function, and a context manager that puts it in conv3's place for the oracle's network functions."""
import contextlib

import torch

from oracle import network as onet

_conv3 = onet.conv3


def rb(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _Conv3Mul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, nbr, kernel, bias):
        ctx.save_for_backward(x, nbr, kernel)
        return _conv3(rb(x), nbr, rb(kernel), bias)

    @staticmethod
    def backward(ctx, g):
        x, nbr, kernel = ctx.saved_tensors
        with torch.enable_grad():
            xr, wr = rb(x).detach().requires_grad_(), rb(kernel).detach().requires_grad_()
            y = _conv3(xr, nbr, wr, torch.zeros(1, kernel.shape[2], dtype=x.dtype, device=x.device))
            gx, gw = torch.autograd.grad(y, [xr, wr], rb(g))          # both linear in rb(g): products of rounded operands only
        return gx, None, gw, g.sum(0, keepdim=True)


def conv3_mul(x, nbr, kernel, bias):
    return _Conv3Mul.apply(x, nbr, kernel, bias)


@contextlib.contextmanager
def emulated():
    """Inside: every conv3 of oracle.network (make_block, inception, the prune convolutions) multiplies in bf16."""
    keep = onet.conv3
    onet.conv3 = conv3_mul
    try:
        yield
    finally:
        onet.conv3 = keep
