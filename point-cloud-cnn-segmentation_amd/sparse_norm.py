"""BatchNorm (+ residual) (+ ReLU) for the occupied-voxel path (csrc/sparse_bn.hip): the
normalisation / activation layer between the sparse convolutions of pcs_amd.sparse.

    bn = SparseBatchNorm(64, relu=True)           # nn.BatchNorm1d's parameters, buffers and state dict
    h = bn(conv(x, sv))                           # [V, C] -> relu(bn(.)), one statistics pass + one apply
    y = bn2(conv2(h, sv), residual=x)             # relu(bn(.) + x)
    block = SparseResBlock(64); y = block(x, sv)  # conv -> BN+ReLU -> conv -> BN(+ x)+ReLU

Build-defined like the rest of the voxel vocabulary (tests/sparse_norm_refs.py states it in numpy
and proves the statement against torch.nn.functional.batch_norm).  The statistics are taken over the
V rows of one level on one device, as nn.BatchNorm1d takes them over a batch.  Forward: a Welford
statistics pass and an apply pass; backward: a reduce pass (the ReLU gate, dz, the two column sums)
and an apply pass.  No atomics, fp32 arithmetic: forward and backward are bitwise reproducible.
"""
from __future__ import annotations

import ctypes as ct

import torch
from torch.autograd.function import once_differentiable

from . import _lib as L
from .sparse import SparseVoxels, SubMConv3d

MAX_CHANNELS = 1024


def _check_channels(c, x_dtype, out_dtype):
    e = 8 if torch.bfloat16 in (x_dtype, out_dtype) else 4
    if c < e or c % e or c > MAX_CHANNELS:
        side = "bf16 on either side" if e == 8 else "fp32"
        raise ValueError(f"sparse_batch_norm: {c} channels; a multiple of {e} ({side}) between {e} and "
                         f"{MAX_CHANNELS} is required (no zero padding: the parameters and running buffers would "
                         "have to be padded too)")


def _geometry(V, C):
    """(num_blocks, rows_per_block) of the two reductions (pcs_sparse_bn_geometry)."""
    nb = ct.c_int32(0)
    rpb = L.workspace("pcs_sparse_bn_geometry", V, C, ct.byref(nb))
    return nb.value, rpb


def _vec(t, name, C):
    if t.dtype != torch.float32 or t.shape != (C,) or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"sparse_batch_norm: {name} must be a contiguous fp32 [{C}] tensor on the device")
    return t


class _SparseBNFn(torch.autograd.Function):
    """y = act(gamma * (x - mean) * rstd + beta (+ residual)) over the rows of x [V, C]; mean / rstd
    of the batch (training: the running buffers are updated in place) or of the running buffers."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, residual, training, momentum, eps, relu, out_dtype):
        V, C = x.shape
        dev, st = x.device, L.stream_ptr(x.device)
        xdt = L.dtype_code(x.dtype, what="sparse_batch_norm: x")
        ydt = L.dtype_code(out_dtype, what="sparse_batch_norm: out_dtype")
        x = x.contiguous()
        res = residual.contiguous() if residual is not None else None
        gamma, beta = weight.detach().float().contiguous(), bias.detach().float().contiguous()
        y = torch.empty(V, C, dtype=out_dtype, device=dev)
        coef = torch.empty(4, C, dtype=torch.float32, device=dev)
        mean, rstd, scale, shift = coef[0], coef[1], coef[2], coef[3]
        nb, rpb = _geometry(V, C)
        if training:
            stats = torch.empty(nb, C, 2, dtype=torch.float32, device=dev)
            L.call("pcs_sparse_bn_stats", x, xdt, V, C, nb, rpb, stats, st)
            L.call("pcs_bn_fwd_finalize", stats, 1, V, C, nb, rpb, gamma, beta, None, running_mean, running_var,
                   float(momentum), float(eps), 1, mean, rstd, scale, shift, None, st)
        else:
            L.call("pcs_bn_eval_coefs", gamma, beta, running_mean, running_var, None, float(eps), C, scale, shift, st)
            if any(ctx.needs_input_grad):   # the backward's xhat is (x - running_mean) * rstd_running
                mean.copy_(running_mean)
                rstd.copy_(torch.rsqrt(running_var.double() + eps))
        L.call("pcs_sparse_bn_apply", x, xdt, res, scale, shift, int(relu), V, C, y, ydt, st)
        ctx.save_for_backward(x, y if relu else None, mean, rstd, gamma)
        ctx.cfg = (training, relu, xdt, ydt, nb, rpb, weight.dtype, bias.dtype)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, y, mean, rstd, gamma = ctx.saved_tensors
        training, relu, xdt, ydt, nb, rpb, wdtype, bdtype = ctx.cfg
        need_x, need_w, need_b, need_r = (ctx.needs_input_grad[i] for i in (0, 1, 2, 5))
        V, C = x.shape
        dev, st = x.device, L.stream_ptr(x.device)
        dy = dy.contiguous()
        if L.dtype_code(dy.dtype, what="sparse_batch_norm: the output gradient") != ydt:
            raise ValueError("sparse_batch_norm backward: the output gradient must have the output's dtype")
        dx = dw = db = None
        dz = torch.empty_like(dy) if relu else dy          # without a gate dz is dy itself
        if V == 0:
            zeros = torch.zeros(C, dtype=torch.float32, device=dev)
            return (x.new_empty(0, C) if need_x else None, zeros.to(wdtype) if need_w else None,
                    zeros.to(bdtype) if need_b else None, None, None, dz if need_r else None, None, None, None, None,
                    None)
        if relu or need_x or need_w or need_b:
            stats = torch.empty(nb, C, 2, dtype=torch.float32, device=dev)
            L.call("pcs_sparse_bn_bwd_reduce", dy, y, ydt, x, xdt, mean, rstd, int(relu), V, C, nb, rpb,
                   dz if relu else None, stats, st)
        if need_x or need_w or need_b:
            out = torch.empty(5, C, dtype=torch.float32, device=dev)
            alpha, beta_c, gamma_c, dgamma, dbeta = out[0], out[1], out[2], out[3], out[4]
            L.call("pcs_bn_bwd_finalize", stats, 1, V, C, nb, mean, rstd, gamma, None, alpha, beta_c, gamma_c, dgamma,
                   dbeta, None, None, st)
            if need_x:
                if not training:   # the statistics are constants: dx = scale * dz
                    out[1:3].zero_()
                dx = torch.empty_like(x)
                L.call("pcs_sparse_bn_bwd_apply", dz, ydt, x, xdt, alpha, beta_c, gamma_c, V, C, dx, st)
            dw = dgamma.to(wdtype) if need_w else None
            db = dbeta.to(bdtype) if need_b else None
        return dx, dw, db, None, None, dz if need_r else None, None, None, None, None, None


def sparse_batch_norm(x, weight, bias, running_mean, running_var, training, momentum=0.1, eps=1e-5, relu=False,
                      residual=None, out_dtype=None):
    """BatchNorm over the V rows of per-voxel features x [V, C] (bf16 or fp32), then + residual
    ([V, C] in out_dtype) when given, then ReLU when relu: nn.BatchNorm1d's semantics (biased
    variance for the normalisation; in training the running buffers, fp32 [C], are updated in place
    with the batch mean and the unbiased variance).  Returns [V, C] in out_dtype (default x.dtype).
    Gradients reach x, weight, bias and residual, in training and in eval mode."""
    if not x.is_cuda:
        raise RuntimeError("pcs_amd sparse_batch_norm runs on a HIP device only (no CPU fallback)")
    if x.dim() != 2:
        raise ValueError(f"sparse_batch_norm: x must be [V, C], got {list(x.shape)}")
    out_dtype = x.dtype if out_dtype is None else out_dtype
    L.dtype_code(x.dtype, what="sparse_batch_norm: x")
    L.dtype_code(out_dtype, what="sparse_batch_norm: out_dtype")
    V, C = x.shape
    _check_channels(C, x.dtype, out_dtype)
    if momentum is None:
        raise ValueError("sparse_batch_norm: momentum=None (a cumulative average) is not supported")
    if training and V < 2:
        raise ValueError(f"sparse_batch_norm: training needs at least 2 rows, got {V}")
    for name, t in (("weight", weight), ("bias", bias)):
        if t is None or t.shape != (C,) or not t.is_cuda:
            raise ValueError(f"sparse_batch_norm: {name} must be a [{C}] tensor on the device")
    _vec(running_mean, "running_mean", C), _vec(running_var, "running_var", C)
    if residual is not None and (residual.shape != x.shape or residual.dtype != out_dtype or not residual.is_cuda):
        raise ValueError(f"sparse_batch_norm: residual must be {list(x.shape)} in out_dtype ({out_dtype}), on the "
                         "device")
    return _SparseBNFn.apply(x, weight, bias, running_mean, running_var, residual, bool(training), momentum, eps,
                             bool(relu), out_dtype)


class SparseBatchNorm(torch.nn.BatchNorm1d):
    """nn.BatchNorm1d over per-voxel rows [V, C] with an optional fused residual add and ReLU.  The
    parameters, buffers, init and state dict are BatchNorm1d's own: state dicts load either way."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, relu=False, affine=True, track_running_stats=True,
                 device=None, dtype=None):
        if not affine or not track_running_stats or momentum is None:
            raise ValueError("SparseBatchNorm supports affine=True, track_running_stats=True and a numeric momentum "
                             "only")
        super().__init__(num_features, eps=eps, momentum=momentum, affine=True, track_running_stats=True, device=device,
                         dtype=dtype)
        self.relu = bool(relu)

    def forward(self, x, residual=None, out_dtype=None):
        if self.training:
            self.num_batches_tracked.add_(1)
        return sparse_batch_norm(x, self.weight, self.bias, self.running_mean, self.running_var, self.training,
                                 self.momentum, self.eps, self.relu, residual, out_dtype)

    def extra_repr(self):
        return super().extra_repr() + f", relu={self.relu}"


def conv_then_bn(conv, bn, *inputs, residual=None):
    """The unfused layer, bn(conv(*inputs), residual), with fold.conv_bn's signature."""
    return bn(conv(*inputs), residual=residual)


class SparseResBlock(torch.nn.Module):
    """SubMConv3d -> BN+ReLU -> SubMConv3d -> BN(+ x)+ReLU on bf16 per-voxel features [V, channels],
    identity shortcut.  The convolutions carry no bias: BatchNorm cancels it."""

    def __init__(self, channels):
        super().__init__()
        self.conv1, self.bn1 = SubMConv3d(channels, channels, bias=False), SparseBatchNorm(channels, relu=True)
        self.conv2, self.bn2 = SubMConv3d(channels, channels, bias=False), SparseBatchNorm(channels, relu=True)

    def _walk(self, layer, x, *at):
        """The block with layer(conv, bn, *inputs, residual=None) as its two layers: conv_then_bn or
        fold.conv_bn.  at: what the convolutions take after x (VoxelResBlock's take nothing)."""
        h = layer(self.conv1, self.bn1, x, *at)
        return layer(self.conv2, self.bn2, h, *at, residual=x)

    def forward(self, x, sv: SparseVoxels):
        return self._walk(conv_then_bn, x, sv)

    def infer(self, x, sv: SparseVoxels):
        """forward in eval mode with each BatchNorm folded into its convolution's store (fold.conv_bn):
        the running statistics whatever self.training says, no gradient, nothing updated."""
        from .fold import conv_bn   # (fold imports this module for SparseBatchNorm)
        return self._walk(conv_bn, x, sv)


__all__ = ["SparseBatchNorm", "SparseResBlock", "sparse_batch_norm"]
