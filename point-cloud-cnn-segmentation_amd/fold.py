"""Inference path of the voxel U-Nets: convolution -> BatchNorm in eval mode (+ residual) (+ ReLU) as
one kernel (include/pcs_fold.h, the EpiAffine epilogue of csrc/conv3d.hip).  f4, not reference parity:
build-defined like the rest of the voxel vocabulary.

    y = conv_bn(conv, bn, x, sv)                      # == bn.eval()(conv(x, sv, out_dtype=torch.float32))
    y = conv_bn(conv2, bn2, h, sv, residual=x)        # relu(bn2(conv2(h)) + x)
    labels = model.predict(rb)                        # SparseUNetSegmentation / VoxelUNetSegmentation

In eval mode the BatchNorm is a per-channel affine map of the convolution's fp32 sums, which the kernel
still holds in registers where it stores them: y = act(fmaf(acc, scale, shift) (+ residual)), rounded
once.  The unfused layer rounds the sums to bf16, writes [rows, C], and pcs_sparse_bn_apply reads that
array (and the residual) back and writes a second one.  The folded layer is bit-identical to the unfused
pair run with an fp32 intermediate (the same kernels, routes and summation order; the same fmaf and add),
so it is never less accurate than the unfused bf16 pair.  scale / shift come from the BatchNorm's
parameters and running buffers (pcs_bn_eval_coefs) whatever bn.training says; nothing is updated.

There is one forward per layer family (sparse._sparse_forward, _sparse_cat_forward; voxel._conv3d_forward,
_conv3d_cat_forward), as there is one kernel template per pcs_X / pcs_X_affine pair: it prepares the
operands, picks the route and launches through _lib.forward_call, which appends the epilogue when there is
one.  The layer's autograd Function calls it without, conv_bn (through the layer's _conv) with; this
module holds only conv_bn's checks and the epilogue itself.

Inference only: everything runs under torch.no_grad(), outputs never require grad, and an input that
requires grad while grad is enabled raises.  The bf16 weights are not rescaled (that would round them
again); the epilogue is exact fp32.
"""
from __future__ import annotations

from functools import partial

import torch

from . import _lib as L
from .sparse import SparseDownConv3d, SparseUpConv3d, SubMConv3d, SubMConv3dCat
from .sparse_norm import SparseBatchNorm, conv_then_bn
from .voxel import Conv3d, Conv3dCat, ConvTranspose3d, _pad_channels

CONVS = (SubMConv3d, SubMConv3dCat, SparseDownConv3d, SparseUpConv3d, Conv3d, ConvTranspose3d, Conv3dCat)


def _epilogue(bn, residual, out_dtype, cout, cout_k, out_shape, dev):
    """(scale, shift, R, relu) as L.forward_call hands them to a pcs_*_affine entry point: the eval
    coefficients of bn (its running buffers) and the residual.  A layer's forward asks for them (the
    last four arguments) once it knows its output: cout channels in out_shape, run as cout_k with the
    zero channels _conv_operands pads (zero coefficients and zero residual channels there)."""
    if bn.num_features != cout:
        raise ValueError(f"conv_bn: the BatchNorm has {bn.num_features} channels, the convolution {cout}")
    if residual is not None:
        if not isinstance(residual, torch.Tensor) or not residual.is_cuda or residual.dtype != out_dtype or \
                tuple(residual.shape) != tuple(out_shape):
            raise ValueError(f"conv_bn: residual must be {list(out_shape)} in out_dtype ({out_dtype}), on the device")
        residual = _pad_channels(residual, cout_k)
    gamma, beta = bn.weight.detach().float().contiguous(), bn.bias.detach().float().contiguous()
    coef = torch.zeros(2, cout_k, dtype=torch.float32, device=dev) if cout_k != cout else \
        torch.empty(2, cout, dtype=torch.float32, device=dev)
    own = coef if cout_k == cout else torch.empty(2, cout, dtype=torch.float32, device=dev)
    L.call("pcs_bn_eval_coefs", gamma, beta, bn.running_mean, bn.running_var, None, float(bn.eps), cout, own[0], own[1],
           L.stream_ptr(dev))
    if own is not coef:
        coef[:, :cout] = own
    return coef[0], coef[1], residual, int(bn.relu)


def conv_bn(conv, bn, *inputs, residual=None, out_dtype=torch.bfloat16):
    """bn in eval mode applied to conv(*inputs) (+ residual, then ReLU when bn.relu) as one kernel:
    bit-identical to bn.eval()(conv(*inputs, out_dtype=torch.float32), residual=residual,
    out_dtype=out_dtype) without the fp32 array.  conv: a SubMConv3d, SubMConv3dCat, SparseDownConv3d,
    SparseUpConv3d (pcs_amd.sparse) or Conv3d, ConvTranspose3d, Conv3dCat (pcs_amd.voxel); inputs: what
    its forward takes (without out_dtype); bn: a SparseBatchNorm / VoxelBatchNorm of the convolution's
    output channels, whose running buffers give scale / shift whatever bn.training says; residual: None
    or a tensor of the output's shape in out_dtype (bf16 or fp32).  The checks, the torch.cat fall-back
    and the pair-list / tile-gather route are the unfused layer's: it is that layer's forward, with the
    epilogue.  Inference only: the output never requires grad, and an input that requires grad while
    grad is enabled raises."""
    if not isinstance(bn, SparseBatchNorm):
        raise TypeError(f"conv_bn: bn must be a SparseBatchNorm or VoxelBatchNorm, got {type(bn).__name__}")
    if not isinstance(conv, CONVS):
        raise TypeError(f"conv_bn: conv must be one of {', '.join(c.__name__ for c in CONVS)}, got {type(conv).__name__}")
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (*inputs, residual)):
        raise RuntimeError("conv_bn is inference only and has no backward: an input requires grad (detach it, or call "
                           "under torch.no_grad())")
    L.dtype_code(out_dtype, what="out_dtype")
    # one source or two, then a sparse layer's level or link
    want = 1 + isinstance(conv, (SubMConv3dCat, Conv3dCat)) + (not isinstance(conv, (Conv3d, ConvTranspose3d, Conv3dCat)))
    if len(inputs) != want:
        raise TypeError(f"conv_bn: {type(conv).__name__} takes {want} inputs, got {len(inputs)}")
    with torch.no_grad():   # the layer's own checks, operands, route and launch (its _conv), with the epilogue
        return conv._conv(partial(_epilogue, bn, residual, out_dtype), *inputs, out_dtype)


# How a U-Net is walked (its _walk): the (conv, bn, *inputs, residual) layers and the residual blocks as
# the modules themselves, or folded
MODULES = (conv_then_bn, lambda block, *at: block(*at))
FOLDED = (conv_bn, lambda block, *at: block.infer(*at))


def argmax_labels(logits: torch.Tensor) -> torch.Tensor:
    """int64 [T] = argmax over the classes of fp32 logits [T, K] (pcs_argmax; a NaN row as torch.argmax)."""
    T, K = logits.shape
    out = torch.empty(T, dtype=torch.int64, device=logits.device)
    if T:
        L.call("pcs_argmax", logits, logits.stride(0), T, K, out, L.stream_ptr(logits.device))
    return out


__all__ = ["argmax_labels", "conv_bn"]
