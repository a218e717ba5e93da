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

Inference only: everything runs under torch.no_grad(), outputs never require grad, and an input that
requires grad while grad is enabled raises.  The bf16 weights are not rescaled (that would round them
again); the epilogue is exact fp32.
"""
from __future__ import annotations

import ctypes as ct

import torch

from . import _lib as L
from .sparse import (CH_ALIGN, K2_TAPS, TAPS, SparseDownConv3d, SparseUpConv3d, SubMConv3d, SubMConv3dCat)
from .sparse_norm import SparseBatchNorm
from .voxel import DENSE_CH_ALIGN, Conv3d, Conv3dCat, ConvTranspose3d, _bf16_2d, _conv_operands, _geom, _pad_channels

CONVS = (SubMConv3d, SubMConv3dCat, SparseDownConv3d, SparseUpConv3d, Conv3d, ConvTranspose3d, Conv3dCat)


def _bf16_input(x, name, dim, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("pcs_amd fold.conv_bn runs on a HIP device only (no CPU fallback)")
    if x.dtype != torch.bfloat16 or x.dim() != dim:
        raise ValueError(f"conv_bn: {name} must be {what}, got {x.dtype} {list(x.shape)}")
    return x


def _epilogue(bn, cout, cout_k, residual, out_shape, out_dtype, dev):
    """(scale, shift, residual) as a pcs_*_affine entry point takes them: the eval coefficients of bn
    (its running buffers) and the residual, with the zero channels _conv_operands pads an output with."""
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
    return coef[0], coef[1], residual


def _unpad(y, cout):
    return y if y.shape[-1] == cout else y[..., :cout].contiguous()


def _sparse_layer(nmap, pairs, rows_out, x, wk, bias, taps, bn, residual, out_dtype, up_pairs=None):
    """One sparse layer through nmap [rows_out, taps]: the pair lists (pairs), the tile gather (pairs
    None), or one pair per output row (up_pairs: the up-convolution).  x bf16 [rows_in, cin], wk the
    kernel-layout weight [cout, taps * cin]."""
    cout, dev, st = wk.shape[0], x.device, L.stream_ptr(x.device)
    xk, wb, bk, cin_k, cout_k = _conv_operands(x, wk, bias, taps, CH_ALIGN)
    scale, shift, res = _epilogue(bn, cout, cout_k, residual, (rows_out, cout), out_dtype, dev)
    y = torch.empty(rows_out, cout_k, dtype=out_dtype, device=dev)
    ydt, relu = L.dtype_code(out_dtype, what="out_dtype"), int(bn.relu)
    if up_pairs is not None:
        pin, pout, _, tap_off, P = up_pairs
        assert P == rows_out, "the up map has one pair per fine voxel"
        L.call("pcs_sparse_conv_rows_affine", pin, pout, ct.addressof(tap_off), taps, rows_out, xk, cin_k, wb, cout_k, bk,
               y, ydt, scale, shift, res, relu, st)
    elif pairs is None:
        L.call("pcs_sparse_conv_affine", nmap, rows_out, taps, xk, cin_k, wb, cout_k, bk, y, ydt, 0, scale, shift, res,
               relu, st)
    else:
        pin, _, ppos, tap_off, P = pairs
        z = torch.empty(max(P, 1), cout_k, dtype=torch.float32, device=dev)
        L.call("pcs_sparse_conv_pairs_affine", pin, ppos, ct.addressof(tap_off), taps, rows_out, xk, cin_k, wb, cout_k, bk,
               z, y, ydt, 0, scale, shift, res, relu, st)
    return _unpad(y, cout)


def _subm(conv, bn, x, sv, residual, out_dtype):
    V, cin = x.shape
    if sv.nbr.shape != (V, TAPS):
        raise ValueError("conv_bn: x must be bf16 [V, C] with a [V, 27] neighbour map")
    w = conv.weight
    if w.shape[1] != cin:
        raise ValueError(f"conv_bn: weight has {w.shape[1]} input channels, x has {cin}")
    wk = w.detach().permute(0, 2, 3, 4, 1).reshape(w.shape[0], TAPS * cin)
    return _sparse_layer(sv.nbr, sv.pairs() if sv.use_pairs() else None, V, x, wk, conv.bias, TAPS, bn, residual,
                         out_dtype)


def _subm_cat(conv, bn, xa, xb, sv, residual, out_dtype):
    V, ca, cb, cout = sv.nbr.shape[0], xa.shape[1], xb.shape[1], conv.weight.shape[0]
    if xa.shape[0] != V or xb.shape[0] != V or (ca, cb) != (conv.ca, conv.cb):
        raise ValueError(f"conv_bn: SubMConv3dCat({conv.ca}, {conv.cb}) takes bf16 [{V}, {conv.ca}] and [{V}, {conv.cb}]")
    if ca % CH_ALIGN or cb % CH_ALIGN or cout % CH_ALIGN:   # no two-source path: as submanifold_conv3d_cat
        return _subm(conv, bn, torch.cat([xa, xb], 1), sv, residual, out_dtype)
    dev, st = xa.device, L.stream_ptr(xa.device)
    xa, xb = xa.contiguous(), xb.contiguous()
    wb = _bf16_2d(conv.weight.detach().permute(0, 2, 3, 4, 1).reshape(cout, TAPS * (ca + cb)), cout, TAPS * (ca + cb))
    bk = None if conv.bias is None else conv.bias.detach().float().contiguous()
    scale, shift, res = _epilogue(bn, cout, cout, residual, (V, cout), out_dtype, dev)
    y = torch.empty(V, cout, dtype=out_dtype, device=dev)
    ydt, relu = L.dtype_code(out_dtype, what="out_dtype"), int(bn.relu)
    if V == 0:
        return y
    if sv.use_pairs():
        pin, _, ppos, tap_off, P = sv.pairs()
        z = torch.empty(max(P, 1), cout, dtype=torch.float32, device=dev)
        L.call("pcs_sparse_conv_cat_pairs_affine", pin, ppos, ct.addressof(tap_off), TAPS, V, xa, ca, xb, cb, wb, cout, bk,
               z, y, ydt, 0, scale, shift, res, relu, st)
    else:
        L.call("pcs_sparse_conv_cat_affine", sv.nbr, V, TAPS, xa, ca, xb, cb, wb, cout, bk, y, ydt, 0, scale, shift, res,
               relu, st)
    return y


def _stride(conv, bn, x, link, residual, out_dtype, up):
    rows_in, rows_out = (link.coarse, link.fine) if up else (link.fine, link.coarse)
    if x.shape[0] != rows_in:
        raise ValueError(f"conv_bn: x must be bf16 [{rows_in}, C]: the {'coarse' if up else 'fine'} voxels of the link")
    w, cin = conv.weight.detach(), x.shape[1]
    if w.shape[1 - int(up)] != cin:
        raise ValueError(f"conv_bn: weight has {w.shape[1 - int(up)]} input channels, x has {cin}")
    cout = w.shape[int(up)]
    wk = (w.permute(1, 2, 3, 4, 0) if up else w.permute(0, 2, 3, 4, 1)).reshape(cout, K2_TAPS * cin)
    if up:
        return _sparse_layer(link.up, None, rows_out, x, wk, conv.bias, K2_TAPS, bn, residual, out_dtype, link.up_pairs())
    return _sparse_layer(link.child, link.down_pairs() if link.use_pairs() else None, rows_out, x, wk, conv.bias, K2_TAPS,
                         bn, residual, out_dtype)


def _dense(conv, bn, x, residual, out_dtype, transposed, stride=None, padding=None):
    """pcs_conv3d_affine with conv's weight and bias: a Conv3d or ConvTranspose3d with its own stride and
    padding, or (stride, padding given) a Conv3dCat's weight on the concatenated grid."""
    B, D, H, W, cin = x.shape
    w = conv.weight.detach()
    k = w.shape[2]
    stride, padding = (conv.stride, conv.padding) if stride is None else (stride, padding)
    if w.shape[1 - int(transposed)] != cin:   # Conv3d [Cout, Cin, k, k, k], ConvTranspose3d [Cin, Cout, k, k, k]
        raise ValueError(f"conv_bn: weight has {w.shape[1 - int(transposed)]} input channels, x has {cin}")
    cout = w.shape[int(transposed)]
    wk = (w.permute(1, 2, 3, 4, 0) if transposed else w.permute(0, 2, 3, 4, 1)).reshape(cout, k ** 3 * cin)
    op = 0
    if transposed:
        op = conv.output_padding
        op = (int(op),) * 3 if isinstance(op, int) else tuple(int(o) for o in op)
    xk, wb, bk, cin_k, cout_k = _conv_operands(x, wk, conv.bias, k ** 3, DENSE_CH_ALIGN)
    g = _geom(B, (D, H, W), cin_k, cout_k, k, int(stride), int(padding), transposed, op)
    scale, shift, res = _epilogue(bn, cout, cout_k, residual, (B, g.Do, g.Ho, g.Wo, cout), out_dtype, x.device)
    y = torch.empty(B, g.Do, g.Ho, g.Wo, cout_k, dtype=out_dtype, device=x.device)
    L.call("pcs_conv3d_affine", g, xk, wb, bk, y, L.dtype_code(out_dtype, what="out_dtype"), scale, shift, res, int(bn.relu),
           L.stream_ptr(x.device))
    return _unpad(y, cout)


def _dense_cat(conv, bn, xa, xb, residual, out_dtype):
    if xa.shape[:4] != xb.shape[:4] or (xa.shape[-1], xb.shape[-1]) != (conv.ca, conv.cb):
        raise ValueError(f"conv_bn: Conv3dCat({conv.ca}, {conv.cb}) takes two bf16 grids [B, D, H, W, {conv.ca}] and "
                         f"[B, D, H, W, {conv.cb}]")
    (B, D, H, W, ca), cb, cout = xa.shape, xb.shape[-1], conv.weight.shape[0]
    if ca % DENSE_CH_ALIGN or cb % DENSE_CH_ALIGN or cout % DENSE_CH_ALIGN:   # no two-source path: as conv3d_cat
        return _dense(conv, bn, torch.cat([xa, xb], -1), residual, out_dtype, False, 1, 1)
    dev = xa.device
    xa, xb = xa.contiguous(), xb.contiguous()
    wb = _bf16_2d(conv.weight.detach().permute(0, 2, 3, 4, 1).reshape(cout, 27 * (ca + cb)), cout, 27 * (ca + cb))
    bk = None if conv.bias is None else conv.bias.detach().float().contiguous()
    g = _geom(B, (D, H, W), ca + cb, cout, 3, 1, 1, False)
    scale, shift, res = _epilogue(bn, cout, cout, residual, (B, D, H, W, cout), out_dtype, dev)
    y = torch.empty(B, D, H, W, cout, dtype=out_dtype, device=dev)
    L.call("pcs_conv3d_cat_affine", g, xa, ca, xb, cb, wb, bk, y, L.dtype_code(out_dtype, what="out_dtype"), scale, shift,
           res, int(bn.relu), L.stream_ptr(dev))
    return y


def conv_bn(conv, bn, *inputs, residual=None, out_dtype=torch.bfloat16):
    """bn in eval mode applied to conv(*inputs) (+ residual, then ReLU when bn.relu) as one kernel:
    bit-identical to bn.eval()(conv(*inputs, out_dtype=torch.float32), residual=residual,
    out_dtype=out_dtype) without the fp32 array.  conv: a SubMConv3d, SubMConv3dCat, SparseDownConv3d,
    SparseUpConv3d (pcs_amd.sparse) or Conv3d, ConvTranspose3d, Conv3dCat (pcs_amd.voxel); inputs: what
    its forward takes (without out_dtype); bn: a SparseBatchNorm / VoxelBatchNorm of the convolution's
    output channels, whose running buffers give scale / shift whatever bn.training says; residual: None
    or a tensor of the output's shape in out_dtype (bf16 or fp32).  The pair-list / tile-gather route is
    the unfused layer's for the same map.  Inference only: the output never requires grad, and an input
    that requires grad while grad is enabled raises."""
    if not isinstance(bn, SparseBatchNorm):
        raise TypeError(f"conv_bn: bn must be a SparseBatchNorm or VoxelBatchNorm, got {type(bn).__name__}")
    if not isinstance(conv, CONVS):
        raise TypeError(f"conv_bn: conv must be one of {', '.join(c.__name__ for c in CONVS)}, got {type(conv).__name__}")
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (*inputs, residual)):
        raise RuntimeError("conv_bn is inference only and has no backward: an input requires grad (detach it, or call "
                           "under torch.no_grad())")
    L.dtype_code(out_dtype, what="out_dtype")
    sparse = isinstance(conv, (SubMConv3d, SubMConv3dCat, SparseDownConv3d, SparseUpConv3d))
    two = isinstance(conv, (SubMConv3dCat, Conv3dCat))
    if len(inputs) != 1 + int(two) + int(sparse):
        raise TypeError(f"conv_bn: {type(conv).__name__} takes {1 + int(two) + int(sparse)} inputs, got {len(inputs)}")
    what = "bf16 [V, C] per-voxel features" if sparse else "a bf16 [B, D, H, W, C] channels-last voxel grid"
    xs = [_bf16_input(x, "x" if not two else ("xa", "xb")[i], 2 if sparse else 5, what)
          for i, x in enumerate(inputs[:1 + int(two)])]
    with torch.no_grad():
        if isinstance(conv, SubMConv3d):
            return _subm(conv, bn, xs[0], inputs[1], residual, out_dtype)
        if isinstance(conv, SubMConv3dCat):
            return _subm_cat(conv, bn, xs[0], xs[1], inputs[2], residual, out_dtype)
        if isinstance(conv, (SparseDownConv3d, SparseUpConv3d)):
            return _stride(conv, bn, xs[0], inputs[1], residual, out_dtype, isinstance(conv, SparseUpConv3d))
        if isinstance(conv, Conv3dCat):
            return _dense_cat(conv, bn, xs[0], xs[1], residual, out_dtype)
        return _dense(conv, bn, xs[0], residual, out_dtype, isinstance(conv, ConvTranspose3d))


def argmax_labels(logits: torch.Tensor) -> torch.Tensor:
    """int64 [T] = argmax over the classes of fp32 logits [T, K] (pcs_argmax; a NaN row as torch.argmax)."""
    T, K = logits.shape
    out = torch.empty(T, dtype=torch.int64, device=logits.device)
    if T:
        L.call("pcs_argmax", logits, logits.stride(0), T, K, out, L.stream_ptr(logits.device))
    return out


__all__ = ["argmax_labels", "conv_bn"]
