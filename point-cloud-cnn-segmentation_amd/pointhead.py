"""The two per-point ends of the occupied-voxel U-Net as fused operators (csrc/pointhead.hip): the
lift relu(Linear(points)) -> voxel_mean and the head devoxelize -> Linear (-> weighted cross-entropy),
with gradients, without a [T, C] array in either direction.

    x = point_lift_mean(rb.points.cuda(), lift.weight, lift.bias, pvm)        # [V, C] bf16
    ...                                                                      # the sparse U-Net
    logits = point_head(x, pvm, head.weight, head.bias)                      # fp32 [T, K]
    loss = point_head_loss(x, pvm, head.weight, head.bias, labels, class_weight)

Lift: relu(W p + b) of a point of at most 8 floats costs less than loading its C-channel result, so
the forward computes it while it walks a voxel's points and stores only the [V, C] mean; the backward
recomputes the gate z > 0 from the points and writes only dW and db.  The points get no gradient.

Head: trilinear devoxelisation and the Linear are both linear, so logits[p] = b + sum_k w[p][k] *
(W x[corner[p][k]]): the V voxel rows are projected to the K classes first (Z = X W^T, fp32 [V, K])
and K numbers per corner are interpolated instead of C.  The backward sums dlogits over a voxel's
(point, corner) pairs into dZ[v] (K numbers), then dX[v] = dZ[v] W and dW = sum_v dZ[v]^T X[v].  Kept
for the backward: the voxel features and, for the loss, dlogits [T, K] fp32.

Every sum runs in a fixed order without atomics: forward and backward are bitwise reproducible.
More than 16 classes run the composition devoxelize + F.linear (+ F.cross_entropy).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib as L
from .pointvoxel import PV_CH_ALIGN, PointVoxelMap, _cut, _rows_in, devoxelize
from .voxel import _pad_channels

MAX_CIN = 8        # point columns of the lift kernel
MAX_CLASSES = 16   # classes of the head kernels; wider heads run the composition


def _align(c):
    return (c + PV_CH_ALIGN - 1) // PV_CH_ALIGN * PV_CH_ALIGN


def _pad_rows(t, rows):
    """[R, ...] fp32 -> [rows, ...] contiguous fp32 with zero rows appended."""
    t = t.detach().float()
    if t.shape[0] == rows:
        return t.contiguous()
    out = t.new_zeros(rows, *t.shape[1:])
    out[: t.shape[0]] = t
    return out


def _workspace(nbytes, device):
    return torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=device)


# ---- lift
class _PointLiftMeanFn(torch.autograd.Function):
    """Y[v] = mean over v's points of relu(W p + b);  dW, db with the gate recomputed."""

    @staticmethod
    def forward(ctx, weight, bias, points, pvm, out_dtype):
        C, cin = weight.shape
        ck, V, dev = _align(C), pvm.num_voxels, points.device
        wk = _pad_rows(weight, ck)
        bk = None if bias is None else _pad_rows(bias, ck)
        ctx.pvm, ctx.cfg = pvm, (C, cin, ck, bias is not None)
        ctx.save_for_backward(wk, bk, points)
        if V == 0 or points.shape[0] == 0:   # no voxel, or every segment empty
            return torch.zeros(V, C, dtype=out_dtype, device=dev)
        order, seg_off, _, inv, _ = pvm.points_by_voxel()
        y = torch.empty(V, ck, dtype=out_dtype, device=dev)
        L.call("pcs_point_lift_mean", points, points.shape[1], cin, wk, bk, order, seg_off, inv, V, ck, y,
               L.dtype_code(out_dtype), L.stream_ptr(dev))
        return _cut(y, C)

    @staticmethod
    def backward(ctx, dv):
        pvm, (C, cin, ck, has_bias) = ctx.pvm, ctx.cfg
        wk, bk, points = ctx.saved_tensors
        V, dev = pvm.num_voxels, points.device
        want_b = has_bias and ctx.needs_input_grad[1]
        if V == 0 or points.shape[0] == 0:
            dw = torch.zeros(C, cin, device=dev)
            return dw, (torch.zeros(C, device=dev) if want_b else None), None, None, None
        dk = _rows_in(dv, "point_lift_mean backward", V)
        order, seg_off, _, inv, _ = pvm.points_by_voxel()
        nbytes = L.workspace("pcs_point_lift_bwd_workspace", V, ck, cin)
        ws = _workspace(nbytes, dev)
        dw = torch.empty(ck, cin, device=dev)
        db = torch.empty(ck, device=dev) if want_b else None
        L.call("pcs_point_lift_mean_bwd", dk, L.dtype_code(dk.dtype), points, points.shape[1], cin, wk, bk, order,
               seg_off, inv, V, ck, ws, nbytes, dw, db, L.stream_ptr(dev))
        return dw[:C], (db[:C] if want_b else None), None, None, None


def point_lift_mean(points: torch.Tensor, weight: torch.Tensor, bias, pvm: PointVoxelMap,
                    out_dtype=torch.bfloat16) -> torch.Tensor:
    """voxel_mean(relu(F.linear(points[:, :Cin], weight, bias)), pvm, out_dtype) in one pass over the
    points: [T, >= Cin] fp32 points, weight [C, Cin] (Cin <= 8), bias [C] or None -> [V, C] in
    out_dtype.  Gradients reach weight and bias only (the points must not require one)."""
    if not points.is_cuda or not weight.is_cuda:
        raise RuntimeError("pcs_amd point_lift_mean runs on a HIP device only (no CPU fallback)")
    if points.requires_grad:
        raise ValueError("point_lift_mean: the points get no gradient (points.requires_grad must be False)")
    if weight.dim() != 2 or not 1 <= weight.shape[1] <= MAX_CIN:
        raise ValueError(f"point_lift_mean: weight must be [C, Cin] with 1 <= Cin <= {MAX_CIN}, got {list(weight.shape)}")
    if points.dim() != 2 or points.shape[0] != pvm.num_points or points.shape[1] < weight.shape[1]:
        raise ValueError(f"point_lift_mean: expected [{pvm.num_points}, >= {weight.shape[1]}] points for this map, got "
                         f"{list(points.shape)}")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"point_lift_mean: bias must be [{weight.shape[0]}], got {list(bias.shape)}")
    L.dtype_code(out_dtype)
    return _PointLiftMeanFn.apply(weight, bias, points.detach().float().contiguous(), pvm, out_dtype)


# ---- head
def _head_operands(x, pvm, weight, bias, name):
    if weight.dim() != 2 or x.dim() != 2 or weight.shape[1] != x.shape[1]:
        raise ValueError(f"{name}: weight must be [K, {x.shape[-1]}], got {list(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"{name}: bias must be [{weight.shape[0]}], got {list(bias.shape)}")
    xk = _rows_in(x.detach(), name, pvm.num_voxels)
    return xk, _pad_channels(weight.detach().float(), xk.shape[1]), None if bias is None else bias.detach().float().contiguous()


def _project(xk, wk):
    """Z = X W^T, fp32 [V, K] (one zero row for a level without voxels: no corner points at it)."""
    V, K = xk.shape[0], wk.shape[0]
    if V == 0:
        return torch.zeros(1, K, device=xk.device)
    z = torch.empty(V, K, device=xk.device)
    L.call("pcs_point_head_project", xk, L.dtype_code(xk.dtype), V, xk.shape[1], wk, K, z, L.stream_ptr(xk.device))
    return z


def _head_bwd(dl, pvm, xk, wk, gscale, want_dx, want_dw):
    """(dX [V, Ck] in xk's dtype, dW [K, Ck]) of pcs_point_head_bwd; None where not wanted."""
    V, ck, K, dev = xk.shape[0], xk.shape[1], wk.shape[0], xk.device
    if V == 0 or pvm.num_points == 0:
        return (torch.zeros_like(xk) if want_dx else None), (torch.zeros_like(wk) if want_dw else None)
    point, w, seg_off = pvm.pairs_by_voxel()
    nbytes = L.workspace("pcs_point_head_workspace", pvm.num_points, V, ck, K)
    ws = _workspace(nbytes, dev)
    dx = torch.empty_like(xk) if want_dx else None
    dw = torch.empty_like(wk) if want_dw else None
    L.call("pcs_point_head_bwd", dl, point, w, seg_off, xk, L.dtype_code(xk.dtype), V, ck, wk, K, gscale, dx, ws,
           nbytes, dw, L.stream_ptr(dev))
    return dx, dw


class _PointHeadFn(torch.autograd.Function):
    """logits = b + interpolate(X W^T);  any dlogits back through pcs_point_head_bwd."""

    @staticmethod
    def forward(ctx, x, weight, bias, pvm):
        xk, wk, bk = _head_operands(x, pvm, weight, bias, "point_head")
        T, K, dev = pvm.num_points, wk.shape[0], xk.device
        ctx.pvm, ctx.cfg = pvm, (x.shape[1], x.dtype)
        ctx.save_for_backward(xk, wk)
        logits = torch.empty(T, K, device=dev)
        if T > 0:
            z = _project(xk, wk)
            L.call("pcs_point_head_logits", z, pvm.corner, pvm.weight, T, K, bk, None, None, None, logits, None, None,
                   0, None, None, L.stream_ptr(dev))
        return logits

    @staticmethod
    def backward(ctx, dl):
        pvm, (c, dtype) = ctx.pvm, ctx.cfg
        xk, wk = ctx.saved_tensors
        dl = dl.float().contiguous()
        dx, dw = _head_bwd(dl, pvm, xk, wk, None, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (None if dx is None else _cut(dx, c).to(dtype), None if dw is None else _cut(dw, c),
                dl.sum(0) if ctx.needs_input_grad[2] else None, None)


class _PointHeadLossFn(torch.autograd.Function):
    """The weighted cross-entropy of the head's logits in the logits kernel: loss, dlogits and db in
    one pass over the points; the upstream gradient reaches the backward kernel as a device scalar."""

    @staticmethod
    def forward(ctx, x, weight, bias, pvm, labels, class_weight, return_logits):
        xk, wk, bk = _head_operands(x, pvm, weight, bias, "point_head_loss")
        T, V, K, dev = pvm.num_points, xk.shape[0], wk.shape[0], xk.device
        s = L.stream_ptr(dev)
        counts = torch.empty(K, dtype=torch.int64, device=dev)
        wsum = torch.empty(4, device=dev)   # [sum of class_weight[label], valid labels, 1 / sum, -]
        L.call("pcs_ce_weight_sum", labels, T, class_weight, K, counts, wsum, s)
        want = ctx.needs_input_grad[:3]
        want_b = bias is not None and want[2]
        dl = torch.empty(T, K, device=dev) if (want[0] or want[1]) else None
        db = torch.empty(K, device=dev) if want_b else None
        logits = torch.empty(T, K, device=dev) if return_logits else None
        loss = torch.empty(1, device=dev)
        nbytes = L.workspace("pcs_point_head_workspace", T, V, xk.shape[1], K)
        ws = _workspace(nbytes, dev)
        z = _project(xk, wk)
        L.call("pcs_point_head_logits", z, pvm.corner, pvm.weight, T, K, bk, labels, class_weight, wsum[2:], logits, dl,
               ws, nbytes, loss, db, s)
        ctx.pvm, ctx.cfg = pvm, (x.shape[1], x.dtype)
        ctx.save_for_backward(xk, wk, dl, db)
        if return_logits:
            ctx.mark_non_differentiable(logits)
            return loss[0], logits
        return loss[0]

    @staticmethod
    def backward(ctx, gloss, *_):
        pvm, (c, dtype) = ctx.pvm, ctx.cfg
        xk, wk, dl, db = ctx.saved_tensors
        g = gloss.detach().float().reshape(1).contiguous()
        dx = dw = None
        if dl is not None:
            dx, dw = _head_bwd(dl, pvm, xk, wk, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (None if dx is None else _cut(dx, c).to(dtype), None if dw is None else _cut(dw, c),
                None if db is None else db * g, None, None, None, None)


def _check_head(voxel_feats, weight, name):
    if not voxel_feats.is_cuda or not weight.is_cuda:
        raise RuntimeError(f"pcs_amd {name} runs on a HIP device only (no CPU fallback)")


def point_head(voxel_feats: torch.Tensor, pvm: PointVoxelMap, weight: torch.Tensor, bias=None) -> torch.Tensor:
    """F.linear(devoxelize(voxel_feats, pvm), weight, bias) as project-then-interpolate: [V, C] (bf16
    or fp32), weight [K, C], bias [K] or None -> fp32 logits [T, K].  A point without an occupied
    corner gets the bias alone.  Gradients: voxel_feats (its dtype), weight, bias."""
    _check_head(voxel_feats, weight, "point_head")
    if weight.dim() == 2 and weight.shape[0] > MAX_CLASSES:
        return F.linear(devoxelize(voxel_feats, pvm), weight, bias)
    return _PointHeadFn.apply(voxel_feats, weight, bias, pvm)


def point_head_loss(voxel_feats: torch.Tensor, pvm: PointVoxelMap, weight: torch.Tensor, bias, labels: torch.Tensor,
                    class_weight=None, return_logits: bool = False):
    """F.cross_entropy(point_head(voxel_feats, pvm, weight, bias), labels, weight=class_weight,
    ignore_index=-1) with the loss, its gradient and the bias gradient computed where the logits are:
    a 0-dim fp32 tensor, or (loss, logits.detach()) with return_logits.  labels: int64 [T], -1 (any
    value outside [0, K)) = ignored; class_weight: fp32 [K], None = ones.  The denominator (the sum of
    class_weight[label] over the valid labels) is computed on the device, without a host
    synchronisation.  Without a single valid label the loss is NaN, as torch's is (0 / 0): that is
    not a training input."""
    _check_head(voxel_feats, weight, "point_head_loss")
    dev = voxel_feats.device
    labels = labels.to(dev, torch.int64).contiguous()
    if labels.dim() != 1 or labels.shape[0] != pvm.num_points:
        raise ValueError(f"point_head_loss: labels must be [{pvm.num_points}], got {list(labels.shape)}")
    K = weight.shape[0]
    if class_weight is not None:
        class_weight = class_weight.detach().to(dev, torch.float32).contiguous()
        if tuple(class_weight.shape) != (K,):
            raise ValueError(f"point_head_loss: class_weight must be [{K}], got {list(class_weight.shape)}")
    if K > MAX_CLASSES or pvm.num_points == 0:
        logits = (F.linear(devoxelize(voxel_feats, pvm), weight, bias) if K > MAX_CLASSES
                  else point_head(voxel_feats, pvm, weight, bias))
        loss = F.cross_entropy(logits, labels, weight=class_weight, ignore_index=-1)
        return (loss, logits.detach()) if return_logits else loss
    if class_weight is None:
        class_weight = torch.ones(K, device=dev)
    return _PointHeadLossFn.apply(voxel_feats, weight, bias, pvm, labels, class_weight, bool(return_logits))


__all__ = ["point_head", "point_head_loss", "point_lift_mean"]
