"""Segmented max for the occupied-voxel path (csrc/segmax.hip, the fused lift in csrc/pointhead.hip):
the max over a segment of rows with torch.max's pick, with gradients, and the three things a voxel
network is built from it.

    v = voxel_max(point_feats, pvm)                          # [T, C] -> [V, C]: max of a voxel's points
    c = sparse_max_pool(x_fine, link)                        # [Vf, C] -> [Vc, C]: nn.MaxPool3d(2, 2)
    v = point_lift_max(rb.points.cuda(), lift.weight, lift.bias, pvm)   # voxel_max(relu(Linear(p)))

Build-defined like the rest of the voxel vocabulary (tests/segmax_refs.py states it in numpy).  The
pick is torch.max's over a dim: a NaN beats every number, and among equal values the first row of
the segment wins; the backward hands the whole gradient to the picked row (torch.max's and
max_pool3d's rule, not the even split over ties of scatter_reduce(amax)).  Kept for the backward: the
picked rows (int32 [M, C]), neither the input nor the output.  point_lift_max keeps nothing of size
[T, C]: its backward recomputes relu(W p + b) and re-finds the pick.  Forward and backward are bitwise
reproducible.  A NaN met in a backward is unspecified.
"""
from __future__ import annotations

import torch

from . import _lib as L
from .pointhead import MAX_CIN, _align, _pad_rows, _workspace
from .pointvoxel import PointVoxelMap, _cut, _rows_in
from .sparse import CoarseLink


class _SegmentMaxFn(torch.autograd.Function):
    """Y[m], arg[m] = pcs_rows_segmax over segment m;  dX = pcs_rows_argselect(dY, arg, seg_of)."""

    @staticmethod
    def forward(ctx, x, src, seg_off, seg_of, out_dtype, name):
        xk = _rows_in(x, name, x.shape[0])
        R, ck, M, dev = xk.shape[0], xk.shape[1], seg_off.numel() - 1, xk.device
        ctx.cfg = (x.shape[1], x.dtype, R, name)
        if M == 0 or R == 0:   # no segment, or every segment empty
            ctx.save_for_backward(None, seg_of)
            return torch.zeros(M, x.shape[1], dtype=out_dtype, device=dev)
        y = torch.empty(M, ck, dtype=out_dtype, device=dev)
        arg = torch.empty(M, ck, dtype=torch.int32, device=dev)
        L.call("pcs_rows_segmax", xk, L.dtype_code(xk.dtype), src, seg_off, M, ck, y, L.dtype_code(out_dtype), arg,
               L.stream_ptr(dev))
        ctx.save_for_backward(arg, seg_of)
        return _cut(y, x.shape[1])

    @staticmethod
    def backward(ctx, dy):
        c, dtype, R, name = ctx.cfg
        arg, seg_of = ctx.saved_tensors
        if arg is None:
            return torch.zeros(R, c, dtype=dtype, device=dy.device), None, None, None, None, None
        dk = _rows_in(dy, name + " backward", arg.shape[0])
        dx = torch.empty(R, dk.shape[1], dtype=dtype, device=dk.device)
        L.call("pcs_rows_argselect", dk, L.dtype_code(dk.dtype), arg, seg_of, R, dk.shape[1], dx, L.dtype_code(dtype),
               L.stream_ptr(dk.device))
        return _cut(dx, c), None, None, None, None, None


def _index(t, name, what, dtype, numel=None):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 1 or (numel is not None and t.numel() != numel):
        raise ValueError(f"{name}: {what} must be a 1-d {dtype} tensor" + (f" of {numel} entries" if numel is not None else ""))
    return t.contiguous()


def _segment_max(x, src, seg_off, seg_of, out_dtype, name):
    if not x.is_cuda:
        raise RuntimeError(f"pcs_amd {name} runs on a HIP device only (no CPU fallback)")
    if x.dim() != 2:
        raise ValueError(f"{name}: expected [R, C] features, got {list(x.shape)}")
    out_dtype = x.dtype if out_dtype is None else out_dtype
    L.dtype_code(out_dtype)
    seg_off = _index(seg_off, name, "seg_off", torch.int64)
    if seg_off.numel() < 1:
        raise ValueError(f"{name}: seg_off must hold M + 1 offsets")
    if src is not None:
        src = _index(src, name, "src", torch.int32)
    seg_of = _index(seg_of, name, "seg_of", torch.int32, x.shape[0])
    return _SegmentMaxFn.apply(x, src, seg_off, seg_of, out_dtype, name)


def segment_max(x: torch.Tensor, src, seg_off: torch.Tensor, seg_of: torch.Tensor, out_dtype=None) -> torch.Tensor:
    """The max over segments of rows: y[m] = max of x[src[j]] over j in [seg_off[m], seg_off[m + 1]), per
    channel, with torch.max's pick (a NaN wins; among equal values the smallest j).  x [R, C] bf16 or
    fp32; src int32 (-1 = skipped) or None (the rows themselves, src[j] = j); seg_off int64 [M + 1],
    ascending, on the device; seg_of int32 [R], the segment of each row of x or -1, which the backward
    reads: a row may belong to at most one segment, once.  Returns [M, C] in out_dtype (None: x's); a
    segment without a row is a zero row.  The gradient (x's dtype) of y[m][c] goes to the picked row."""
    return _segment_max(x, src, seg_off, seg_of, out_dtype, "segment_max")


def voxel_max(point_feats: torch.Tensor, pvm: PointVoxelMap, out_dtype=torch.bfloat16) -> torch.Tensor:
    """Per-voxel max of per-point features: [T, C] (bf16 or fp32) -> [V, C] in out_dtype, the max in
    point order with torch.max's pick (a NaN wins; among equal values the first point).  A point whose
    voxel the level does not hold is ignored (zero gradient); a voxel without points is a zero row.
    The gradient has point_feats' dtype and goes to the picked point alone."""
    if point_feats.dim() != 2 or point_feats.shape[0] != pvm.num_points:
        raise ValueError(f"voxel_max: expected [{pvm.num_points}, C] features for this map, got {list(point_feats.shape)}")
    order, seg_off = pvm.points_by_voxel()[:2]
    return _segment_max(point_feats, order, seg_off, pvm.own, out_dtype, "voxel_max")


def sparse_max_pool(x_fine: torch.Tensor, link: CoarseLink, out_dtype=None) -> torch.Tensor:
    """nn.MaxPool3d(2, 2) on occupied voxels only: [Vf, C] (bf16 or fp32) on the fine level of link ->
    [Vc, C] on its coarse level, the max over the occupied voxels of each 2x2x2 cell.  Among equal
    values the first tap in CoarseLink's tap order wins, which is max_pool3d's window scan order; the
    gradient goes to that voxel alone."""
    if x_fine.dim() != 2 or x_fine.shape[0] != link.fine:
        raise ValueError(f"sparse_max_pool: expected [{link.fine}, C] features for this link, got {list(x_fine.shape)}")
    src, seg_off = link.child_segments()
    return _segment_max(x_fine, src, seg_off, link.parent, out_dtype, "sparse_max_pool")


class SparseMaxPool3d(torch.nn.Module):
    """sparse_max_pool as a layer: forward(x_fine, link)."""

    def __init__(self, out_dtype=None):
        super().__init__()
        self.out_dtype = out_dtype

    def forward(self, x_fine, link: CoarseLink):
        return sparse_max_pool(x_fine, link, self.out_dtype)


class _PointLiftMaxFn(torch.autograd.Function):
    """Y[v] = relu(max over v's points of W p + b);  dW, db through the re-found pick."""

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
        order, seg_off = pvm.points_by_voxel()[:2]
        y = torch.empty(V, ck, dtype=out_dtype, device=dev)
        L.call("pcs_point_lift_max", points, points.shape[1], cin, wk, bk, order, seg_off, V, ck, y,
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
        dk = _rows_in(dv, "point_lift_max backward", V)
        order, seg_off = pvm.points_by_voxel()[:2]
        nbytes = L.workspace("pcs_point_lift_max_bwd_workspace", V, ck, cin)
        ws = _workspace(nbytes, dev)
        dw = torch.empty(ck, cin, device=dev)
        db = torch.empty(ck, device=dev) if want_b else None
        L.call("pcs_point_lift_max_bwd", dk, L.dtype_code(dk.dtype), points, points.shape[1], cin, wk, bk, order, seg_off,
               V, ck, ws, nbytes, dw, db, L.stream_ptr(dev))
        return dw[:C], (db[:C] if want_b else None), None, None, None


def point_lift_max(points: torch.Tensor, weight: torch.Tensor, bias, pvm: PointVoxelMap,
                   out_dtype=torch.bfloat16) -> torch.Tensor:
    """voxel_max(relu(F.linear(points[:, :Cin], weight, bias)), pvm, out_dtype) in one pass over the
    points (the VoxelNet / PointPillars feature encoder): [T, >= Cin] fp32 points, weight [C, Cin]
    (Cin <= 8), bias [C] or None -> [V, C] in out_dtype.  Gradients reach weight and bias only (the
    points must not require one), through the first point of the largest W p + b of each voxel."""
    if not points.is_cuda or not weight.is_cuda:
        raise RuntimeError("pcs_amd point_lift_max runs on a HIP device only (no CPU fallback)")
    if points.requires_grad:
        raise ValueError("point_lift_max: the points get no gradient (points.requires_grad must be False)")
    if weight.dim() != 2 or not 1 <= weight.shape[1] <= MAX_CIN:
        raise ValueError(f"point_lift_max: weight must be [C, Cin] with 1 <= Cin <= {MAX_CIN}, got {list(weight.shape)}")
    if points.dim() != 2 or points.shape[0] != pvm.num_points or points.shape[1] < weight.shape[1]:
        raise ValueError(f"point_lift_max: expected [{pvm.num_points}, >= {weight.shape[1]}] points for this map, got "
                         f"{list(points.shape)}")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"point_lift_max: bias must be [{weight.shape[0]}], got {list(bias.shape)}")
    L.dtype_code(out_dtype)
    return _PointLiftMaxFn.apply(weight, bias, points.detach().float().contiguous(), pvm, out_dtype)


__all__ = ["SparseMaxPool3d", "point_lift_max", "segment_max", "sparse_max_pool", "voxel_max"]
