"""Differentiable point <-> voxel transfer for the occupied-voxel path (csrc/pointvoxel.hip): the
two operators a point-voxel network (PVCNN / SPVCNN style) needs around the sparse U-Net of
pcs_amd.sparse, with gradients.

    vb = voxelize(rb, grid=256); sv = sparse_voxels(rb, vb); svc, link = coarsen(sv)
    pvm, pvc = point_voxel_map(rb, sv), point_voxel_map(rb, svc)   # one map per level
    v = voxel_mean(point_feats, pvm)              # [T, C] -> [V, C]: mean of the points of a voxel
    ...                                           # SubMConv3d / SparseDownConv3d / SparseUpConv3d
    y = devoxelize(v, pvm) + devoxelize(c, pvc)   # [V, C] -> [T, C]: trilinear, from any level

Build-defined like the rest of the voxel vocabulary (tests/point_voxel_refs.py states it in numpy).
A point's own voxel is voxelize()'s; its eight corners are the voxels whose centres surround it,
weighted trilinearly and renormalised over the occupied ones, which on a fully occupied grid is
F.grid_sample(mode="bilinear", padding_mode="border", align_corners=False).  Both operators are
linear and the weights carry no gradient to the coordinates, so each backward is the transpose of
its forward: a gather becomes a sum over the rows grouped by destination (pcs_rows_segsum over a
CSR built once per map), never an atomic add.  Forward and backward are bitwise reproducible.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import torch

from . import _lib as L
from .data import RaggedBatch
from .sparse import SparseVoxels
from .voxel import _box, _pad_channels

CORNERS = 8
PV_CH_ALIGN = 8   # channel multiple of the row kernels (one 16-byte bf16 piece); others run zero-padded


def _csr_by_row(rows: torch.Tensor, n_rows: int):
    """(order int32, seg_off int64 [n_rows + 1]) grouping the entries of rows (int32, -1 = none) by
    row, ascending entry order inside a row (torch's stable sort); the -1 entries sort behind the
    last segment.  No host read."""
    key = torch.where(rows < 0, n_rows, rows.to(torch.int64))
    skey, order = torch.sort(key, stable=True)
    # segment starts by binary search in the sorted keys (a bincount would add every missing
    # entry, most of a sparse level's corners, into the one sentinel bin)
    seg_off = torch.searchsorted(skey, torch.arange(n_rows + 1, dtype=torch.int64, device=rows.device))
    return order.to(torch.int32), seg_off.contiguous()


@dataclass
class PointVoxelMap:
    """Where T points sit in one level of V voxels."""
    own: torch.Tensor      # int32 [T]: row of the point's voxel, -1 when the level does not hold it
    corner: torch.Tensor   # int32 [T, 8]: rows of the trilinear corners, -1 = outside / unoccupied
    weight: torch.Tensor   # fp32 [T, 8]: normalised over the present corners, 0 where missing
    num_voxels: int
    _points: tuple = field(default=None, repr=False)
    _pairs: tuple = field(default=None, repr=False)

    @property
    def num_points(self) -> int:
        return self.own.numel()

    def points_by_voxel(self):
        """(order int32 [T], seg_off int64 [V + 1], counts int64 [V], inv_count fp32 [V], inv_of_point
        fp32 [T]): the points in voxel order (ascending inside a voxel), built once.  inv_count is 0
        for a voxel without points, inv_of_point 0 for a point without a voxel."""
        if self._points is None:
            order, seg_off = _csr_by_row(self.own, self.num_voxels)
            counts = seg_off[1:] - seg_off[:-1]
            inv = torch.where(counts > 0, 1.0 / counts.clamp_min(1).float(), 0.0).float()
            own64 = self.own.to(torch.int64)
            inv_pt = torch.where(own64 >= 0, inv[own64.clamp_min(0)] if self.num_voxels else 0.0, 0.0).float()
            self._points = (order, seg_off, counts, inv.contiguous(), inv_pt.contiguous())
        return self._points

    @property
    def counts(self) -> torch.Tensor:
        return self.points_by_voxel()[2]

    def pairs_by_voxel(self):
        """(point int32 [8 T], weight fp32 [8 T], seg_off int64 [V + 1]): the (point, corner) pairs
        grouped by the corner's voxel, ascending (point, corner) inside a voxel, built once."""
        if self._pairs is None:
            order, seg_off = _csr_by_row(self.corner.reshape(-1), self.num_voxels)
            o64 = order.to(torch.int64)
            point = torch.div(o64, CORNERS, rounding_mode="floor").to(torch.int32)
            self._pairs = (point, self.weight.reshape(-1)[o64].contiguous(), seg_off)
        return self._pairs


def point_voxel_map(rb: RaggedBatch, sv: SparseVoxels, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0)) -> PointVoxelMap:
    """The map of rb's points into the level sv (pcs_trilinear_index): sv itself, a coarser level
    of it (coarsen(sv)[0]), or any level queried at points it was not built from."""
    dev = sv.keys.device
    if dev.type != "cuda":
        raise RuntimeError("pcs_amd point_voxel_map runs on a HIP device only (no CPU fallback)")
    pts = rb.points.to(dev, torch.float32).contiguous()
    off = rb.offsets.to(dev, torch.int64).contiguous()
    T = pts.shape[0]
    own = torch.empty(T, dtype=torch.int32, device=dev)
    corner = torch.empty(T, CORNERS, dtype=torch.int32, device=dev)
    weight = torch.empty(T, CORNERS, dtype=torch.float32, device=dev)
    L.call("pcs_trilinear_index", pts, off, off.numel() - 1, T, int(sv.grid), *_box(lo, hi), sv.table_keys,
           sv.table_vals, sv.table_keys.numel(), own, corner, weight, L.stream_ptr(dev))
    return PointVoxelMap(own, corner, weight, sv.num_voxels)


def _rows_in(x, name, rows):
    if not x.is_cuda:
        raise RuntimeError(f"pcs_amd {name} runs on a HIP device only (no CPU fallback)")
    if x.dim() != 2 or x.shape[0] != rows:
        raise ValueError(f"{name}: expected [{rows}, C] features for this map, got {list(x.shape)}")
    L.dtype_code(x.dtype)
    ck = (x.shape[1] + PV_CH_ALIGN - 1) // PV_CH_ALIGN * PV_CH_ALIGN
    return _pad_channels(x, ck)


def _interp(x, idx, w, M, K, out_dtype):
    """pcs_rows_interp: [M, C] = sum_k w[:, k] * x[idx[:, k]]."""
    if x.shape[0] == 0:   # a level without voxels: nothing to gather
        return torch.zeros(M, x.shape[1], dtype=out_dtype, device=x.device)
    y = torch.empty(M, x.shape[1], dtype=out_dtype, device=x.device)
    L.call("pcs_rows_interp", x, L.dtype_code(x.dtype), idx, w, M, K, x.shape[1], y, L.dtype_code(out_dtype),
           L.stream_ptr(x.device))
    return y


def _segsum(x, src, w, seg_off, scale, M, out_dtype):
    """pcs_rows_segsum: [M, C] = scale * the sums of w * x[src] over the segments."""
    if x.shape[0] == 0:   # no source row: every segment is empty
        return torch.zeros(M, x.shape[1], dtype=out_dtype, device=x.device)
    y = torch.empty(M, x.shape[1], dtype=out_dtype, device=x.device)
    L.call("pcs_rows_segsum", x, L.dtype_code(x.dtype), src, w, seg_off, scale, M, x.shape[1], y,
           L.dtype_code(out_dtype), L.stream_ptr(x.device))
    return y


def _cut(y, c):
    return y if y.shape[1] == c else y[:, :c].contiguous()


class _VoxelMeanFn(torch.autograd.Function):
    """V[v] = mean of P[p] over own[p] == v (ascending p);  dP[p] = dV[own[p]] / count[own[p]]."""

    @staticmethod
    def forward(ctx, p, pvm, out_dtype):
        pk = _rows_in(p, "voxel_mean", pvm.num_points)
        order, seg_off, _, inv, _ = pvm.points_by_voxel()
        ctx.pvm, ctx.cfg = pvm, (p.shape[1], p.dtype)
        return _cut(_segsum(pk, order, None, seg_off, inv, pvm.num_voxels, out_dtype), p.shape[1])

    @staticmethod
    def backward(ctx, dv):
        pvm, (c, dtype) = ctx.pvm, ctx.cfg
        dk = _rows_in(dv, "voxel_mean backward", pvm.num_voxels)
        return _cut(_interp(dk, pvm.own, pvm.points_by_voxel()[4], pvm.num_points, 1, dtype), c), None, None


class _DevoxelizeFn(torch.autograd.Function):
    """trilinear: Y[p] = sum_k weight[p][k] X[corner[p][k]];  dX[v] = the sum over v's (point,
    corner) pairs of weight * dY[point].  nearest: Y[p] = X[own[p]];  dX[v] = the sum of dY over
    v's points."""

    @staticmethod
    def forward(ctx, x, pvm, trilinear, out_dtype):
        xk = _rows_in(x, "devoxelize", pvm.num_voxels)
        ctx.pvm, ctx.cfg = pvm, (x.shape[1], x.dtype, trilinear)
        if trilinear:
            y = _interp(xk, pvm.corner, pvm.weight, pvm.num_points, CORNERS, out_dtype)
        else:
            y = _interp(xk, pvm.own, None, pvm.num_points, 1, out_dtype)
        return _cut(y, x.shape[1])

    @staticmethod
    def backward(ctx, dy):
        pvm, (c, dtype, trilinear) = ctx.pvm, ctx.cfg
        dk = _rows_in(dy, "devoxelize backward", pvm.num_points)
        if trilinear:
            point, w, seg_off = pvm.pairs_by_voxel()
            dx = _segsum(dk, point, w, seg_off, None, pvm.num_voxels, dtype)
        else:
            order, seg_off = pvm.points_by_voxel()[:2]
            dx = _segsum(dk, order, None, seg_off, None, pvm.num_voxels, dtype)
        return _cut(dx, c), None, None, None


def voxel_mean(point_feats: torch.Tensor, pvm: PointVoxelMap, out_dtype=torch.bfloat16) -> torch.Tensor:
    """Per-voxel mean of per-point features: [T, C] (bf16 or fp32) -> [V, C] in out_dtype, fp32 sums
    in point order.  A point whose voxel the level does not hold is ignored (zero gradient); a voxel
    without points is a zero row.  The gradient has point_feats' dtype."""
    L.dtype_code(out_dtype)
    return _VoxelMeanFn.apply(point_feats, pvm, out_dtype)


def devoxelize(voxel_feats: torch.Tensor, pvm: PointVoxelMap, mode: str = "trilinear",
               out_dtype=torch.float32) -> torch.Tensor:
    """Per-point features from per-voxel features: [V, C] (bf16 or fp32) -> [T, C] in out_dtype.
    mode "trilinear": the normalised eight-corner interpolation; "nearest": the row of the point's
    own voxel.  A point with no occupied corner (own voxel) gets a zero row.  The gradient has
    voxel_feats' dtype."""
    if mode not in ("trilinear", "nearest"):
        raise ValueError(f"devoxelize: mode must be 'trilinear' or 'nearest', got {mode!r}")
    L.dtype_code(out_dtype)
    return _DevoxelizeFn.apply(voxel_feats, pvm, mode == "trilinear", out_dtype)


__all__ = ["PointVoxelMap", "devoxelize", "point_voxel_map", "voxel_mean"]
