"""The occupied-voxel U-Net (BASELINE configs[2]) assembled from the sparse layers: the levels of
one voxelisation held together (SparsePyramid), the encoder / decoder on them (SparseUNet) and a
per-point segmentation model around it (SparseUNetSegmentation).  Build-defined, like the rest of
the voxel vocabulary: the reference has no voxel grid.

    model = SparseUNetSegmentation(in_channels=4, num_classes=2, grid=64).cuda()
    opt = FusedAdam(model)
    logits = model(rb)                                   # rb: RaggedBatch -> fp32 [T, num_classes]
    loss = F.cross_entropy(logits, rb.labels.cuda(), weight=class_weight, ignore_index=-1)
    labels = model.predict(rb)                           # inference: int64 [T], BatchNorm folded into the convolutions

Every convolution is a HIP kernel on occupied voxels only; the decoder's skip connection is the
two-source layer (sparse.SubMConv3dCat), so no level builds a concatenated tensor.  model(rb) leaves
the loss to the caller; model(rb, fused=True) and model.loss(rb, class_weight) run the two per-point
ends through pcs_amd.pointhead (the lift recomputed inside the voxel mean, the head projected before
it is interpolated, the cross-entropy where the logits are).  model.predict(rb) is the inference path
(pcs_amd.fold): the running statistics, every convolution -> BatchNorm (+ residual) + ReLU as one kernel,
no gradient, then the argmax.  BatchNorm statistics are per device.  The model is a plain nn.Module: FusedAdam
(optim.flatten_parameters is generic) works on it; checkpoint.save_checkpoint / load_checkpoint
rebuild a PointNetSegmentation and do not apply, use state_dict() / load_state_dict().
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .data import RaggedBatch
from .fold import FOLDED, MODULES, argmax_labels
from .pointhead import point_head, point_head_loss, point_lift_mean
from .pointvoxel import devoxelize, point_voxel_map, voxel_mean
from .segmax import point_lift_max, voxel_max
from .sparse import (CoarseLink, SparseDownConv3d, SparseUpConv3d, SparseVoxels, SubMConv3dCat, coarsen,
                     sparse_voxels)
from .sparse_norm import SparseBatchNorm, SparseResBlock
from .voxel import voxelize


@dataclass
class SparsePyramid:
    """The levels of one voxelisation, finest first: levels[l + 1], links[l] = coarsen(levels[l]),
    so links[l].fine == levels[l].num_voxels and links[l].coarse == levels[l + 1].num_voxels."""
    levels: list[SparseVoxels]
    links: list[CoarseLink]

    @property
    def depth(self) -> int:
        return len(self.links)


def sparse_pyramid(sv: SparseVoxels, depth: int) -> SparsePyramid:
    """sv and its depth coarser levels (grid / 2, / 4, ...); sv.grid must be divisible by 2**depth."""
    if depth < 0 or sv.grid % (1 << depth) != 0:
        raise ValueError(f"sparse_pyramid: a grid of {sv.grid} has no {depth} levels of halving (grid % 2**depth != 0)")
    levels, links = [sv], []
    for _ in range(depth):
        svc, link = coarsen(levels[-1])
        levels.append(svc)
        links.append(link)
    return SparsePyramid(levels, links)


class SparseUNet(torch.nn.Module):
    """U-Net on the levels of a SparsePyramid, bf16 per-voxel features [V0, widths[0]] in and out.
    Per level l above the bottom: enc[l] = SparseResBlock(w_l); down[l] = SparseDownConv3d(w_l,
    w_{l+1}) + BN+ReLU; the bottom is one SparseResBlock; on the way up up[l] = SparseUpConv3d(w_{l+1},
    w_l) + BN+ReLU, merge[l] = SubMConv3dCat(w_l, w_l, w_l) on (up, skip), in that order, + BN+ReLU,
    and dec[l] = SparseResBlock(w_l).  The convolutions carry no bias (BatchNorm cancels it)."""

    def __init__(self, widths=(64, 128, 256)):
        super().__init__()
        widths = tuple(int(w) for w in widths)
        if len(widths) < 1 or any(w <= 0 for w in widths):
            raise ValueError("SparseUNet: widths must be positive channel counts, finest level first")
        self.widths = widths
        pairs = list(zip(widths[:-1], widths[1:]))
        ML, BN = torch.nn.ModuleList, lambda w: SparseBatchNorm(w, relu=True)   # noqa: E731
        self.enc = ML(SparseResBlock(w) for w, _ in pairs)
        self.down = ML(SparseDownConv3d(w, wc, bias=False) for w, wc in pairs)
        self.down_bn = ML(BN(wc) for _, wc in pairs)
        self.bottom = SparseResBlock(widths[-1])
        self.up = ML(SparseUpConv3d(wc, w, bias=False) for w, wc in pairs)
        self.up_bn = ML(BN(w) for w, _ in pairs)
        self.merge = ML(SubMConv3dCat(w, w, w, bias=False) for w, _ in pairs)
        self.merge_bn = ML(BN(w) for w, _ in pairs)
        self.dec = ML(SparseResBlock(w) for w, _ in pairs)

    @property
    def depth(self) -> int:
        return len(self.widths) - 1

    def _walk(self, how, x, pyr):
        """The network with its layers and blocks applied as how = fold.MODULES or fold.FOLDED says."""
        layer, block = how
        if pyr.depth != self.depth:
            raise ValueError(f"SparseUNet: {len(self.widths)} widths need a pyramid of depth {self.depth}, got {pyr.depth}")
        skips = []
        for l in range(self.depth):
            e = block(self.enc[l], x, pyr.levels[l])
            skips.append(e)
            x = layer(self.down[l], self.down_bn[l], e, pyr.links[l])
        x = block(self.bottom, x, pyr.levels[-1])
        for l in reversed(range(self.depth)):
            u = layer(self.up[l], self.up_bn[l], x, pyr.links[l])
            m = layer(self.merge[l], self.merge_bn[l], u, skips[l], pyr.levels[l])
            x = block(self.dec[l], m, pyr.levels[l])
        return x

    def forward(self, x, pyr: SparsePyramid):
        return self._walk(MODULES, x, pyr)

    def infer(self, x, pyr: SparsePyramid):
        """forward in eval mode, layer for layer, with every convolution -> BatchNorm pair as one kernel
        (fold.conv_bn): the running statistics whatever self.training says, no gradient, nothing updated."""
        return self._walk(FOLDED, x, pyr)


class SparseUNetSegmentation(torch.nn.Module):
    """Per-point segmentation of a RaggedBatch through the occupied-voxel U-Net: voxelize ->
    sparse_voxels -> sparse_pyramid -> point_voxel_map -> relu(Linear(in_channels, w_0)) on the points
    -> voxel_mean -> SparseUNet -> trilinear devoxelize -> Linear(w_0, num_classes).  Returns fp32
    logits [T, num_classes] in the batch's point order (the first in_channels columns of the points
    feed the lift).  grid must be divisible by 2**(len(widths) - 1).  lift="max" takes voxel_max in
    voxel_mean's place (the PointNet-style voxel feature encoder; segmax.point_lift_max on the fused
    path) with the same parameters and state_dict."""

    def __init__(self, in_channels=4, num_classes=2, widths=(64, 128, 256), grid=64, lo=(-1.0, -1.0, -1.0),
                 hi=(1.0, 1.0, 1.0), lift="mean"):
        super().__init__()
        if lift not in ("mean", "max"):
            raise ValueError(f"SparseUNetSegmentation: lift must be 'mean' or 'max', got {lift!r}")
        self.lift_mode = lift
        self.unet = SparseUNet(widths)
        if grid <= 0 or grid % (1 << self.unet.depth) != 0:
            raise ValueError(f"SparseUNetSegmentation: grid {grid} is not divisible by 2**{self.unet.depth}")
        self.in_channels, self.num_classes, self.grid = int(in_channels), int(num_classes), int(grid)
        self.lo, self.hi = tuple(float(v) for v in lo), tuple(float(v) for v in hi)
        self.lift = torch.nn.Linear(self.in_channels, self.unet.widths[0])
        self.head = torch.nn.Linear(self.unet.widths[0], self.num_classes)

    def _levels(self, rb: RaggedBatch):
        """(device, pyramid, point map of the finest level) of a batch."""
        dev = self.lift.weight.device
        if dev.type != "cuda":
            raise RuntimeError("pcs_amd SparseUNetSegmentation runs on a HIP device only (no CPU fallback)")
        if rb.points.dim() != 2 or rb.points.shape[1] < self.in_channels:
            raise ValueError(f"SparseUNetSegmentation: points must be [T, >= {self.in_channels}], got "
                             f"{list(rb.points.shape)}")
        vb = voxelize(rb, self.grid, self.lo, self.hi, max(self.num_classes, 1), device=dev)
        sv = sparse_voxels(rb, vb, self.lo, self.hi)
        pyr = sparse_pyramid(sv, self.unet.depth)
        return dev, pyr, point_voxel_map(rb, sv, self.lo, self.hi)

    def _fused_features(self, rb, dev, pyr, pvm, unet=None):
        """The U-Net's output (unet: self.unet.infer in its place) on the finest level with the lift fused into the
        voxel mean (lift="max": the voxel max)."""
        fn = point_lift_max if self.lift_mode == "max" else point_lift_mean
        x = fn(rb.points.to(dev, torch.float32), self.lift.weight, self.lift.bias, pvm)
        return (unet or self.unet)(x, pyr)

    def forward(self, rb: RaggedBatch, fused: bool = False):
        """fused=True: the same function through pointhead.point_lift_mean and point_head on the same
        lift / head parameters (no [T, w_0] array in either direction; another summation order)."""
        dev, pyr, pvm = self._levels(rb)
        if fused:
            return point_head(self._fused_features(rb, dev, pyr, pvm), pvm, self.head.weight, self.head.bias)
        pts = rb.points.to(dev, torch.float32)[:, :self.in_channels]
        x = (voxel_max if self.lift_mode == "max" else voxel_mean)(torch.relu(self.lift(pts)), pvm)
        x = self.unet(x, pyr)
        return self.head(devoxelize(x, pvm))

    def loss(self, rb: RaggedBatch, class_weight=None, return_logits: bool = False):
        """The weighted cross-entropy of the batch's own labels (-1 = ignored) on the fused path:
        F.cross_entropy(self(rb), rb.labels, weight=class_weight, ignore_index=-1) as a 0-dim fp32
        tensor, or (loss, logits.detach()) with return_logits (pointhead.point_head_loss)."""
        dev, pyr, pvm = self._levels(rb)
        x = self._fused_features(rb, dev, pyr, pvm)
        return point_head_loss(x, pvm, self.head.weight, self.head.bias, rb.labels.to(dev), class_weight, return_logits)

    def predict(self, rb: RaggedBatch, return_logits: bool = False):
        """Inference: int64 labels [T] in the batch's point order, or (labels, fp32 logits [T,
        num_classes]) with return_logits.  The fused lift, SparseUNet.infer (every BatchNorm folded into
        its convolution, on the running statistics), point_head and the argmax (pcs_argmax), under
        torch.no_grad().  self.training, the running buffers and num_batches_tracked are left as they
        are, so it may be called on a model in train() mode."""
        with torch.no_grad():
            dev, pyr, pvm = self._levels(rb)
            x = self._fused_features(rb, dev, pyr, pvm, self.unet.infer)
            logits = point_head(x, pvm, self.head.weight, self.head.bias)
            labels = argmax_labels(logits)
        return (labels, logits) if return_logits else labels


__all__ = ["SparsePyramid", "SparseUNet", "SparseUNetSegmentation", "sparse_pyramid"]
