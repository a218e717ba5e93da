"""The dense voxel U-Net (BASELINE configs[1]) assembled from the channels-last dense layers of
pcs_amd.voxel: BatchNorm / residual blocks on a [B, G, G, G, C] grid (VoxelBatchNorm, VoxelResBlock),
the encoder / decoder (VoxelUNet), the point <-> grid map of a dense grid (dense_point_map) and a
per-point segmentation model around them (VoxelUNetSegmentation).  Build-defined, like the rest of
the voxel vocabulary: the reference has no voxel grid.

    model = VoxelUNetSegmentation(in_channels=4, num_classes=2, widths=(32, 64, 128), grid=128).cuda()
    opt = FusedAdam(model)
    loss = model.loss(rb, class_weight)                  # rb: RaggedBatch
    logits = model(rb)                                   # fp32 [T, num_classes]
    labels = model.predict(rb)                           # inference: int64 [T], BatchNorm folded into the convolutions

The module tree and state_dict are SparseUNetSegmentation's for the same widths, and each loads the
other's: on a fully occupied grid a submanifold convolution is the zero-padded dense convolution, so
the two models are the same function there and two independent kernel families can be compared on
the same weights.  They differ where cells are empty: here an empty cell carries a zero row into the
first convolution and is a cell like any other after it, and the BatchNorm statistics run over all
B * G^3 cells, the usual dense meaning.  Every 3x3x3 convolution is the LDS-halo stencil; the
decoder's skip connection is the two-source stencil (voxel.Conv3dCat), so no level builds a
concatenated grid.  The row of cell (scene, ix, iy, iz) is (scene * G + ix) * G * G + iy * G + iz, so
[B * G^3, C] rows and the [B, G, G, G, C] grid are views of each other and the row kernels
(SparseBatchNorm, the point ends of pcs_amd.pointvoxel / pointhead / segmax) run on the grid
unchanged.  model.predict(rb) is the inference path (pcs_amd.fold): the running statistics, every
convolution -> BatchNorm (+ residual) + ReLU as one kernel, no gradient, then the argmax.
"""
from __future__ import annotations

import torch

from . import _lib as L
from .data import RaggedBatch
from .fold import FOLDED, MODULES, argmax_labels, conv_bn
from .pointhead import point_head, point_head_loss, point_lift_mean
from .pointvoxel import CORNERS, PointVoxelMap, devoxelize, voxel_mean
from .segmax import point_lift_max, voxel_max
from .sparse_norm import SparseBatchNorm, SparseResBlock, conv_then_bn
from .voxel import Conv3d, Conv3dCat, ConvTranspose3d, _box


def dense_point_map(rb: RaggedBatch, grid: int, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), device=None) -> PointVoxelMap:
    """The map of rb's points into a dense B x grid^3 level (pcs_dense_trilinear_index): every cell is
    present, at row (scene * grid + ix) * grid^2 + iy * grid + iz, so own is never -1, a corner is -1
    only outside the grid, and no hash table is built.  num_voxels = B * grid^3 (< 2^31).  voxel_mean,
    voxel_max, devoxelize, point_lift_mean, point_lift_max, point_head and point_head_loss run on it as
    on point_voxel_map's."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError("pcs_amd dense_point_map runs on a HIP device only (no CPU fallback)")
    pts = rb.points.to(dev, torch.float32).contiguous()
    off = rb.offsets.to(dev, torch.int64).contiguous()
    if pts.dim() != 2 or pts.shape[1] != 4:
        raise ValueError(f"dense_point_map: points must be [T, 4], got {list(pts.shape)}")
    T, B = pts.shape[0], off.numel() - 1
    own = torch.empty(T, dtype=torch.int32, device=dev)
    corner = torch.empty(T, CORNERS, dtype=torch.int32, device=dev)
    weight = torch.empty(T, CORNERS, dtype=torch.float32, device=dev)
    L.call("pcs_dense_trilinear_index", pts, off, B, T, int(grid), *_box(lo, hi), own, corner, weight, L.stream_ptr(dev))
    return PointVoxelMap(own, corner, weight, B * int(grid) ** 3)


class VoxelBatchNorm(SparseBatchNorm):
    """SparseBatchNorm on the [B * D * H * W, C] view of a channels-last grid [B, D, H, W, C]: the
    statistics run over every cell.  nn.BatchNorm1d's parameters, buffers and state dict."""

    def forward(self, x, residual=None, out_dtype=None):
        if x.dim() != 5:
            raise ValueError(f"VoxelBatchNorm: x must be a [B, D, H, W, C] channels-last grid, got {list(x.shape)}")
        c = x.shape[-1]
        r = None if residual is None else residual.contiguous().view(-1, c)
        return super().forward(x.contiguous().view(-1, c), r, out_dtype).view(x.shape)


class VoxelResBlock(torch.nn.Module):
    """Conv3d -> BN+ReLU -> Conv3d -> BN(+ x)+ReLU on a bf16 grid [B, D, H, W, channels], identity
    shortcut (SparseResBlock's tree).  The convolutions carry no bias: BatchNorm cancels it."""

    def __init__(self, channels):
        super().__init__()
        self.conv1, self.bn1 = Conv3d(channels, channels, bias=False), VoxelBatchNorm(channels, relu=True)
        self.conv2, self.bn2 = Conv3d(channels, channels, bias=False), VoxelBatchNorm(channels, relu=True)

    _walk = SparseResBlock._walk

    def forward(self, x):
        return self._walk(conv_then_bn, x)

    def infer(self, x):
        """forward in eval mode with each BatchNorm folded into its convolution's store (fold.conv_bn):
        the running statistics whatever self.training says, no gradient, nothing updated."""
        return self._walk(conv_bn, x)


class VoxelUNet(torch.nn.Module):
    """U-Net on a dense bf16 grid [B, G, G, G, widths[0]] in and out, SparseUNet's structure and
    attribute names.  Per level l above the bottom: enc[l] = VoxelResBlock(w_l); down[l] = Conv3d(w_l,
    w_{l+1}, k=2, s=2, p=0) + BN+ReLU; the bottom is one VoxelResBlock; on the way up up[l] =
    ConvTranspose3d(w_{l+1}, w_l, k=2, s=2) + BN+ReLU, merge[l] = Conv3dCat(w_l, w_l, w_l) on (up,
    skip), in that order, + BN+ReLU, and dec[l] = VoxelResBlock(w_l).  No convolution carries a bias."""

    def __init__(self, widths=(32, 64, 128)):
        super().__init__()
        widths = tuple(int(w) for w in widths)
        if len(widths) < 1 or any(w <= 0 for w in widths):
            raise ValueError("VoxelUNet: widths must be positive channel counts, finest level first")
        self.widths = widths
        pairs = list(zip(widths[:-1], widths[1:]))
        ML, BN = torch.nn.ModuleList, lambda w: VoxelBatchNorm(w, relu=True)   # noqa: E731
        self.enc = ML(VoxelResBlock(w) for w, _ in pairs)
        self.down = ML(Conv3d(w, wc, 2, 2, 0, bias=False) for w, wc in pairs)
        self.down_bn = ML(BN(wc) for _, wc in pairs)
        self.bottom = VoxelResBlock(widths[-1])
        self.up = ML(ConvTranspose3d(wc, w, 2, 2, bias=False) for w, wc in pairs)
        self.up_bn = ML(BN(w) for w, _ in pairs)
        self.merge = ML(Conv3dCat(w, w, w, bias=False) for w, _ in pairs)
        self.merge_bn = ML(BN(w) for w, _ in pairs)
        self.dec = ML(VoxelResBlock(w) for w, _ in pairs)

    @property
    def depth(self) -> int:
        return len(self.widths) - 1

    def _check_grid(self, x):
        if x.dim() != 5 or any(d % (1 << self.depth) for d in x.shape[1:4]):
            raise ValueError(f"VoxelUNet: a [B, D, H, W, C] grid with D, H, W divisible by 2**{self.depth} is required, "
                             f"got {list(x.shape)}")

    def _walk(self, how, x):
        """The network with its layers and blocks applied as how = fold.MODULES or fold.FOLDED says."""
        layer, block = how
        self._check_grid(x)
        skips = []
        for l in range(self.depth):
            e = block(self.enc[l], x)
            skips.append(e)
            x = layer(self.down[l], self.down_bn[l], e)
        x = block(self.bottom, x)
        for l in reversed(range(self.depth)):
            u = layer(self.up[l], self.up_bn[l], x)
            m = layer(self.merge[l], self.merge_bn[l], u, skips[l])
            x = block(self.dec[l], m)
        return x

    def forward(self, x):
        return self._walk(MODULES, x)

    def infer(self, x):
        """forward in eval mode, layer for layer, with every convolution -> BatchNorm pair as one kernel
        (fold.conv_bn): the running statistics whatever self.training says, no gradient, nothing updated."""
        return self._walk(FOLDED, x)


class VoxelUNetSegmentation(torch.nn.Module):
    """Per-point segmentation of a RaggedBatch through the dense U-Net: dense_point_map ->
    relu(Linear(in_channels, w_0)) on the points -> voxel_mean onto the B x grid^3 cells (an empty cell
    is a zero row) -> VoxelUNet -> trilinear devoxelize -> Linear(w_0, num_classes).  Returns fp32
    logits [T, num_classes] in the batch's point order.  Constructor, forward(rb, fused) and loss(rb,
    class_weight, return_logits) have SparseUNetSegmentation's meaning, and list(state_dict()) is that
    model's for the same widths.  grid must be divisible by 2**(len(widths) - 1)."""

    def __init__(self, in_channels=4, num_classes=2, widths=(32, 64, 128), grid=128, lo=(-1.0, -1.0, -1.0),
                 hi=(1.0, 1.0, 1.0), lift="mean"):
        super().__init__()
        if lift not in ("mean", "max"):
            raise ValueError(f"VoxelUNetSegmentation: lift must be 'mean' or 'max', got {lift!r}")
        self.lift_mode = lift
        self.unet = VoxelUNet(widths)
        if grid <= 0 or grid % (1 << self.unet.depth) != 0:
            raise ValueError(f"VoxelUNetSegmentation: grid {grid} is not divisible by 2**{self.unet.depth}")
        self.in_channels, self.num_classes, self.grid = int(in_channels), int(num_classes), int(grid)
        self.lo, self.hi = tuple(float(v) for v in lo), tuple(float(v) for v in hi)
        self.lift = torch.nn.Linear(self.in_channels, self.unet.widths[0])
        self.head = torch.nn.Linear(self.unet.widths[0], self.num_classes)

    def _map(self, rb: RaggedBatch):
        """(device, scenes, point map of the grid) of a batch."""
        dev = self.lift.weight.device
        if dev.type != "cuda":
            raise RuntimeError("pcs_amd VoxelUNetSegmentation runs on a HIP device only (no CPU fallback)")
        if rb.points.dim() != 2 or rb.points.shape[1] < self.in_channels:
            raise ValueError(f"VoxelUNetSegmentation: points must be [T, >= {self.in_channels}], got "
                             f"{list(rb.points.shape)}")
        return dev, rb.offsets.numel() - 1, dense_point_map(rb, self.grid, self.lo, self.hi, device=dev)

    def _unet_rows(self, x, B, unet=None):
        """The U-Net (unet: self.unet.infer in its place) on per-cell rows [B * grid^3, w_0] (a view of the grid
        either way)."""
        G, c = self.grid, x.shape[1]
        return (unet or self.unet)(x.view(B, G, G, G, c)).reshape(B * G * G * G, c)

    def _fused_features(self, rb, dev, B, pvm, unet=None):
        """The U-Net's output rows with the lift fused into the voxel mean (lift="max": the voxel max)."""
        fn = point_lift_max if self.lift_mode == "max" else point_lift_mean
        x = fn(rb.points.to(dev, torch.float32), self.lift.weight, self.lift.bias, pvm)
        return self._unet_rows(x, B, unet)

    def forward(self, rb: RaggedBatch, fused: bool = False):
        """fused=True: the same function through pointhead.point_lift_mean and point_head on the same
        lift / head parameters (no [T, w_0] array in either direction; another summation order)."""
        dev, B, pvm = self._map(rb)
        if fused:
            return point_head(self._fused_features(rb, dev, B, pvm), pvm, self.head.weight, self.head.bias)
        pts = rb.points.to(dev, torch.float32)[:, :self.in_channels]
        x = (voxel_max if self.lift_mode == "max" else voxel_mean)(torch.relu(self.lift(pts)), pvm)
        return self.head(devoxelize(self._unet_rows(x, B), pvm))

    def loss(self, rb: RaggedBatch, class_weight=None, return_logits: bool = False):
        """The weighted cross-entropy of the batch's own labels (-1 = ignored) on the fused path:
        F.cross_entropy(self(rb), rb.labels, weight=class_weight, ignore_index=-1) as a 0-dim fp32
        tensor, or (loss, logits.detach()) with return_logits (pointhead.point_head_loss)."""
        dev, B, pvm = self._map(rb)
        x = self._fused_features(rb, dev, B, pvm)
        return point_head_loss(x, pvm, self.head.weight, self.head.bias, rb.labels.to(dev), class_weight, return_logits)

    def predict(self, rb: RaggedBatch, return_logits: bool = False):
        """Inference: int64 labels [T] in the batch's point order, or (labels, fp32 logits [T,
        num_classes]) with return_logits.  The fused lift, VoxelUNet.infer (every BatchNorm folded into
        its convolution, on the running statistics), point_head and the argmax (pcs_argmax), under
        torch.no_grad().  self.training, the running buffers and num_batches_tracked are left as they
        are, so it may be called on a model in train() mode."""
        with torch.no_grad():
            dev, B, pvm = self._map(rb)
            x = self._fused_features(rb, dev, B, pvm, self.unet.infer)
            logits = point_head(x, pvm, self.head.weight, self.head.bias)
            labels = argmax_labels(logits)
        return (labels, logits) if return_logits else labels


__all__ = ["VoxelBatchNorm", "VoxelResBlock", "VoxelUNet", "VoxelUNetSegmentation", "dense_point_map"]
