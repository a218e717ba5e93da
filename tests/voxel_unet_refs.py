"""Statements of the dense voxel U-Net (pcs_amd.voxel_unet): the numpy dense trilinear index
(pcs_dense_trilinear_index, dense_point_map) and an fp64 torch-CPU restatement of the whole model from
a state_dict.

TEST INFRASTRUCTURE ONLY.  Build-defined, like the rest of the voxel vocabulary: the reference has no
voxel grid, so this file defines the semantics.

The dense index, for a point p of scene s, box lo / hi and a B x G^3 grid in which every cell is present
at row (s * G + ix) * G^2 + iy * G + iz (tests/point_voxel_refs.py states the occupied-voxel form):
  u_d     = float32((p_d - lo_d) / (hi_d - lo_d)) * float32(G)
  own     = the row of cell i_d = clip(floor(u_d), 0, G - 1): never -1
  corners c_d = float32(min(max(u_d, 0), G)) - 0.5 (two roundings, no fused multiply-add), b_d =
          floor(c_d), f_d = c_d - b_d; corner k = (ax * 2 + ay) * 2 + az is cell b + a of the same scene,
          -1 only when it is outside [0, G - 1]; raw weight prod_d (a_d ? f_d : 1 - f_d); weight = raw /
          the sum of raw over the present corners, 0 for a missing corner
The integer outputs and f are float32-exact statements (what the device must reproduce bit for bit); the
weights are evaluated in float64 from them.

The model (VoxelUNetSegmentation, and SparseUNetSegmentation on a fully occupied grid, where a
submanifold convolution is the zero-padded dense convolution), everything in float64:
  x    = per-cell mean (lift "mean") or max (lift "max") of relu(P[:, :Cin] W_lift^T + b_lift), a zero
         row for a cell without points, as a grid [B, C, G, G, G] (D, H, W = x, y, z)
  res  = relu(bn2(conv2(relu(bn1(conv1(x))))) + x), conv = F.conv3d(., w, padding=1), bn = F.batch_norm
         over all B * G^3 cells (training: batch statistics; eval: the running buffers)
  unet = enc / down (F.conv3d stride 2, k = 2) + bn + relu / bottom / up (F.conv_transpose3d stride 2) +
         bn + relu / merge (F.conv3d on cat([up, skip], 1)) + bn + relu / dec, as SparseUNet's docstring
  out  = (sum_k weight[:, k] * unet[corner[:, k]]) W_head^T + b_head; the loss is F.cross_entropy with
         class weights and ignore_index = -1
"""
import numpy as np
import torch
import torch.nn.functional as F

import point_voxel_refs as pv


def dense_trilinear_index(points, offsets, grid, lo, hi):
    """(own int32 [T], corner int32 [T, 8], weight float64 [T, 8]) of a dense len(offsets) - 1 x grid^3 level."""
    G = int(grid)
    u = pv._u(points, G, lo, hi)
    assert u.dtype == np.float32
    T = len(u)
    base = pv._scene(offsets, T).astype(np.int64) * G ** 3
    i = np.clip(np.floor(u).astype(np.int64), 0, G - 1)
    own = (base + (i[:, 0] * G + i[:, 1]) * G + i[:, 2]).astype(np.int32)
    c = np.minimum(np.maximum(u, np.float32(0)), np.float32(G)) - np.float32(0.5)
    assert c.dtype == np.float32
    b = np.floor(c)
    f = (c - b).astype(np.float64)
    b = b.astype(np.int64)
    corner = np.full((T, 8), -1, np.int32)
    raw = np.zeros((T, 8), np.float64)
    for k in range(8):
        a = np.array([(k >> 2) & 1, (k >> 1) & 1, k & 1])
        j = b + a
        inside = ((j >= 0) & (j < G)).all(axis=1)
        jc = np.clip(j, 0, G - 1)
        corner[:, k] = np.where(inside, base + (jc[:, 0] * G + jc[:, 1]) * G + jc[:, 2], -1)
        raw[:, k] = np.prod(np.where(a == 1, f, 1.0 - f), axis=1)
    raw[corner < 0] = 0.0
    s = raw.sum(axis=1, keepdims=True)
    weight = np.divide(raw, s, out=np.zeros_like(raw), where=s > 0)
    return own, corner, weight


def dense_trilinear_weight32(points, offsets, grid, lo, hi):
    """The weights as the device evaluates them, float32 [T, 8], operation by operation: raw_k = ((x
    factor * y factor) * z factor) with the factor f_d or 1 - f_d, 0 for a missing corner; their sum in
    corner order from 0; inv = 1 / sum (0 when the sum is 0); weight_k = raw_k * inv.  Every operation is
    one correctly rounded float32 operation and none can fuse with another, so the device's weights
    equal these bit for bit."""
    G = int(grid)
    u = pv._u(points, G, lo, hi)
    c = np.minimum(np.maximum(u, np.float32(0)), np.float32(G)) - np.float32(0.5)
    b = np.floor(c)
    f = c - b
    assert f.dtype == np.float32
    j0 = b.astype(np.int64)
    one = np.float32(1)
    raw = np.zeros((len(u), 8), np.float32)
    s = np.zeros(len(u), np.float32)
    for k in range(8):
        a = np.array([(k >> 2) & 1, (k >> 1) & 1, k & 1])
        inside = ((j0 + a >= 0) & (j0 + a < G)).all(axis=1)
        fac = np.where(a == 1, f, one - f)
        raw[:, k] = np.where(inside, (fac[:, 0] * fac[:, 1]) * fac[:, 2], np.float32(0))
        s = s + raw[:, k]
    inv = np.where(s > 0, one / np.where(s > 0, s, one), np.float32(0)).astype(np.float32)
    w = raw * inv[:, None]
    assert w.dtype == np.float32
    return w


def all_keys(num_scenes, grid):
    """The ascending keys of a level in which every cell of every scene is occupied."""
    return np.arange(int(num_scenes) * int(grid) ** 3, dtype=np.int64)


# ---- the model in fp64 on the CPU

def _bn(x, sd, p, training):
    return F.batch_norm(x, sd[p + ".running_mean"].clone(), sd[p + ".running_var"].clone(), sd[p + ".weight"],
                        sd[p + ".bias"], training, 0.1, 1e-5)


def _res(x, sd, p, training):
    h = torch.relu(_bn(F.conv3d(x, sd[p + ".conv1.weight"], padding=1), sd, p + ".bn1", training))
    return torch.relu(_bn(F.conv3d(h, sd[p + ".conv2.weight"], padding=1), sd, p + ".bn2", training) + x)


def unet(x, sd, depth, training=True, prefix="unet."):
    """VoxelUNet / SparseUNet at full occupancy on x fp64 [B, C, G, G, G] from the fp64 state dict sd."""
    skips = []
    for l in range(depth):
        e = _res(x, sd, f"{prefix}enc.{l}", training)
        skips.append(e)
        x = torch.relu(_bn(F.conv3d(e, sd[f"{prefix}down.{l}.weight"], stride=2), sd, f"{prefix}down_bn.{l}", training))
    x = _res(x, sd, f"{prefix}bottom", training)
    for l in reversed(range(depth)):
        u = torch.relu(_bn(F.conv_transpose3d(x, sd[f"{prefix}up.{l}.weight"], stride=2), sd, f"{prefix}up_bn.{l}", training))
        m = F.conv3d(torch.cat([u, skips[l]], 1), sd[f"{prefix}merge.{l}.weight"], padding=1)
        x = _res(torch.relu(_bn(m, sd, f"{prefix}merge_bn.{l}", training)), sd, f"{prefix}dec.{l}", training)
    return x


def params64(state_dict):
    """The state dict in fp64 on the CPU, the floating-point parameters as leaves that take a gradient."""
    sd = {}
    for k, v in state_dict.items():
        v = v.detach().cpu()
        if not v.is_floating_point():
            sd[k] = v
        elif k.endswith(("running_mean", "running_var")):
            sd[k] = v.double()
        else:
            sd[k] = v.double().clone().requires_grad_()
    return sd


def model_logits(sd, points, offsets, grid, lo, hi, training=True, lift="mean", in_channels=4):
    """fp64 logits [T, K] of the model with the (params64) state dict sd on a batch."""
    G, B = int(grid), len(offsets) - 1
    own, corner, weight = dense_trilinear_index(points, offsets, G, lo, hi)
    V = B * G ** 3
    P = torch.from_numpy(np.asarray(points, np.float64))[:, :in_channels]
    z = torch.relu(P @ sd["lift.weight"].T + sd["lift.bias"])
    C = z.shape[1]
    own_t = torch.from_numpy(own.astype(np.int64))
    if lift == "mean":
        cnt = torch.zeros(V, dtype=torch.float64).index_add_(0, own_t, torch.ones(len(own), dtype=torch.float64))
        x = torch.zeros(V, C, dtype=torch.float64).index_add_(0, own_t, z) / cnt.clamp_min(1.0)[:, None]
    else:
        x = torch.zeros(V, C, dtype=torch.float64).scatter_reduce(0, own_t[:, None].expand(-1, C), z, "amax",
                                                                   include_self=True)   # relu(z) >= 0: zero rows stay
    depth = sum(1 for k in sd if k.startswith("unet.down.") and k.endswith(".weight"))
    y = unet(x.view(B, G, G, G, C).permute(0, 4, 1, 2, 3), sd, depth, training)
    rows = y.permute(0, 2, 3, 4, 1).reshape(V, C)
    ct = torch.from_numpy(corner.astype(np.int64))
    wt = torch.from_numpy(weight) * (ct >= 0)
    feats = (rows[ct.clamp_min(0)] * wt[:, :, None]).sum(1)
    return feats @ sd["head.weight"].T + sd["head.bias"]


def model_loss(sd, points, labels, offsets, grid, lo, hi, class_weight=None, training=True, lift="mean", in_channels=4):
    """(loss, logits) in fp64: the weighted cross-entropy of the labels (-1 ignored)."""
    logits = model_logits(sd, points, offsets, grid, lo, hi, training, lift, in_channels)
    w = None if class_weight is None else torch.as_tensor(class_weight, dtype=torch.float64)
    return F.cross_entropy(logits, torch.as_tensor(np.asarray(labels), dtype=torch.int64), weight=w, ignore_index=-1), logits
