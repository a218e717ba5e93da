"""The point <-> grid map of a dense grid (pcs_dense_trilinear_index, pcs_amd.voxel_unet.dense_point_map)
on MI355X: bit-equal to the numpy statement of tests/voxel_unet_refs.py, equal to point_voxel_map's on a
fully occupied level, and accepted unchanged by the point ends (voxel_mean, devoxelize,
point_head_loss)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_voxel_refs as pv  # noqa: E402
import voxel_unet_refs as vr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def _rb(scenes):
    from pcs_amd.data import ragged_collate
    rb = ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in scenes])
    off = np.concatenate([[0], np.cumsum([len(p) for p, _ in scenes])]).astype(np.int64)
    return rb, np.concatenate([p for p, _ in scenes]).astype(np.float32), off


def _scenes(grid, seed, n=(41, 23), spread=1.15):
    """Two ragged scenes: random points (some outside the box for spread > 1) and the points on faces, at
    centres, on the box faces and outside of point_voxel_refs.edge_points."""
    rng = np.random.default_rng(seed)
    out = []
    for m in n:
        p = np.zeros((m, 4), np.float32)
        p[:, :3] = rng.uniform(-spread, spread, (m, 3)).astype(np.float32)
        p[:, 3] = rng.uniform(0, 1, m).astype(np.float32)
        p = np.concatenate([p, pv.edge_points(grid)])
        out.append((p, rng.integers(-1, 2, len(p)).astype(np.int64)))
    return out


@pytest.mark.parametrize("grid", [1, 2, 5])
def test_index_is_the_numpy_statement(grid):
    from pcs_amd.voxel_unet import dense_point_map
    rb, pts, off = _rb(_scenes(grid, 10 + grid))
    assert off[1] - off[0] != off[2] - off[1]
    pvm = dense_point_map(rb, grid, LO, HI)
    own, corner, weight = vr.dense_trilinear_index(pts, off, grid, LO, HI)
    w32 = vr.dense_trilinear_weight32(pts, off, grid, LO, HI)
    assert pvm.num_voxels == 2 * grid ** 3 and pvm.num_points == len(pts)
    assert pvm.own.dtype == torch.int32 and pvm.corner.dtype == torch.int32 and pvm.weight.dtype == torch.float32
    assert np.array_equal(pvm.own.cpu().numpy(), own) and (own >= 0).all()
    assert np.array_equal(pvm.corner.cpu().numpy(), corner) and (corner < 0).any()
    got = pvm.weight.cpu().numpy()
    print(f"weight: max |device - float32 statement| {np.abs(got - w32).max():.3e}, "
          f"max |device - float64 weights| {np.abs(got.astype(np.float64) - weight).max():.3e}")
    assert np.array_equal(got, w32)
    assert np.abs(got.astype(np.float64) - weight).max() < 2e-6   # tests/test_gpu_point_voxel.py's bound


def _full_scenes(grid, seed, extra=3):
    """Every cell of the grid holds its centre point and a few random ones; two scenes of unequal size."""
    rng = np.random.default_rng(seed)
    h = 2.0 / grid
    ax = (-1.0 + (np.arange(grid) + 0.5) * h).astype(np.float32)
    centres = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    out = []
    for s in range(2):
        m = extra * grid ** 3 + 17 * s
        p = np.zeros((len(centres) + m, 4), np.float32)
        p[:len(centres), :3] = centres
        p[len(centres):, :3] = rng.uniform(-1, 1, (m, 3)).astype(np.float32)
        p[:, 3] = rng.uniform(0, 1, len(p)).astype(np.float32)
        p = p[rng.permutation(len(p))]
        out.append((p, rng.integers(-1, 2, len(p)).astype(np.int64)))
    return out


def test_equals_point_voxel_map_on_a_full_level():
    from pcs_amd.pointvoxel import point_voxel_map
    from pcs_amd.sparse import sparse_voxels
    from pcs_amd.voxel import voxelize
    from pcs_amd.voxel_unet import dense_point_map
    G = 4
    rb, pts, off = _rb(_full_scenes(G, 3))
    sv = sparse_voxels(rb, voxelize(rb, G, LO, HI), LO, HI)
    assert sv.num_voxels == 2 * G ** 3
    assert torch.equal(sv.keys.cpu().long(), torch.arange(2 * G ** 3))   # the dense row is the sparse row
    sparse, dense = point_voxel_map(rb, sv, LO, HI), dense_point_map(rb, G, LO, HI)
    assert sparse.num_voxels == dense.num_voxels
    assert torch.equal(dense.own, sparse.own) and torch.equal(dense.corner, sparse.corner)
    assert torch.equal(dense.weight, sparse.weight)
    # and the same map for query points the level was not built from, outside ones included
    qb, _, _ = _rb(_scenes(G, 4))
    sparse, dense = point_voxel_map(qb, sv, LO, HI), dense_point_map(qb, G, LO, HI)
    assert torch.equal(dense.own, sparse.own) and torch.equal(dense.corner, sparse.corner)
    assert torch.equal(dense.weight, sparse.weight)


def test_point_ends_run_on_the_dense_map():
    """voxel_mean, devoxelize and point_head_loss on a dense map with empty cells, against the fp64
    statements of tests/point_voxel_refs.py; gradients reach their inputs."""
    import torch.nn.functional as F
    from pcs_amd.pointhead import point_head_loss
    from pcs_amd.pointvoxel import devoxelize, voxel_mean
    from pcs_amd.voxel_unet import dense_point_map
    G, C, K = 5, 32, 3
    rb, pts, off = _rb(_scenes(G, 7, n=(60, 35)))
    pvm = dense_point_map(rb, G, LO, HI)
    own, corner, weight = vr.dense_trilinear_index(pts, off, G, LO, HI)
    V, T = 2 * G ** 3, len(pts)
    assert (np.bincount(own, minlength=V) == 0).any()                 # some cells are empty: zero rows
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(T, C, generator=g)
    p = feats.to(DEV).requires_grad_()
    v = voxel_mean(p, pvm, out_dtype=torch.float32)
    ref_v = pv.voxel_mean(feats.numpy(), own, V)
    assert tuple(v.shape) == (V, C)
    assert np.abs(v.detach().cpu().numpy() - ref_v).max() < 1e-5 * np.abs(ref_v).max()
    assert not v.detach()[torch.from_numpy(np.bincount(own, minlength=V) == 0).to(DEV)].any()
    x = torch.randn(V, C, generator=g)
    xd = x.to(DEV).requires_grad_()
    y = devoxelize(xd, pvm)
    ref_y = pv.devoxelize(x.numpy(), corner, weight)
    assert np.abs(y.detach().cpu().numpy() - ref_y).max() < 1e-5 * np.abs(ref_y).max()
    dv, dy = torch.randn(V, C, generator=g), torch.randn(T, C, generator=g)
    v.backward(dv.to(DEV))
    y.backward(dy.to(DEV))
    ref_dp, ref_dx = pv.voxel_mean_t(dv.numpy(), own, T), pv.devoxelize_t(dy.numpy(), corner, weight, V)
    assert np.abs(p.grad.cpu().numpy() - ref_dp).max() < 1e-5 * np.abs(ref_dp).max()
    assert np.abs(xd.grad.cpu().numpy() - ref_dx).max() < 1e-5 * np.abs(ref_dx).max()
    # the fused head and loss: against torch on the device's own devoxelize (each has its own fp64 test)
    w = (torch.randn(K, C, generator=g) * 0.2).to(DEV).requires_grad_()
    b = torch.randn(K, generator=g).to(DEV).requires_grad_()
    xh = x.to(DEV).requires_grad_()
    labels = rb.labels.to(DEV)
    assert (labels == -1).any() and (labels >= 0).any()
    cw = torch.tensor([1.0, 2.0, 0.5], device=DEV)
    loss, logits = point_head_loss(xh, pvm, w, b, labels, cw, return_logits=True)
    loss.backward()
    ref = F.cross_entropy(F.linear(devoxelize(x.to(DEV), pvm).double(), w.detach().double(), b.detach().double()), labels,
                          weight=cw.double(), ignore_index=-1)
    assert tuple(logits.shape) == (T, K) and abs(loss.item() - ref.item()) < 1e-5 * max(1.0, abs(ref.item()))
    for t in (xh, w, b):
        assert t.grad is not None and torch.isfinite(t.grad).all() and t.grad.abs().max() > 0
