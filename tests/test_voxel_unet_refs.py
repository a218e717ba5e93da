"""tests/voxel_unet_refs.py checked on the CPU: the dense trilinear index against the occupied-voxel
statement of tests/point_voxel_refs.py with every cell given as occupied, its behaviour at the places
the index can go wrong, its read-out against F.grid_sample, and the dense model's state dict against the
sparse model's."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_voxel_refs as pv  # noqa: E402
import voxel_unet_refs as vr  # noqa: E402

LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def _points(grid, seed=0, n=(37, 22)):
    """Two ragged scenes: random points (some outside the box) followed by point_voxel_refs' edge points."""
    rng = np.random.default_rng(seed)
    scenes = []
    for m in n:
        p = np.zeros((m, 4), np.float32)
        p[:, :3] = rng.uniform(-1.15, 1.15, (m, 3)).astype(np.float32)
        scenes.append(np.concatenate([p, pv.edge_points(grid)]))
    off = np.cumsum([0] + [len(s) for s in scenes]).astype(np.int64)
    return np.concatenate(scenes), off


@pytest.mark.parametrize("grid", [1, 2, 5, 8])
def test_dense_index_is_the_sparse_statement_on_a_full_level(grid):
    pts, off = _points(grid)
    own, corner, weight = vr.dense_trilinear_index(pts, off, grid, LO, HI)
    so, sc, sw = pv.trilinear_index(pts, off, vr.all_keys(2, grid), grid, LO, HI)
    assert own.dtype == np.int32 and corner.dtype == np.int32 and weight.dtype == np.float64
    assert np.array_equal(own, so) and np.array_equal(corner, sc) and np.array_equal(weight, sw)
    # the float32 evaluation order of the device against the float64 weights: ten roundings of values <= 1
    w32 = vr.dense_trilinear_weight32(pts, off, grid, LO, HI)
    assert w32.dtype == np.float32 and np.abs(w32.astype(np.float64) - weight).max() < 2e-6
    assert np.array_equal(w32 > 0, weight > 0)


@pytest.mark.parametrize("grid", [1, 2, 5, 8])
def test_dense_index_properties(grid):
    G = grid
    pts, off = _points(G, seed=1)
    own, corner, weight = vr.dense_trilinear_index(pts, off, G, LO, HI)
    T, n0 = len(pts), int(off[1])
    scene = (np.arange(T) >= n0).astype(np.int64)
    # every point has its own cell, in its own scene; outside points are clamped onto the border cells
    assert (own >= 0).all() and np.array_equal(own // G ** 3, scene)
    present = corner >= 0
    assert np.array_equal(np.where(present, corner // G ** 3, scene[:, None]), np.broadcast_to(scene[:, None], (T, 8)))
    # the own cell is always one of the corners; the weights are a partition of one over the present ones
    assert (corner == own[:, None]).any(axis=1).all()
    assert (weight[~present] == 0).all() and (weight >= 0).all()
    assert np.allclose(weight.sum(1), 1.0, atol=1e-12)
    # a corner is missing only outside the grid: the cell b + a computed apart from the statement
    u = ((pts[:, :3].astype(np.float64) + 1.0) / 2.0) * G
    b = np.floor(np.clip(u, 0, G) - 0.5).astype(np.int64)
    for k in range(8):
        j = b + np.array([(k >> 2) & 1, (k >> 1) & 1, k & 1])
        inside = ((j >= 0) & (j < G)).all(axis=1)
        exact = np.abs((np.clip(u, 0, G) - 0.5) - np.round(np.clip(u, 0, G) - 0.5)).min(axis=1) > 1e-5   # off the planes
        assert np.array_equal(present[exact, k], inside[exact]), k


def test_dense_index_at_hand_made_points():
    G = 4
    h = 2.0 / G
    centre = -1.0 + 1.5 * h          # the centre of cell 1
    face = -1.0 + 2.0 * h            # the face between cells 1 and 2
    rows = np.array([
        (centre, centre, centre),    # a cell centre: the whole weight on the own cell
        (face, centre, centre),      # on a face along x: half each to cells 1 and 2, own is the upper cell
        (-1.0, -1.0, -1.0),          # the low corner of the box: cell 0 alone, the other corners are outside
        (1.0, 1.0, 1.0),             # the high corner: own clamps to G - 1
        (-5.0, centre, 7.0),         # outside: clamped to the border cells
    ], np.float32)
    pts = np.zeros((len(rows), 4), np.float32)
    pts[:, :3] = rows
    own, corner, weight = vr.dense_trilinear_index(pts, np.array([0, len(rows)], np.int64), G, LO, HI)
    cell = lambda x, y, z: (x * G + y) * G + z   # noqa: E731
    assert own.tolist() == [cell(1, 1, 1), cell(2, 1, 1), cell(0, 0, 0), cell(3, 3, 3), cell(0, 1, 3)]
    assert weight[0, corner[0] == cell(1, 1, 1)].sum() == 1.0 and np.count_nonzero(weight[0]) == 1
    w1 = {int(c): w for c, w in zip(corner[1], weight[1]) if w > 0}
    assert w1 == {cell(1, 1, 1): 0.5, cell(2, 1, 1): 0.5}
    assert (corner[2] >= 0).sum() == 1 and corner[2, 7] == cell(0, 0, 0) and weight[2, 7] == 1.0
    assert (corner[3] >= 0).sum() == 1 and corner[3, 0] == cell(3, 3, 3) and weight[3, 0] == 1.0
    assert {int(c) for c, w in zip(corner[4], weight[4]) if w > 0} == {cell(0, 1, 3)}
    with pytest.raises(AssertionError):   # the sparse statement on a level without cell 0 loses that point
        assert (pv.trilinear_index(pts, np.array([0, len(rows)]), vr.all_keys(1, G)[1:], G, LO, HI)[0] >= 0).all()


def test_dense_readout_is_grid_sample():
    """On a dense grid the normalised eight-corner read-out is F.grid_sample(mode="bilinear",
    padding_mode="border", align_corners=False) (pcs_amd.pointvoxel's docstring), for points in the box."""
    G, C = 5, 3
    rng = np.random.default_rng(3)
    pts = np.zeros((64, 4), np.float32)
    pts[:, :3] = rng.uniform(-1, 1, (64, 3)).astype(np.float32)
    _, corner, weight = vr.dense_trilinear_index(pts, np.array([0, 64], np.int64), G, LO, HI)
    X = rng.standard_normal((G ** 3, C))
    got = pv.devoxelize(X, corner, weight)
    vol = torch.from_numpy(X).view(1, G, G, G, C).permute(0, 4, 1, 2, 3)            # [1, C, D = x, H = y, W = z]
    q = torch.from_numpy(pts[:, [2, 1, 0]].astype(np.float64)).view(1, 64, 1, 1, 3)  # grid_sample takes (W, H, D)
    ref = F.grid_sample(vol, q, mode="bilinear", padding_mode="border", align_corners=False).view(C, 64).T
    assert np.allclose(got, ref.numpy(), atol=1e-6)                                 # float32 u, float64 after it


def test_fp64_model_statement_runs_and_differentiates():
    """The restatement against the plain torch modules it is made of: one residual block and the whole
    model's shape, and a gradient for every parameter."""
    from pcs_amd.voxel_unet import VoxelUNetSegmentation
    torch.manual_seed(0)
    model = VoxelUNetSegmentation(4, 3, (32, 64), grid=4)
    sd = vr.params64(model.state_dict())
    x = torch.randn(2, 32, 4, 4, 4, dtype=torch.float64)
    c1, c2 = torch.nn.Conv3d(32, 32, 3, padding=1, bias=False).double(), torch.nn.Conv3d(32, 32, 3, padding=1, bias=False).double()
    b1, b2 = torch.nn.BatchNorm3d(32).double(), torch.nn.BatchNorm3d(32).double()
    sub ={"r.conv1.weight": c1.weight, "r.conv2.weight": c2.weight}
    for n, b in (("bn1", b1), ("bn2", b2)):
        sub.update({f"r.{n}.{k}": v for k, v in b.state_dict().items()})
    assert torch.allclose(vr._res(x, sub, "r", True), torch.relu(b2(c2(torch.relu(b1(c1(x))))) + x), atol=1e-12)
    pts, off = _points(4, seed=2)
    labels = np.random.default_rng(0).integers(-1, 3, len(pts))
    for lift in ("mean", "max"):
        loss, logits = vr.model_loss(sd, pts, labels, off, 4, LO, HI, [1.0, 2.0, 0.5], lift=lift)
        assert logits.shape == (len(pts), 3) and logits.dtype == torch.float64 and torch.isfinite(loss)
    loss.backward()
    for k, v in sd.items():
        if v.requires_grad:
            assert v.grad is not None and torch.isfinite(v.grad).all() and v.grad.abs().max() > 0, k


@pytest.mark.parametrize("widths", [(32, 64), (32, 64, 128), (64,)])
def test_state_dict_is_the_sparse_models(widths):
    from pcs_amd.sparse_unet import SparseUNetSegmentation
    from pcs_amd.voxel_unet import VoxelUNetSegmentation
    torch.manual_seed(1)
    dense = VoxelUNetSegmentation(4, 3, widths, grid=8)
    sparse = SparseUNetSegmentation(4, 3, widths, grid=8)
    assert list(dense.state_dict()) == list(sparse.state_dict())
    assert [tuple(v.shape) for v in dense.state_dict().values()] == [tuple(v.shape) for v in sparse.state_dict().values()]
    assert [k for k, _ in dense.named_parameters()] == [k for k, _ in sparse.named_parameters()]
    assert not any(k.endswith("conv1.bias") or k.endswith("merge.0.bias") for k in dense.state_dict())
    before = {k: v.clone() for k, v in dense.state_dict().items()}
    sparse.load_state_dict(dense.state_dict())
    assert all(torch.equal(v, before[k]) for k, v in sparse.state_dict().items())
    fresh = VoxelUNetSegmentation(4, 3, widths, grid=8)
    fresh.load_state_dict(sparse.state_dict())
    assert all(torch.equal(v, before[k]) for k, v in fresh.state_dict().items())
    with pytest.raises(ValueError, match="divisible"):
        VoxelUNetSegmentation(4, 3, (32, 64, 128), grid=6)
    with pytest.raises(ValueError, match="lift"):
        VoxelUNetSegmentation(lift="sum")
