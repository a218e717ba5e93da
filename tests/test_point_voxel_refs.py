"""tests/point_voxel_refs.py (the numpy statement of pcs_amd.pointvoxel) against independent
statements: voxel_oracle's voxel of a point, torch's grid_sample on a fully occupied grid, and the
transpose identities of both operators.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import point_voxel_refs as pv
import voxel_oracle as vo

LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def _cloud(seed, n_scenes, grid, occupancy, per_voxel=3, edges=True):
    """(points [T, 4], offsets [B + 1]) of jittered clouds, the edge points appended to each scene."""
    from pcs_amd.data import jittered_clouds
    clouds = [p for p, _ in jittered_clouds(seed, n_scenes, grid=grid, occupancy=occupancy, per_voxel=per_voxel)]
    if edges:
        clouds = [np.concatenate([p, pv.edge_points(grid)]) for p in clouds]
    off = np.concatenate([[0], np.cumsum([len(p) for p in clouds])]).astype(np.int64)
    return np.concatenate(clouds).astype(np.float32), off


@pytest.mark.parametrize("grid,occupancy", [(8, 0.4), (16, 0.3), (32, 0.02)])
def test_own_voxel_and_corners(grid, occupancy):
    pts, off = _cloud(11 + grid, 3, grid, occupancy)
    keys = pv.level_keys(pts, off, grid, LO, HI)
    own, corner, weight = pv.trilinear_index(pts, off, keys, grid, LO, HI)
    vop = vo.voxelize(pts, None, off, grid, LO, HI, 2)[0]
    assert np.array_equal(own, vop)                              # voxel_oracle's voxel of every point
    hit = corner == own[:, None]
    assert (hit.sum(axis=1) == 1).all()                          # the own voxel is one of the corners
    assert (weight[hit] >= 0.125 - 1e-6).all()                   # and carries at least 1/8
    assert np.allclose(weight.sum(axis=1), 1.0, atol=1e-12)
    assert (weight[corner < 0] == 0).all() and (weight >= 0).all()
    # corners are voxels of the point's own scene
    scene = np.searchsorted(off, np.arange(len(pts)), side="right") - 1
    ok = corner >= 0
    assert (keys[corner[ok]] // grid ** 3 == np.repeat(scene[:, None], 8, 1)[ok]).all()


@pytest.mark.parametrize("grid", [8, 16, 32])
def test_edge_points_sit_where_they_say(grid):
    e = pv.edge_points(grid)
    u = pv._u(e, grid, LO, HI)
    fi = max(grid // 4, 1)
    assert (u[9] == fi).all() and (np.floor(u[10]) == fi - 1).all() and (u[10] > fi - 1e-4).all()   # face, one ulp below
    assert (u[7] == grid // 2 + 0.5).all()                                                      # a cell centre
    assert (u[0] == 0).all() and (u[1] == grid).all() and (u[4:7] < 0).any() and (u[4:7] > grid).any()


def test_query_points_off_the_level():
    """Points the level was not built from: own and every corner may be missing; weights are then 0."""
    grid = 16
    pts, off = _cloud(3, 2, grid, 0.05, edges=False)
    keys = pv.level_keys(pts, off, grid, LO, HI)
    q, qoff = _cloud(4, 2, grid, 0.3)
    own, corner, weight = pv.trilinear_index(q, qoff, keys, grid, LO, HI)
    assert (own < 0).any() and (own >= 0).any()
    none = (corner < 0).all(axis=1)
    assert none.any() and (weight[none] == 0).all()
    assert (own[none] < 0).all()                                 # the own voxel is a corner
    # a point exactly on a cell-centre plane gives its far corners the raw weight 0: when only those
    # are occupied there is nothing to normalise and the weights stay 0 (the edge points do this)
    total = weight.sum(axis=1)
    assert np.allclose(total[own >= 0], 1.0, atol=1e-12)
    assert (np.isclose(total, 1.0, atol=1e-12) | (total == 0)).all()


def _full_grid(G, B, n, seed):
    rng = np.random.default_rng(seed)
    pts = np.zeros((B * n, 4), np.float32)
    pts[:, :3] = rng.uniform(-1.2, 1.2, size=(B * n, 3))         # some outside the box
    edges = pv.edge_points(G)
    pts[: len(edges)] = edges
    off = np.arange(B + 1, dtype=np.int64) * n
    keys = np.arange(B * G ** 3, dtype=np.int64)
    return pts, off, keys


def test_full_grid_matches_grid_sample():
    G, B, n, C = 6, 2, 200, 5
    pts, off, keys = _full_grid(G, B, n, 0)
    own, corner, weight = pv.trilinear_index(pts, off, keys, G, LO, HI)
    assert (own >= 0).all() and (corner.max(axis=1) >= 0).all()
    X = np.random.default_rng(1).standard_normal((B * G ** 3, C))
    dense = torch.from_numpy(X).reshape(B, G, G, G, C).permute(0, 4, 1, 2, 3)       # [B, C, G(x), G(y), G(z)]
    xyz = torch.from_numpy(pts[:, :3].astype(np.float64)).reshape(B, n, 1, 1, 3)
    ref = F.grid_sample(dense, xyz.flip(-1), mode="bilinear", padding_mode="border", align_corners=False)
    ref = ref.reshape(B, C, n).permute(0, 2, 1).reshape(B * n, C).numpy()
    got = pv.devoxelize(X, corner, weight)
    assert np.abs(got - ref).max() < 1e-5                       # float32 coordinates against float64 ones
    assert np.array_equal(pv.nearest(X, own), X[own])


def test_transpose_identities():
    grid = 8
    pts, off = _cloud(5, 2, grid, 0.3, edges=False)
    keys = pv.level_keys(pts, off, grid, LO, HI)
    q, qoff = _cloud(6, 2, grid, 0.5)
    rng = np.random.default_rng(2)
    for points, offsets in ((pts, off), (q, qoff)):
        own, corner, weight = pv.trilinear_index(points, offsets, keys, grid, LO, HI)
        T, V, C = len(points), len(keys), 3
        X, Gp = rng.standard_normal((V, C)), rng.standard_normal((T, C))
        P, Gv = rng.standard_normal((T, C)), rng.standard_normal((V, C))
        assert np.isclose((pv.devoxelize(X, corner, weight) * Gp).sum(), (X * pv.devoxelize_t(Gp, corner, weight, V)).sum(),
                          rtol=1e-12)
        assert np.isclose((pv.nearest(X, own) * Gp).sum(), (X * pv.nearest_t(Gp, own, V)).sum(), rtol=1e-12)
        assert np.isclose((pv.voxel_mean(P, own, V) * Gv).sum(), (P * pv.voxel_mean_t(Gv, own, T)).sum(), rtol=1e-12)
    # the mean itself, by hand
    own = np.array([1, 1, -1, 0, 1], np.int32)
    P = np.array([[1.0], [2.0], [100.0], [5.0], [6.0]])
    assert np.array_equal(pv.voxel_mean(P, own, 3), np.array([[5.0], [3.0], [0.0]]))
