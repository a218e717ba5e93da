"""tests/segmax_refs.py against torch on the CPU: segment_max against torch.max over each segment
(values, indices, autograd), sparse_max_pool against F.max_pool3d(2, 2, return_indices=True) on a dense
grid that holds -inf at the unoccupied cells, the max lift against autograd through torch.max on padded
voxels, and the share of undecided elements of the inputs the GPU test of the lift runs.  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import point_head_refs as ph
import segmax_refs as sm
import sparse_stride_refs as ss

TOL = 1e-12
C = 8


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max() if a.size else 0.0
    assert err <= TOL * max(1.0, np.abs(b).max() if b.size else 0.0), (what, err)


def _case(shuffled):
    src, seg_off, seg_of, R = sm.segments(0, shuffled=shuffled)
    return src, seg_off, seg_of, R, sm.segment_rows(1, R, C, src, seg_off)


def _present(src, seg_off, m):
    j = np.arange(seg_off[m], seg_off[m + 1])
    s = j if src is None else src[j].astype(np.int64)
    return s[s >= 0]


@pytest.mark.parametrize("shuffled", [True, False])
def test_segments_have_their_edges(shuffled):
    src, seg_off, seg_of, R, x = _case(shuffled)
    assert len(seg_off) == sm.SEG_M + 1 and set(np.diff(seg_off)) == set(sm.SEG_LENGTHS)
    assert np.isnan(x).sum() == 1 and np.isinf(x).any()
    if shuffled:
        assert (src < 0).any() and (src[seg_off[sm.GONE_SEG]:seg_off[sm.GONE_SEG + 1]] < 0).all()
        assert (seg_of < 0).any() and len(np.unique(src[src >= 0])) == (src >= 0).sum()   # a row in one segment, once
    else:
        assert src is None and R == seg_off[-1]


@pytest.mark.parametrize("shuffled", [True, False])
def test_segment_max_is_torch_max_over_each_segment(shuffled):
    src, seg_off, seg_of, R, x = _case(shuffled)
    y, arg = sm.segment_max(x, src, seg_off)
    xt = torch.from_numpy(x).double().requires_grad_()
    dY = ph.rows(2, sm.SEG_M, C).astype(np.float64)
    total = 0.0
    for m in range(sm.SEG_M):
        rows = _present(src, seg_off, m)
        if len(rows) == 0:
            assert not y[m].any() and (arg[m] == -1).all()
            continue
        val, idx = torch.max(xt[torch.from_numpy(rows)], dim=0)
        assert np.array_equal(y[m], val.detach().numpy(), equal_nan=True), m
        assert np.array_equal(arg[m], rows[idx.numpy()]), m
        total = total + (val * torch.from_numpy(dY[m])).sum()
    total.backward()
    assert np.array_equal(sm.argselect(dY, arg, seg_of, R), xt.grad.numpy())
    assert not sm.argselect(dY, arg, seg_of, R)[seg_of < 0].any()


@pytest.mark.parametrize("shuffled", [True, False])
def test_nan_ties_and_inf_stay_in_their_columns(shuffled):
    src, seg_off, _, R, x = _case(shuffled)
    row = (lambda j: j) if src is None else (lambda j: int(src[j]))
    y, arg = sm.segment_max(x, src, seg_off)
    nan_row = row(int(seg_off[sm.NAN_SEG]) + 2)
    clean = x.copy()
    clean[nan_row, sm.NAN_COL] = 0.0
    y0, arg0 = sm.segment_max(clean, src, seg_off)
    other = np.ones_like(y, bool)
    other[sm.NAN_SEG, sm.NAN_COL] = False
    assert np.array_equal(y[other], y0[other]) and np.array_equal(arg[other], arg0[other])   # the neighbours are untouched
    assert np.isnan(y[sm.NAN_SEG, sm.NAN_COL]) and arg[sm.NAN_SEG, sm.NAN_COL] == nan_row and np.isnan(y).sum() == 1
    j0 = int(seg_off[sm.TIE_SEG])
    want = np.full(C, row(j0 + 3))
    want[1] = row(j0 + 20)
    assert np.array_equal(arg[sm.TIE_SEG], want) and y[sm.TIE_SEG, 0] == 9.0 and y[sm.TIE_SEG, 1] == 10.0
    assert np.isneginf(y[sm.INF_SEG]).all() and (arg[sm.INF_SEG] == row(int(seg_off[sm.INF_SEG]))).all()


def test_sparse_max_pool_is_max_pool3d_on_the_occupied_cells():
    G, B, Cp = 8, 3, 6
    _, _, keys = sm.cpu_level(G, 0.4)
    ckeys, _, child, parent, _ = ss.coarse_maps(keys, G)
    Vf, Vc = len(keys), len(ckeys)
    rng = np.random.default_rng(3)
    x = np.round(rng.standard_normal((Vf, Cp)) * 2.0) / 2.0            # half-integers: many exact ties
    dY = rng.standard_normal((Vc, Cp))
    y, arg = sm.sparse_max_pool(x, child)
    assert ((child >= 0).sum(1) >= 2).any() and ((child >= 0).sum(1) < 8).any()
    s, ix, iy, iz = ss.decode(keys, G)
    dense = torch.full((B, Cp, G, G, G), -np.inf, dtype=torch.float64)
    dense[s, :, ix, iy, iz] = torch.from_numpy(x)
    dense.requires_grad_()
    out, idx = F.max_pool3d(dense, 2, 2, return_indices=True)
    cs, cx, cy, cz = ss.decode(ckeys, G // 2)
    assert np.array_equal(y, out[cs, :, cx, cy, cz].detach().numpy())
    flat = idx[cs, :, cx, cy, cz].numpy()                               # [Vc, Cp]: the cell's index in its scene's G^3
    fine_row = {int(k): i for i, k in enumerate(keys)}
    want = np.array([[fine_row[int(cs[m]) * G ** 3 + int(flat[m, c])] for c in range(Cp)] for m in range(Vc)])
    ties = sum(int((x[child[m][child[m] >= 0], c] == y[m, c]).sum() > 1) for m in range(Vc) for c in range(Cp))
    assert ties > 20                                                    # the tap order is max_pool3d's scan order
    assert np.array_equal(arg, want)
    up = torch.zeros_like(out)
    up[cs, :, cx, cy, cz] = torch.from_numpy(dY)
    out.backward(up)
    assert np.array_equal(sm.argselect(dY, arg, parent, Vf), dense.grad[s, :, ix, iy, iz].numpy())
    unocc = torch.ones(B, G, G, G, dtype=torch.bool)
    unocc[s, ix, iy, iz] = False
    assert not dense.grad.permute(0, 2, 3, 4, 1)[unocc].any()


def _padded_max(P, W, b, own, V):
    """(relu(max z) [V, C] with zero rows for the voxels without points, w, bt) through torch.max on
    [V, longest, C] padded with -inf."""
    w, bt = torch.from_numpy(W).double().requires_grad_(), torch.from_numpy(b).double().requires_grad_()
    z = F.linear(torch.from_numpy(P).double()[:, :W.shape[1]], w, bt)
    order, seg_off, _ = ph.points_by_voxel(own, V)
    n = int(seg_off[-1])
    vox = np.repeat(np.arange(V), np.diff(seg_off))
    slot = np.arange(n) - seg_off[vox]
    pad = torch.full((V, max(int(np.diff(seg_off).max()), 1), W.shape[0]), -np.inf, dtype=torch.float64)
    pad = pad.index_put((torch.from_numpy(vox), torch.from_numpy(slot)), z[torch.from_numpy(order[:n].astype(np.int64))])
    y = torch.relu(torch.max(pad, dim=1).values)
    has = torch.from_numpy(np.diff(seg_off) > 0)
    return torch.where(has[:, None], y, torch.zeros_like(y)), w, bt


@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_lift_max_matches_autograd_through_torch_max(name):
    p4, own, _, _, V = ph.cpu_map(name)
    W, b = sm.lift_max_params(16, 1)
    dV = ph.rows(3, V, 16)
    y, w, bt = _padded_max(p4, W, b, own, V)
    (y * torch.from_numpy(dV).double()).sum().backward()
    _close(sm.point_lift_max(p4, W, b, own, V), y.detach().numpy(), "Y")
    g = sm.point_lift_max_grad(dV, p4, W, b, own, V)
    _close(g["dW"], w.grad.numpy(), "dW")
    _close(g["db"], bt.grad.numpy(), "db")
    assert (g["abs_dW"] >= np.abs(g["dW"]) - 1e-12).all() and (g["amb_dW"] >= 0).all()
    order, seg_off, _ = ph.points_by_voxel(own, V)
    relu_then_max, _ = sm.voxel_max(np.maximum(p4[:, :4].astype(np.float64) @ W.astype(np.float64).T + b, 0.0), own, V)
    _close(sm.point_lift_max(p4, W, b, own, V), relu_then_max, "max relu = relu max")
    if name == "C":
        assert (np.diff(seg_off) == 0).any() and (own < 0).any()


@pytest.mark.parametrize("grid,occupancy,per_voxel", sm.LIFT_INPUTS + [(8, 0.4, 3)])
@pytest.mark.parametrize("w0", [64, 96])
def test_undecided_share_of_the_gpu_inputs(grid, occupancy, per_voxel, w0):
    """The (voxel, channel) elements whose pick or gate a correct fp32 evaluation may take either way
    are at most UNDECIDED_CAP of all, for exactly the inputs of tests/test_gpu_lift_max.py: the cap is
    a condition on the inputs, not a measurement of the device."""
    pts, own, keys = sm.cpu_level(grid, occupancy, per_voxel)
    W, b = sm.lift_max_params(w0)
    order, seg_off, _ = ph.points_by_voxel(own, len(keys))
    und = sm.lift_max(pts, sm.LIFT_CIN, W, b, order, seg_off)["undecided"]
    print(f"undecided: {int(und.sum())} of {und.size} ({und.mean():.2e}); longest segment {int(np.diff(seg_off).max())}")
    assert und.mean() <= sm.UNDECIDED_CAP
