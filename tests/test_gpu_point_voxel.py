"""Point <-> voxel transfer on MI355X (pcs_amd.pointvoxel; pcs_trilinear_index, pcs_rows_interp,
pcs_rows_segsum): the index bit-exact against tests/point_voxel_refs.py, every operator forward and
backward against the fp64 statement on the device's own maps and against torch's grid_sample on a
fully occupied grid, the segment and empty-row edges, determinism, and a point-voxel network that
trains on a per-point loss.  Build-defined: the reference has no voxel grid."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import point_voxel_refs as pv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
BF, F32 = torch.bfloat16, torch.float32


def _rb(clouds):
    """(RaggedBatch, points [T, 4], offsets [B + 1]) of a list of (points, labels) numpy clouds."""
    from pcs_amd.data import ragged_collate
    rb = ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in clouds])
    off = np.concatenate([[0], np.cumsum([len(p) for p, _ in clouds])]).astype(np.int64)
    return rb, np.concatenate([p for p, _ in clouds]).astype(np.float32), off


def _clouds(seed, n_scenes, grid, occupancy, edges=False):
    from pcs_amd.data import jittered_clouds
    out = []
    for p, l in jittered_clouds(seed, n_scenes, grid=grid, occupancy=occupancy, per_voxel=3):
        if edges:
            e = pv.edge_points(grid)
            p, l = np.concatenate([p, e]), np.concatenate([l, np.zeros(len(e), np.int64)])
        out.append((p, l))
    return out


def _level(rb, grid):
    from pcs_amd.sparse import sparse_voxels
    from pcs_amd.voxel import voxelize
    vb = voxelize(rb, grid, LO, HI)
    return vb, sparse_voxels(rb, vb, LO, HI)


def _map(rb, sv):
    from pcs_amd.pointvoxel import point_voxel_map
    return point_voxel_map(rb, sv, LO, HI)


def _check_index(pvm, pts, off, keys, grid):
    own, corner, weight = pv.trilinear_index(pts, off, keys, grid, LO, HI)
    assert pvm.own.dtype == torch.int32 and pvm.corner.dtype == torch.int32 and pvm.weight.dtype == F32
    assert np.array_equal(pvm.own.cpu().numpy(), own)
    assert np.array_equal(pvm.corner.cpu().numpy(), corner)
    err = np.abs(pvm.weight.cpu().numpy().astype(np.float64) - weight).max()
    print(f"weight max abs err {err:.3e}")
    assert err < 2e-6        # ten fp32 roundings of values <= 1 give 6e-7; three times that
    return own, corner, weight


@pytest.mark.parametrize("grid,occupancy", [(8, 0.4), (16, 0.3), (32, 0.02)])
def test_index_bit_exact(grid, occupancy):
    from pcs_amd.sparse import coarsen
    rb, pts, off = _rb(_clouds(17 + grid, 3, grid, occupancy, edges=True))
    vb, sv = _level(rb, grid)
    pvm = _map(rb, sv)
    own, corner, _ = _check_index(pvm, pts, off, sv.keys.cpu().numpy(), grid)
    assert torch.equal(pvm.own.long(), vb.voxel_of_point)            # the level came from these points
    assert torch.equal(pvm.counts, vb.counts)
    assert ((corner == own[:, None]).sum(axis=1) == 1).all()
    # the coarse level, same points
    svc, link = coarsen(sv)
    pvc = _map(rb, svc)
    _check_index(pvc, pts, off, svc.keys.cpu().numpy(), grid // 2)
    assert torch.equal(pvc.own, link.parent[vb.voxel_of_point])
    # query points the level was not built from
    qb, qpts, qoff = _rb(_clouds(91 + grid, 3, grid, min(2 * occupancy, 0.6), edges=True))
    qown, _, _ = _check_index(_map(qb, sv), qpts, qoff, sv.keys.cpu().numpy(), grid)
    assert (qown < 0).any() and (qown >= 0).any()


# ---- the operators against the fp64 statement, on the device's own maps
def _rel(a, r):
    r = torch.as_tensor(r)
    return float((a.double().cpu() - r).abs().max() / r.abs().max().clamp_min(1e-30))


def _bound(dtype):
    return 1e-5 if dtype == F32 else 8e-3      # fp32 accumulate; a bf16 store rounds to 8 bits


_SHARED = {}


def _shared():
    """One level (16^3, 3 scenes), its own points and a query set, the maps of both on the device and
    as numpy: built once, never changed."""
    if not _SHARED:
        rb, _, _ = _rb(_clouds(5, 3, 16, 0.3))
        _, sv = _level(rb, 16)
        qb, _, _ = _rb(_clouds(6, 3, 16, 0.5, edges=True))
        for name, b in (("own", rb), ("query", qb)):
            m = _map(b, sv)
            _SHARED[name] = (m, m.own.cpu().numpy(), m.corner.cpu().numpy(), m.weight.cpu().numpy().astype(np.float64))
    return _SHARED


def _run_ops(pvm, c, in_dtype, out_dtype, seed=0):
    """Forward and gradient of the three operators on the device: a dict of tensors, and the
    (bf16-exact) inputs they ran on as float64 numpy."""
    from pcs_amd.pointvoxel import devoxelize, voxel_mean
    T, V = pvm.num_points, pvm.num_voxels
    g = torch.Generator().manual_seed(seed + c)
    mk = lambda n: torch.randn(n, c, generator=g).to(BF).float()     # noqa: E731  exact in every dtype
    P, X, dV, dY = mk(T), mk(V), mk(V), mk(T)
    out = {}
    p = P.to(DEV).to(in_dtype).requires_grad_()
    v = voxel_mean(p, pvm, out_dtype=out_dtype)
    v.backward(dV.to(DEV).to(out_dtype))
    out["mean"], out["mean_grad"] = v.detach(), p.grad
    for mode in ("trilinear", "nearest"):
        x = X.to(DEV).to(in_dtype).requires_grad_()
        y = devoxelize(x, pvm, mode=mode, out_dtype=out_dtype)
        y.backward(dY.to(DEV).to(out_dtype))
        out[mode], out[mode + "_grad"] = y.detach(), x.grad
    torch.cuda.synchronize()
    for k, t in out.items():
        want = (T if k in ("mean_grad", "trilinear", "nearest") else V, c)
        assert tuple(t.shape) == want, (k, t.shape)
        assert t.dtype == (in_dtype if k.endswith("_grad") else out_dtype), (k, t.dtype)
    return out, tuple(t.double().numpy() for t in (P, X, dV, dY))


def _check_ops(out, inputs, own, corner, weight, V, in_dtype, out_dtype):
    P, X, dV, dY = inputs
    T = len(own)
    want = {"mean": pv.voxel_mean(P, own, V), "mean_grad": pv.voxel_mean_t(dV, own, T),
            "trilinear": pv.devoxelize(X, corner, weight), "trilinear_grad": pv.devoxelize_t(dY, corner, weight, V),
            "nearest": pv.nearest(X, own), "nearest_grad": pv.nearest_t(dY, own, V)}
    for k, r in want.items():
        e = _rel(out[k], r)
        print(f"{k}: rel err {e:.3e}")
        assert e < _bound(in_dtype if k.endswith("_grad") else out_dtype), k


OP_CASES = [(c, BF, F32) for c in (8, 64, 72, 4, 20)] + [(64, BF, BF), (64, F32, BF), (64, F32, F32)]


@pytest.mark.parametrize("which", ["own", "query"])
@pytest.mark.parametrize("c,in_dtype,out_dtype", OP_CASES,
                         ids=[f"C{c}-{str(i)[6:]}-{str(o)[6:]}" for c, i, o in OP_CASES])
def test_operators_match_fp64(c, in_dtype, out_dtype, which):
    pvm, own, corner, weight = _shared()[which]
    out, inputs = _run_ops(pvm, c, in_dtype, out_dtype)
    _check_ops(out, inputs, own, corner, weight, pvm.num_voxels, in_dtype, out_dtype)


def test_operators_are_deterministic():
    """Two runs of every forward and backward, the map (and its CSRs) rebuilt between them."""
    rb, _, _ = _rb(_clouds(5, 3, 16, 0.3))
    _, sv = _level(rb, 16)
    qb, _, _ = _rb(_clouds(6, 3, 16, 0.5, edges=True))
    for b in (rb, qb):
        for in_dtype, out_dtype in ((BF, BF), (F32, F32)):
            a, _ = _run_ops(_map(b, sv), 64, in_dtype, out_dtype)
            c, _ = _run_ops(_map(b, sv), 64, in_dtype, out_dtype)
            for k in a:
                assert torch.equal(a[k], c[k]), k


@pytest.mark.parametrize("in_dtype,out_dtype", [(F32, F32), (BF, BF)], ids=["f32", "bf16"])
def test_full_grid_matches_grid_sample(in_dtype, out_dtype):
    """On a fully occupied 6^3 grid devoxelize is grid_sample(bilinear, border, align_corners=False)
    on the dense [B, C, G(x), G(y), G(z)] grid, coordinates in the order (z, y, x)."""
    from pcs_amd.pointvoxel import devoxelize
    from pcs_amd.sparse import sparse_from_keys
    G, B, n, C = 6, 2, 200, 8
    rng = np.random.default_rng(0)
    pts = np.zeros((B * n, 4), np.float32)
    pts[:, :3] = rng.uniform(-1.2, 1.2, size=(B * n, 3))             # some outside the box
    e = pv.edge_points(G)
    pts[: len(e)] = e
    lab = np.zeros(n, np.int64)
    rb, _, _ = _rb([(pts[:n], lab), (pts[n:], lab)])
    sv = sparse_from_keys(torch.arange(B * G ** 3, dtype=torch.int64, device=DEV), G)
    pvm = _map(rb, sv)
    assert int(pvm.own.min()) >= 0
    g = torch.Generator().manual_seed(1)
    X = torch.randn(B * G ** 3, C, generator=g).to(BF).float()
    dY = torch.randn(B * n, C, generator=g).to(BF).float()
    dense = X.double().reshape(B, G, G, G, C).permute(0, 4, 1, 2, 3).contiguous().requires_grad_()
    xyz = torch.from_numpy(pts[:, :3].astype(np.float64)).reshape(B, n, 1, 1, 3)
    ref = F.grid_sample(dense, xyz.flip(-1), mode="bilinear", padding_mode="border", align_corners=False)
    ref = ref.reshape(B, C, n).permute(0, 2, 1).reshape(B * n, C)
    ref.backward(dY.double())
    rgrad = dense.grad.permute(0, 2, 3, 4, 1).reshape(B * G ** 3, C)
    x = X.to(DEV).to(in_dtype).requires_grad_()
    y = devoxelize(x, pvm, out_dtype=out_dtype)
    y.backward(dY.to(DEV).to(out_dtype))
    ey, eg = _rel(y.detach(), ref.detach()), _rel(x.grad, rgrad)
    print(f"forward rel err {ey:.3e}, gradient rel err {eg:.3e}")
    assert ey < _bound(out_dtype) and eg < _bound(in_dtype)


def _counted_cloud(counts, grid=16, seed=3):
    """One scene whose voxels hold exactly these point counts, in cells three apart (no voxel is a
    corner of another's points), points shuffled."""
    rng = np.random.default_rng(seed)
    h = 2.0 / grid
    pts = []
    for i, n in enumerate(counts):
        cell = np.array([1 + 3 * i, 2, 1 + 3 * (i % 2)], np.float64)
        pts.append(-1.0 + (cell + rng.uniform(0.05, 0.95, size=(n, 3))) * h)
    p = np.zeros((sum(counts), 4), np.float32)
    p[:, :3] = rng.permutation(np.concatenate(pts))
    return p, np.zeros(len(p), np.int64)


def test_segment_edges_and_empty_rows():
    """Segments of exactly 1, 63, 64, 65 and 300 rows (a wave is 64 lanes, four rows in flight), and
    voxels no query point touches: their rows are exactly zero."""
    from pcs_amd.pointvoxel import devoxelize, voxel_mean
    counts = (1, 63, 64, 65, 300)
    rb, pts, off = _rb([_counted_cloud(counts)])
    vb, sv = _level(rb, 16)
    assert sorted(vb.counts.tolist()) == sorted(counts)
    pvm = _map(rb, sv)
    assert torch.equal(pvm.counts, vb.counts)
    for in_dtype, out_dtype in ((F32, F32), (BF, BF)):
        out, inputs = _run_ops(pvm, 64, in_dtype, out_dtype, seed=9)
        _check_ops(out, inputs, pvm.own.cpu().numpy(), pvm.corner.cpu().numpy(),
                   pvm.weight.cpu().numpy().astype(np.float64), pvm.num_voxels, in_dtype, out_dtype)
    # a query set inside two of the five voxels, and far from all of them
    keep = vb.voxel_of_point.cpu().numpy()
    q = np.concatenate([pts[np.isin(keep, [1, 3])][:40], np.array([[0.9, 0.9, 0.9, 1.0], [-0.9, 0.9, -0.9, 1.0]], np.float32)])
    qb, _, _ = _rb([(q, np.zeros(len(q), np.int64))])
    qm = _map(qb, sv)
    own, corner = qm.own.cpu().numpy(), qm.corner.cpu().numpy()
    touched = np.zeros(sv.num_voxels, bool)
    touched[corner[corner >= 0]] = True
    assert touched.sum() == 2 and (own[-2:] < 0).all()
    out, inputs = _run_ops(qm, 64, F32, F32, seed=10)
    _check_ops(out, inputs, own, corner, qm.weight.cpu().numpy().astype(np.float64), sv.num_voxels, F32, F32)
    untouched = torch.from_numpy(~touched).to(DEV)
    for k in ("mean", "trilinear_grad", "nearest_grad"):
        assert out[k][untouched].abs().max() == 0, k                 # written, as zero rows
        assert out[k][~untouched].abs().max(dim=1)[0].min() > 0, k
    assert voxel_mean(torch.ones(len(q), 3, device=DEV), qm, out_dtype=F32)[untouched].abs().max() == 0
    assert devoxelize(torch.ones(sv.num_voxels, 3, device=DEV), qm)[-2:].abs().max() == 0


def test_query_points_outside_the_occupied_set():
    """own == -1: zero devoxelize rows, zero voxel_mean gradient."""
    pvm, own, corner, _ = _shared()["query"]
    off_level = torch.from_numpy(own < 0).to(DEV)
    no_corner = torch.from_numpy((corner < 0).all(axis=1)).to(DEV)
    assert off_level.any() and no_corner.any() and (~off_level).any()
    out, _ = _run_ops(pvm, 64, BF, F32, seed=4)
    assert out["nearest"][off_level].abs().max() == 0
    assert out["trilinear"][no_corner].abs().max() == 0
    assert out["mean_grad"][off_level].abs().max() == 0
    assert out["mean_grad"][~off_level].abs().max(dim=1)[0].min() > 0


def test_rejects_bad_inputs():
    from pcs_amd.pointvoxel import devoxelize, voxel_mean
    pvm = _shared()["own"][0]
    T, V = pvm.num_points, pvm.num_voxels
    with pytest.raises(RuntimeError, match="HIP device only"):
        voxel_mean(torch.zeros(T, 8), pvm)
    with pytest.raises(RuntimeError, match="HIP device only"):
        devoxelize(torch.zeros(V, 8), pvm)
    with pytest.raises(ValueError):
        devoxelize(torch.zeros(V, 8, device=DEV), pvm, mode="cubic")
    with pytest.raises(ValueError):
        devoxelize(torch.zeros(V + 1, 8, device=DEV), pvm)
    with pytest.raises(ValueError):
        voxel_mean(torch.zeros(T + 1, 8, device=DEV), pvm)
    with pytest.raises(ValueError):
        voxel_mean(torch.zeros(T, 8, device=DEV, dtype=torch.float16), pvm)


def test_point_voxel_network_trains():
    """Linear on the raw points -> voxel_mean -> an occupied-only two-level U-Net -> devoxelize from
    both levels -> a per-point cross-entropy on the points' own labels: finite gradients down to
    the first Linear, falling loss."""
    from pcs_amd.pointvoxel import devoxelize, voxel_mean
    from pcs_amd.sparse import SparseDownConv3d, SparseUpConv3d, SubMConv3d, coarsen
    torch.manual_seed(0)
    rb, _, _ = _rb(_clouds(21, 2, 24, 0.15))
    _, sv = _level(rb, 24)
    svc, link = coarsen(sv)
    pvm, pvc = _map(rb, sv), _map(rb, svc)
    lift = torch.nn.Linear(4, 32).to(DEV)
    enc, down, mid = SubMConv3d(32, 32).to(DEV), SparseDownConv3d(32, 64).to(DEV), SubMConv3d(64, 64).to(DEV)
    up, head = SparseUpConv3d(64, 32).to(DEV), torch.nn.Linear(32 + 64 + 32, 2).to(DEV)
    mods = (lift, enc, down, mid, up, head)
    params = [p for m in mods for p in m.parameters()]
    opt = torch.optim.SGD(params, lr=0.05)
    raw = rb.points.to(DEV).float()
    labels = rb.labels.to(DEV)
    act = lambda t: torch.relu(t).to(BF)  # noqa: E731
    losses = []
    for _ in range(8):
        pf = torch.relu(lift(raw))                                   # fp32 [T, 32] per-point features
        e = act(enc(voxel_mean(pf, pvm), sv, out_dtype=F32))
        c = act(mid(act(down(e, link, out_dtype=F32)), svc, out_dtype=F32))
        u = act(up(c, link, out_dtype=F32))
        feats = torch.cat([pf, devoxelize(c, pvc), devoxelize(u + e, pvm)], dim=1)
        loss = F.cross_entropy(head(feats), labels, ignore_index=-1)
        opt.zero_grad()
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
        assert lift.weight.grad.abs().max() > 0
        opt.step()
        losses.append(loss.item())
    print("losses", [round(v, 4) for v in losses])
    assert losses[-1] < losses[0]
