"""Stride-2 sparse down / up convolutions on MI355X (pcs_amd.sparse.coarsen, sparse_conv3d_down,
sparse_conv_transpose3d_up; pcs_sparse_coarse_*, pcs_sparse_conv_rows): the coarse maps bit-exact
against tests/sparse_stride_refs.py; both layers, forward and all three gradients, against torch's
dense conv3d(stride=2) / conv_transpose3d(stride=2) in fp64 on a grid that is zero off the occupied
voxels, read at the represented sites.  Build-defined: the reference has no voxel grid."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sparse_oracle as so
import sparse_stride_refs as sr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def _sparse(seed, n_scenes, grid, occupancy):
    from pcs_amd.data import jittered_clouds, ragged_collate
    from pcs_amd.sparse import sparse_voxels
    from pcs_amd.voxel import voxelize
    clouds = jittered_clouds(seed, n_scenes, grid=grid, occupancy=occupancy, per_voxel=2)
    rb = ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in clouds])
    return sparse_voxels(rb, voxelize(rb, grid, *BOX), *BOX)


def _from_keys(keys, grid):
    from pcs_amd.sparse import sparse_from_keys
    return sparse_from_keys(torch.from_numpy(np.asarray(keys, dtype=np.int64)).to(DEV), grid)


def _check_maps(sv, svc, link):
    keys, G = sv.keys.cpu().numpy(), sv.grid
    ckeys, tap, child, parent, up = sr.coarse_maps(keys, G)
    assert svc.grid == G // 2 and (link.fine, link.coarse) == (len(keys), len(ckeys))
    assert np.array_equal(svc.keys.cpu().numpy(), ckeys)
    assert np.array_equal(link.tap.cpu().numpy(), tap) and link.tap.dtype == torch.int32
    assert np.array_equal(link.child.cpu().numpy(), child) and link.child.dtype == torch.int32
    assert np.array_equal(link.parent.cpu().numpy(), parent) and link.parent.dtype == torch.int32
    assert np.array_equal(link.up.cpu().numpy(), up) and link.up.dtype == torch.int32
    # the coarse level is a sparse level like any other: its own table and 27-neighbour map
    assert np.array_equal(svc.nbr.cpu().numpy(), so.neighbors(ckeys, G // 2))
    assert np.array_equal(svc.find(svc.keys).cpu().numpy(), np.arange(len(ckeys)))


@pytest.mark.parametrize("grid,occupancy", [(8, 0.4), (16, 0.1), (32, 0.02)])
def test_coarse_maps_bit_exact(grid, occupancy):
    from pcs_amd.sparse import coarsen
    sv = _sparse(31 + grid, 3, grid, occupancy)
    svc, link = coarsen(sv)
    _check_maps(sv, svc, link)
    if grid == 32:                               # G -> G/2 -> G/4
        svcc, link2 = coarsen(svc)
        _check_maps(svc, svcc, link2)
        assert svcc.grid == 8 and link2.fine == link.coarse


def test_coarse_maps_keep_scenes_apart():
    """The last cell of scene 0 and the first cell of scene 1 are neighbours in key order only."""
    from pcs_amd.sparse import coarsen
    G = 8
    G3 = G ** 3
    key = lambda s, x, y, z: s * G3 + (x * G + y) * G + z  # noqa: E731
    keys = sorted({key(0, 7, 7, 7), key(0, 7, 7, 6), key(0, 6, 6, 6), key(0, 0, 0, 0), key(1, 0, 0, 0),
                   key(1, 0, 0, 1), key(1, 1, 1, 1), key(1, 7, 7, 7), key(2, 3, 4, 5)})
    sv = _from_keys(keys, G)
    svc, link = coarsen(sv)
    _check_maps(sv, svc, link)
    ck = svc.keys.cpu().numpy().tolist()
    assert ck == [0, 63, 64, 127, 128 + (1 * 4 + 2) * 4 + 2]
    child = link.child.cpu().numpy()
    assert (child[1] >= 0).sum() == 3 and (child[2] >= 0).sum() == 3   # scene 0's last cell, scene 1's first


def test_coarsen_rejects_an_odd_grid():
    from pcs_amd.sparse import coarsen
    sv = _from_keys([0, 5, 30], 7)
    with pytest.raises(ValueError):
        coarsen(sv)


@pytest.fixture(params=["gather", "pairs", "default"])
def conv_path(request, monkeypatch):
    """Both forms of the 8-tap gather through the child map (the down forward, the up input
    gradient) and of the down weight gradient, as test_gpu_sparse.py's fixture, and the module's
    own choice."""
    import pcs_amd.sparse as S
    if request.param != "default":
        monkeypatch.setattr(S, "PAIR_TAPS_MAX", 0.0 if request.param == "gather" else 27.0)
        monkeypatch.setattr(S, "PAIR_WGRAD", request.param == "pairs")
    return request.param


def _rel(a, r):
    return float((a.double().cpu() - r).abs().max() / r.abs().max().clamp_min(1e-30))


def _dense(x, idx, grid, B):
    d = torch.zeros(B, x.shape[1], grid, grid, grid, dtype=torch.float64)
    d[idx[0], :, idx[1], idx[2], idx[3]] = x.double().cpu()
    return d


CASES = [(16, 0.3, 64, 64), (32, 0.05, 64, 128), (16, 0.2, 4, 32), (24, 0.1, 32, 64)]
_LEVELS = {}


def _levels(grid, occupancy, cin):
    """(sv, svc, link, fine index, coarse index) of a case, built once."""
    from pcs_amd.sparse import coarsen
    k = (grid, occupancy, cin)
    if k not in _LEVELS:
        sv = _sparse(5 + cin + grid, 2, grid, occupancy)
        svc, link = coarsen(sv)
        _LEVELS[k] = (sv, svc, link, sr.decode(sv.keys.cpu().numpy(), grid), sr.decode(svc.keys.cpu().numpy(), grid // 2))
    return _LEVELS[k]


def _run_layer(up, grid, occupancy, cin, cout, out_dtype):
    """The layer on the device and torch's dense layer in fp64: (y, dw, db, dx) of each."""
    from pcs_amd.sparse import sparse_conv3d_down, sparse_conv_transpose3d_up
    sv, svc, link, fidx, cidx = _levels(grid, occupancy, cin)
    (n_in, iidx, gin), (n_out, oidx) = ((link.coarse, cidx, grid // 2), (link.fine, fidx)) if up else \
        ((link.fine, fidx, grid), (link.coarse, cidx))
    g = torch.Generator().manual_seed(cin + cout + int(up))
    x = torch.randn(n_in, cin, generator=g).to(torch.bfloat16)
    wshape = (cin, cout, 2, 2, 2) if up else (cout, cin, 2, 2, 2)
    w = (torch.randn(*wshape, generator=g) * 0.05).to(torch.bfloat16).float()   # bf16-exact
    b = torch.randn(cout, generator=g) * 0.1
    dy = torch.randn(n_out, cout, generator=g).to(torch.bfloat16)
    xd = _dense(x, iidx, gin, 2).requires_grad_()
    wr, br = w.double().requires_grad_(), b.double().requires_grad_()
    yd = F.conv_transpose3d(xd, wr, br, stride=2) if up else F.conv3d(xd, wr, br, stride=2)
    ref = yd[oidx[0], :, oidx[1], oidx[2], oidx[3]]
    ref.backward(dy.double())
    xs = x.to(DEV).requires_grad_()
    ws, bs = w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    fn = sparse_conv_transpose3d_up if up else sparse_conv3d_down
    y = fn(xs, ws, link, bs, out_dtype=out_dtype)
    assert y.dtype == out_dtype and y.shape == (n_out, cout)
    y.backward(dy.to(DEV).to(out_dtype))
    torch.cuda.synchronize()
    got = (y.detach(), ws.grad, bs.grad, xs.grad)
    want = (ref.detach(), wr.grad, br.grad, xd.grad[iidx[0], :, iidx[1], iidx[2], iidx[3]])
    return got, want, (x, w, b, link)


@pytest.mark.parametrize("up", [False, True], ids=["down", "up"])
@pytest.mark.parametrize("grid,occupancy,cin,cout", CASES)
def test_layers_match_dense_fp64(grid, occupancy, cin, cout, up, conv_path):
    (y, dw, db, dx), (ry, rdw, rdb, rdx), (x, w, b, link) = _run_layer(up, grid, occupancy, cin, cout, torch.float32)
    assert _rel(y, ry) < 1e-5
    assert _rel(dw, rdw) < 1e-5
    assert _rel(db, rdb) < 1e-5
    assert dx.dtype == torch.bfloat16
    assert _rel(dx.float(), rdx) < 8e-3                     # dx stored in bf16
    # and the numpy restatement on the maps
    if up:
        mine = sr.up_conv(x.double().numpy(), w.numpy(), b.numpy(), link.parent.cpu().numpy(), link.tap.cpu().numpy())
    else:
        mine = sr.down_conv(x.double().numpy(), w.numpy(), b.numpy(), link.child.cpu().numpy())
    assert _rel(y, torch.from_numpy(mine)) < 1e-5
    if conv_path != "default":
        assert link.use_pairs() == (conv_path == "pairs")   # the form the 8-tap gather ran in


@pytest.mark.parametrize("up", [False, True], ids=["down", "up"])
def test_layers_bf16_output(up):
    (y, dw, db, dx), (ry, rdw, rdb, rdx), _ = _run_layer(up, 24, 0.1, 32, 64, torch.bfloat16)
    assert _rel(y.float(), ry) < 8e-3                       # y stored in bf16
    assert _rel(dw, rdw) < 1e-5 and _rel(db, rdb) < 1e-5
    assert _rel(dx.float(), rdx) < 8e-3


def _tap_counted_keys(counts, G=16):
    """Keys on a G grid (one scene) with exactly counts[t] voxels at tap t, in distinct cells."""
    Gc = G // 2
    rng = np.random.default_rng(7)
    keys = []
    for t, n in enumerate(counts):
        a, b, c = (t >> 2) & 1, (t >> 1) & 1, t & 1
        cells = rng.permutation(Gc ** 3)[:n]
        cx, cy, cz = cells // (Gc * Gc), (cells // Gc) % Gc, cells % Gc
        keys.append(((2 * cx + a) * G + 2 * cy + b) * G + 2 * cz + c)
    return np.sort(np.concatenate(keys)).astype(np.int64)


@pytest.mark.parametrize("counts", [(512, 0, 0, 0, 0, 0, 0, 0), (1, 63, 64, 65, 0, 129, 0, 200)],
                         ids=["tap0-only", "tile-edges"])
def test_conv_rows_tile_edges(counts):
    """pcs_sparse_conv_rows on taps of exactly 1, 63, 64, 65 and 0 pairs (64-pair tiles): empty
    taps launch no tile, ragged tiles write only their own rows."""
    from pcs_amd.sparse import coarsen, sparse_conv3d_down, sparse_conv_transpose3d_up
    sv = _from_keys(_tap_counted_keys(counts), 16)
    assert sv.num_voxels == sum(counts)
    svc, link = coarsen(sv)
    tap_off = link.up_pairs()[3]
    assert [tap_off[t + 1] - tap_off[t] for t in range(8)] == list(counts)
    parent, tap = link.parent.cpu().numpy(), link.tap.cpu().numpy()
    g = torch.Generator().manual_seed(3)
    # the up forward
    x = torch.randn(link.coarse, 64, generator=g).to(torch.bfloat16)
    u = (torch.randn(64, 64, 2, 2, 2, generator=g) * 0.05).to(torch.bfloat16).float()
    b = torch.randn(64, generator=g) * 0.1
    y = sparse_conv_transpose3d_up(x.to(DEV), u.to(DEV), link, b.to(DEV), out_dtype=torch.float32)
    assert _rel(y, torch.from_numpy(sr.up_conv(x.double().numpy(), u.numpy(), b.numpy(), parent, tap))) < 1e-5
    # the down input gradient: dx[f] = W_tap(f)^T dy[parent[f]], the up convolution with w as u
    w = (torch.randn(64, 64, 2, 2, 2, generator=g) * 0.05).to(torch.bfloat16).float()
    dy = torch.randn(link.coarse, 64, generator=g).to(torch.bfloat16)
    xf = torch.randn(link.fine, 64, generator=g).to(torch.bfloat16).to(DEV).requires_grad_()
    sparse_conv3d_down(xf, w.to(DEV), link, None, out_dtype=torch.float32).backward(dy.float().to(DEV))
    assert _rel(xf.grad.float(), torch.from_numpy(sr.up_conv(dy.double().numpy(), w.numpy(), None, parent, tap))) < 8e-3


@pytest.mark.parametrize("up", [False, True], ids=["down", "up"])
def test_layers_are_deterministic(up):
    a, _, _ = _run_layer(up, 24, 0.1, 32, 64, torch.float32)
    b, _, _ = _run_layer(up, 24, 0.1, 32, 64, torch.float32)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_sparse_unet_trains():
    """An occupied-only two-level U-Net (module API): finite gradients, falling loss."""
    from pcs_amd.sparse import SparseDownConv3d, SparseUpConv3d, SubMConv3d, coarsen
    torch.manual_seed(0)
    sv = _sparse(21, 2, 24, 0.15)
    svc, link = coarsen(sv)
    enc, down, mid = SubMConv3d(4, 32).to(DEV), SparseDownConv3d(32, 64).to(DEV), SubMConv3d(64, 64).to(DEV)
    up, dec = SparseUpConv3d(64, 32).to(DEV), SubMConv3d(64, 32).to(DEV)
    params = [p for m in (enc, down, mid, up, dec) for p in m.parameters()]
    opt = torch.optim.SGD(params, lr=0.05)
    x = torch.randn(sv.num_voxels, 4, device=DEV).to(torch.bfloat16)
    target = torch.randn(sv.num_voxels, 32, device=DEV) * 0.1
    act = lambda t: torch.relu(t).to(torch.bfloat16)  # noqa: E731
    losses = []
    for _ in range(8):
        e = act(enc(x, sv, out_dtype=torch.float32))
        c = act(down(e, link, out_dtype=torch.float32))
        c = act(mid(c, svc, out_dtype=torch.float32))
        u = act(up(c, link, out_dtype=torch.float32))
        y = dec(torch.cat([u, e], dim=1), sv, out_dtype=torch.float32)
        loss = ((y - target) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0]
