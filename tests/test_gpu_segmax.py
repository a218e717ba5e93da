"""The segmented max on MI355X (pcs_amd.segmax; csrc/segmax.hip) against the fp64 statement
tests/segmax_refs.py with no tolerance: pcs_rows_segmax / pcs_rows_argselect directly and through
segment_max on hand-made segments (lengths around the kernel's unroll, missing entries, a single-column
NaN, exact ties, an all -inf segment), every channel form and dtype pair, then voxel_max and
sparse_max_pool forward and backward on the device's own maps, the pool also against F.max_pool3d on
the CPU.  A max is exact: values (after the one round-to-nearest-even cast of an fp32 -> bf16 store),
picked rows and gradients are compared with array_equal.  Build-defined: the reference has no voxel grid."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import point_head_refs as ph
import segmax_refs as sm
import sparse_stride_refs as ss

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BF, F32 = torch.bfloat16, torch.float32
PAIRS = [(BF, BF), (BF, F32), (F32, BF), (F32, F32)]


def _dev(a, dtype=F32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _idx(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().float().cpu().numpy()


def _stored(ref, dtype):
    """The fp64 statement's values as the device stores them: exact in fp32 (the inputs are fp32 or
    bf16 values), one RNE rounding into bf16."""
    r = np.asarray(ref, np.float64).astype(np.float32)
    return ph.bf16_exact(r) if dtype == BF else r


def _same(got, ref, dtype):
    return np.array_equal(_np(got), _stored(ref, dtype), equal_nan=True)


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


_SEG = {}


def _segments(shuffled, C, xdtype):
    """(src, seg_off, seg_of, R, x float32 [R, C], its fp64 pick) of a case, built once."""
    key = (shuffled, C, xdtype)
    if key not in _SEG:
        src, seg_off, seg_of, R = sm.segments(0, shuffled=shuffled)
        x = sm.segment_rows(C, R, C, src, seg_off)
        if xdtype == F32:
            x = x * np.float32(1.001)          # no longer bf16 values; equal values stay equal
        _SEG[key] = (src, seg_off, seg_of, R, x, sm.segment_max(x, src, seg_off))
    return _SEG[key]


@pytest.mark.parametrize("shuffled", [True, False], ids=["src", "rows"])
@pytest.mark.parametrize("xdtype,ydtype", PAIRS, ids=["bf16-bf16", "bf16-f32", "f32-bf16", "f32-f32"])
@pytest.mark.parametrize("C", [8, 64, 96, 2048])
def test_entry_points_are_exact(C, xdtype, ydtype, shuffled):
    import pcs_amd._lib as L
    src, seg_off, seg_of, R, x, (y_ref, arg_ref) = _segments(shuffled, C, xdtype)
    M, s = sm.SEG_M, L.stream_ptr(DEV)
    xt, st, ot, sf = _dev(x, xdtype), _idx(src), _idx(seg_off), _idx(seg_of)
    runs = []
    for _ in range(2):
        y = torch.full((M, C), 7.0, dtype=ydtype, device=DEV)
        arg = torch.full((M, C), 7, dtype=torch.int32, device=DEV)
        L.call("pcs_rows_segmax", xt, L.dtype_code(xdtype), st, ot, M, C, y, L.dtype_code(ydtype), arg, s)
        runs.append((y, arg))
    (y, arg), (y2, arg2) = runs
    torch.cuda.synchronize()
    assert torch.equal(_bits(y), _bits(y2)) and torch.equal(arg, arg2)
    assert _same(y, y_ref, ydtype)
    assert np.array_equal(arg.cpu().numpy(), arg_ref)
    only = torch.full((M, C), 7.0, dtype=ydtype, device=DEV)
    L.call("pcs_rows_segmax", xt, L.dtype_code(xdtype), st, ot, M, C, only, L.dtype_code(ydtype), None, s)
    assert torch.equal(_bits(only), _bits(y))
    # the cases are there: one NaN, in its column alone; -inf kept; a segment without a present row
    got = _np(y)
    assert np.isnan(got).sum() == 1 and np.isnan(got[sm.NAN_SEG, sm.NAN_COL]) and np.isneginf(got[sm.INF_SEG]).all()
    empty = np.diff(seg_off) == 0
    if shuffled:
        empty[sm.GONE_SEG] = True
    assert empty.sum() >= 2 and not got[empty].any() and (arg.cpu().numpy()[empty] == -1).all()
    # the backward: the gradient's dtype is the output's, dX's the input's
    dY = ph.rows(200 + C, M, C)
    dyt = _dev(dY, ydtype)
    dx = torch.full((R, C), 7.0, dtype=xdtype, device=DEV)
    dx2 = torch.full((R, C), 3.0, dtype=xdtype, device=DEV)
    for out in (dx, dx2):
        L.call("pcs_rows_argselect", dyt, L.dtype_code(ydtype), arg, sf, R, C, out, L.dtype_code(xdtype), s)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dx), _bits(dx2))
    assert _same(dx, sm.argselect(dY, arg_ref, seg_of, R), xdtype)


@pytest.mark.parametrize("shuffled", [True, False], ids=["src", "rows"])
@pytest.mark.parametrize("xdtype,ydtype", PAIRS, ids=["bf16-bf16", "bf16-f32", "f32-bf16", "f32-f32"])
@pytest.mark.parametrize("C", [64, 20])
def test_segment_max_forward_and_backward(C, xdtype, ydtype, shuffled):
    """Through the autograd function; C = 20 runs zero-padded to 24 channels."""
    from pcs_amd.segmax import segment_max
    src, seg_off, seg_of, R, x, (y_ref, arg_ref) = _segments(shuffled, C, xdtype)
    dY = ph.rows(300 + C, sm.SEG_M, C)
    outs = []
    for _ in range(2):
        xt = _dev(x, xdtype).requires_grad_()
        y = segment_max(xt, _idx(src), _idx(seg_off), _idx(seg_of), out_dtype=ydtype)
        y.backward(_dev(dY, ydtype))
        outs.append((y.detach(), xt.grad))
    torch.cuda.synchronize()
    (y, dx), (y2, dx2) = outs
    assert y.dtype == ydtype and tuple(y.shape) == (sm.SEG_M, C) and dx.dtype == xdtype and tuple(dx.shape) == (R, C)
    assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(dx), _bits(dx2))
    assert _same(y, y_ref, ydtype)
    assert _same(dx, sm.argselect(dY, arg_ref, seg_of, R), xdtype)
    assert segment_max(_dev(x, xdtype), _idx(src), _idx(seg_off), _idx(seg_of)).dtype == xdtype   # out_dtype None


def test_rejects_bad_inputs():
    from pcs_amd.segmax import point_lift_max, segment_max, sparse_max_pool, voxel_max
    src, seg_off, seg_of, R, x, _ = _segments(True, 8, F32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        segment_max(torch.from_numpy(x), None, torch.from_numpy(seg_off), torch.from_numpy(seg_of))
    with pytest.raises(ValueError):
        segment_max(_dev(x), _idx(src), _idx(seg_off), _idx(seg_of)[:-1])
    with pytest.raises(ValueError):
        segment_max(_dev(x), _idx(src).long(), _idx(seg_off), _idx(seg_of))
    with pytest.raises(ValueError):
        segment_max(_dev(x).half(), _idx(src), _idx(seg_off), _idx(seg_of))
    lv = _level(8, 0.4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        voxel_max(torch.zeros(lv["T"], 8), lv["pvm"])
    with pytest.raises(ValueError):
        voxel_max(torch.zeros(lv["T"] + 1, 8, device=DEV), lv["pvm"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sparse_max_pool(torch.zeros(lv["V"], 8), lv["link"])
    with pytest.raises(ValueError):
        sparse_max_pool(torch.zeros(lv["V"] + 1, 8, device=DEV), lv["link"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        point_lift_max(torch.zeros(lv["T"], 4), torch.zeros(8, 4), None, lv["pvm"])


# ---- on the device's own maps
_LEVELS = {}


def _level(grid, occupancy):
    if (grid, occupancy) not in _LEVELS:
        from pcs_amd.data import ragged_collate
        from pcs_amd.pointvoxel import point_voxel_map
        from pcs_amd.sparse import coarsen, sparse_voxels
        from pcs_amd.voxel import voxelize
        rb = ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in sm.clouds(grid, occupancy)])
        sv = sparse_voxels(rb, voxelize(rb, grid, ph.LO, ph.HI), ph.LO, ph.HI)
        svc, link = coarsen(sv)
        pvm = point_voxel_map(rb, sv, ph.LO, ph.HI)
        _LEVELS[grid, occupancy] = dict(
            grid=grid, pvm=pvm, link=link, T=pvm.num_points, V=pvm.num_voxels, Vc=svc.num_voxels,
            own=pvm.own.cpu().numpy(), keys=sv.keys.cpu().numpy(), ckeys=svc.keys.cpu().numpy(),
            child=link.child.cpu().numpy(), parent=link.parent.cpu().numpy())
    return _LEVELS[grid, occupancy]


def _tied_rows(seed, n, C):
    """bf16-exact half-integers: most maxima are met more than once."""
    return (np.round(ph.rows(seed, n, C) * 2.0) / 2.0).astype(np.float32)


@pytest.mark.parametrize("grid,occupancy", [(8, 0.4), (16, 0.3)])
@pytest.mark.parametrize("xdtype,ydtype", [(BF, BF), (F32, BF), (F32, F32)], ids=["bf16-bf16", "f32-bf16", "f32-f32"])
def test_voxel_max_on_the_device_map(grid, occupancy, xdtype, ydtype):
    from pcs_amd.segmax import voxel_max
    lv, C = _level(grid, occupancy), 64
    P = _tied_rows(grid, lv["T"], C) if xdtype == BF else ph.rows(grid, lv["T"], C) * np.float32(1.001)
    dV = ph.rows(grid + 1, lv["V"], C)
    y_ref, arg_ref = sm.voxel_max(P, lv["own"], lv["V"])
    pt = _dev(P, xdtype).requires_grad_()
    y = voxel_max(pt, lv["pvm"], out_dtype=ydtype)
    y.backward(_dev(dV, ydtype))
    torch.cuda.synchronize()
    assert y.dtype == ydtype and tuple(y.shape) == (lv["V"], C) and pt.grad.dtype == xdtype
    assert _same(y, y_ref, ydtype)
    assert _same(pt.grad, sm.argselect(dV, arg_ref, lv["own"], lv["T"]), xdtype)
    assert voxel_max(_dev(P, xdtype), lv["pvm"]).dtype == BF      # the default, as voxel_mean's


@pytest.mark.parametrize("grid,occupancy", [(8, 0.4), (16, 0.3)])
@pytest.mark.parametrize("xdtype", [BF, F32], ids=["bf16", "f32"])
def test_sparse_max_pool_on_the_device_link(grid, occupancy, xdtype):
    from pcs_amd.segmax import SparseMaxPool3d, sparse_max_pool
    lv, C, B = _level(grid, occupancy), 64, 3
    Vf, Vc, G = lv["V"], lv["Vc"], grid
    x = _tied_rows(grid + 2, Vf, C)
    dY = ph.rows(grid + 3, Vc, C)
    xt = _dev(x, xdtype).requires_grad_()
    y = sparse_max_pool(xt, lv["link"])
    y.backward(_dev(dY, xdtype))
    torch.cuda.synchronize()
    assert y.dtype == xdtype and tuple(y.shape) == (Vc, C)
    y_ref, arg_ref = sm.sparse_max_pool(x, lv["child"])
    assert _same(y, y_ref, xdtype)
    assert _same(xt.grad, sm.argselect(dY, arg_ref, lv["parent"], Vf), xdtype)
    assert torch.equal(SparseMaxPool3d()(_dev(x, xdtype), lv["link"]), y.detach())
    # ... and nn.MaxPool3d(2, 2) itself, on a dense grid that holds -inf at the unoccupied cells
    s, ix, iy, iz = ss.decode(lv["keys"], G)
    dense = torch.full((B, C, G, G, G), -np.inf)
    dense[s, :, ix, iy, iz] = torch.from_numpy(x)
    dense.requires_grad_()
    out = F.max_pool3d(dense, 2, 2)
    cs, cx, cy, cz = ss.decode(lv["ckeys"], G // 2)
    up = torch.zeros_like(out)
    up[cs, :, cx, cy, cz] = torch.from_numpy(dY)
    out.backward(up)
    assert np.array_equal(_np(y), out[cs, :, cx, cy, cz].detach().numpy())
    assert np.array_equal(_np(xt.grad), dense.grad[s, :, ix, iy, iz].numpy())
