"""The fused max lift on MI355X (pcs_amd.segmax.point_lift_max; csrc/pointhead.hip) against the fp64
statement tests/segmax_refs.py on the device's own maps: forward and backward, against the composition
voxel_max(relu(F.linear(...))) on the device, determinism and the voxels without points.

Bounds (tests/test_gpu_point_head.py's for the mean lift): fp32 outputs 1e-5 and bf16 stores 8e-3, max
error over max |reference|; dW and db 1e-5 of the fp64 sum of the absolute values of their terms, plus
the widening over the undecided elements (segmax_refs; tests/test_segmax_refs.py caps their share on
exactly these inputs)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import point_head_refs as ph
import segmax_refs as sm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BF, F32 = torch.bfloat16, torch.float32
SUM_TOL = 1e-5


def _dev(a, dtype=F32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _rb(clouds):
    from pcs_amd.data import ragged_collate
    return ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in clouds])


def _map(level, query):
    from pcs_amd.pointvoxel import point_voxel_map
    from pcs_amd.sparse import sparse_voxels
    from pcs_amd.voxel import voxelize
    grid, clouds = level
    rb = _rb(clouds)
    sv = sparse_voxels(rb, voxelize(rb, grid, ph.LO, ph.HI), ph.LO, ph.HI)
    pvm = point_voxel_map(_rb(query), sv, ph.LO, ph.HI)
    order, seg_off = pvm.points_by_voxel()[:2]
    return dict(pvm=pvm, points=ph.flat(query)[0], V=pvm.num_voxels, order=order.cpu().numpy(), seg_off=seg_off.cpu().numpy())


_REFS = {}


def _input(i, w0):
    """The device's map of LIFT_INPUTS[i], the parameters, an upstream gradient and the fp64 statement
    of both directions, built once."""
    if (i, w0) not in _REFS:
        grid, occupancy, per_voxel = sm.LIFT_INPUTS[i]
        clouds = sm.clouds(grid, occupancy, per_voxel)
        m = _map((grid, clouds), clouds)
        W, b = sm.lift_max_params(w0)
        dV = ph.rows(10 * i + w0, m["V"], w0)
        m.update(W=W, b=b, dV=dV, fwd=sm.lift_max(m["points"], sm.LIFT_CIN, W, b, m["order"], m["seg_off"]),
                 bwd=sm.lift_max_bwd(dV, m["points"], sm.LIFT_CIN, W, b, m["order"], m["seg_off"]))
        _REFS[i, w0] = m
    return _REFS[i, w0]


def _rel(got, ref):
    ref = np.asarray(ref, np.float64)
    got = got.detach().double().cpu().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)) if ref.size else 0.0


def _sum_excess(got, ref, abs_sum, extra):
    """max of |got - ref| - (SUM_TOL * abs_sum + extra): <= 0 passes; also the plain error for the log."""
    got = got.detach().double().cpu().numpy()
    ref, abs_sum = np.asarray(ref, np.float64), np.asarray(abs_sum, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref)
    return float((err - (SUM_TOL * abs_sum + extra)).max()), float((err / np.maximum(abs_sum, 1e-300)).max())


def _store_bound(dtype):
    return 1e-5 if dtype == F32 else 8e-3


def _run(m, out_dtype):
    from pcs_amd.segmax import point_lift_max
    w, bt = _dev(m["W"]).requires_grad_(), _dev(m["b"]).requires_grad_()
    y = point_lift_max(_dev(m["points"]), w, bt, m["pvm"], out_dtype=out_dtype)
    y.backward(_dev(m["dV"], out_dtype))
    torch.cuda.synchronize()
    return y.detach(), w.grad, bt.grad


@pytest.mark.parametrize("bf", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("w0", [64, 96])
@pytest.mark.parametrize("i", range(len(sm.LIFT_INPUTS)), ids=[str(c) for c in sm.LIFT_INPUTS])
def test_lift_max_matches_fp64(i, w0, bf):
    m, out_dtype = _input(i, w0), BF if bf else F32
    y, dw, db = _run(m, out_dtype)
    y2, dw2, db2 = _run(m, out_dtype)
    assert y.dtype == out_dtype and tuple(y.shape) == (m["V"], w0) and tuple(dw.shape) == (w0, sm.LIFT_CIN)
    assert torch.equal(y, y2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    g = m["bwd"]
    e = _rel(y, m["fwd"]["Y"])
    xw, ew = _sum_excess(dw, g["dW"], g["abs_dW"], g["amb_dW"])
    xb, eb = _sum_excess(db, g["db"], g["abs_db"], g["amb_db"])
    print(f"Y rel err {e:.3e}; dW err / sum|term| {ew:.3e}; db {eb:.3e}; undecided {int(g['undecided'].sum())} of "
          f"{g['undecided'].size}, their widening of dW at most {g['amb_dW'].max():.3e}")
    assert g["undecided"].mean() <= sm.UNDECIDED_CAP
    assert e < _store_bound(out_dtype)
    assert xw <= 0 and xb <= 0


@pytest.mark.parametrize("bf", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("i,w0", [(0, 64), (1, 96)])
def test_lift_max_matches_the_composition_on_the_device(i, w0, bf):
    """voxel_max(relu(F.linear(points, W, b))): the Linear in fp64 (its fp32 rounding is voxel_max's
    input), so that what differs from the fused form is the fused form's own arithmetic."""
    from pcs_amd.segmax import voxel_max
    m, out_dtype = _input(i, w0), BF if bf else F32
    y, dw, db = _run(m, out_dtype)
    w, bt = _dev(m["W"]).double().requires_grad_(), _dev(m["b"]).double().requires_grad_()
    z = F.linear(_dev(m["points"]).double(), w, bt).float()
    yc = voxel_max(torch.relu(z), m["pvm"], out_dtype=out_dtype)
    yc.backward(_dev(m["dV"], out_dtype))
    torch.cuda.synchronize()
    g = m["bwd"]
    e = _rel(y, yc.detach().double().cpu().numpy())
    xw, ew = _sum_excess(dw, w.grad.cpu().numpy(), g["abs_dW"], g["amb_dW"])
    xb, eb = _sum_excess(db, bt.grad.cpu().numpy(), g["abs_db"], g["amb_db"])
    print(f"fused against composed: Y {e:.3e}, dW {ew:.3e}, db {eb:.3e}")
    assert e < _store_bound(out_dtype) and xw <= 0 and xb <= 0


def test_voxels_without_points_are_zero_rows():
    """A level queried with points it was not built from (point_head_refs' case C): voxels without
    points, points without a voxel."""
    from pcs_amd.segmax import point_lift_max
    grid, level, query = ph.case_clouds("C")
    m = _map((grid, level), query)
    empty = np.diff(m["seg_off"]) == 0
    assert empty.any() and (m["pvm"].own < 0).any()
    W, b = sm.lift_max_params(64, 2)
    dV = ph.rows(77, m["V"], 64)
    m.update(W=W, b=b, dV=dV)
    y, dw, db = _run(m, F32)
    assert not y[torch.from_numpy(empty).to(DEV)].any()            # written, as zero rows
    f = sm.lift_max(m["points"], sm.LIFT_CIN, W, b, m["order"], m["seg_off"])
    g = sm.lift_max_bwd(dV, m["points"], sm.LIFT_CIN, W, b, m["order"], m["seg_off"])
    assert _rel(y, f["Y"]) < 1e-5
    assert _sum_excess(dw, g["dW"], g["abs_dW"], g["amb_dW"])[0] <= 0
    assert _sum_excess(db, g["db"], g["abs_db"], g["amb_db"])[0] <= 0
    with pytest.raises(ValueError, match="gradient"):
        point_lift_max(_dev(m["points"]).requires_grad_(), _dev(W), _dev(b), m["pvm"])
    with pytest.raises(ValueError):
        point_lift_max(_dev(m["points"]), torch.zeros(8, 9, device=DEV), None, m["pvm"])          # Cin > 8


def test_empty_levels():
    from pcs_amd.pointvoxel import PointVoxelMap
    from pcs_amd.segmax import point_lift_max, voxel_max
    T, C = 5, 16
    none = PointVoxelMap(torch.full((T,), -1, dtype=torch.int32, device=DEV),
                         torch.full((T, 8), -1, dtype=torch.int32, device=DEV), torch.zeros(T, 8, device=DEV), 0)
    lw, lb = (t.requires_grad_() for t in (torch.randn(C, 4, device=DEV), torch.randn(C, device=DEV)))
    v = point_lift_max(torch.randn(T, 4, device=DEV), lw, lb, none)
    assert tuple(v.shape) == (0, C) and v.dtype == BF
    v.sum().backward()
    assert not lw.grad.any() and not lb.grad.any()
    p = torch.randn(T, C, device=DEV).requires_grad_()
    v = voxel_max(p, none)
    assert tuple(v.shape) == (0, C)
    v.sum().backward()
    assert tuple(p.grad.shape) == (T, C) and not p.grad.any()
    V = 7
    nopts = PointVoxelMap(torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, 8, dtype=torch.int32, device=DEV),
                          torch.zeros(0, 8, device=DEV), V)
    v = point_lift_max(torch.zeros(0, 4, device=DEV), lw, lb, nopts, out_dtype=F32)
    assert tuple(v.shape) == (V, C) and not v.any()
    v = voxel_max(torch.zeros(0, C, device=DEV), nopts, out_dtype=F32)
    assert tuple(v.shape) == (V, C) and not v.any()
