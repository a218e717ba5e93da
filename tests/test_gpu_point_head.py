"""The fused point lift and point head on MI355X (pcs_amd.pointhead; csrc/pointhead.hip) against the
fp64 statement tests/point_head_refs.py on the device's own maps: the five entry points directly, the
three Python functions forward and backward, determinism, the ignored labels, the composition
fallback and the empty levels.  Build-defined: the reference has no voxel grid.

Bounds (tests/test_gpu_point_voxel.py, tests/test_gpu_sparse_norm.py): fp32 outputs 1e-5 and bf16
stores 8e-3, max error over max |reference|; sums (loss, dW, db) 1e-5 of the fp64 sum of the absolute
values of their terms, for the lift's dW and db plus the sum of |term| over the elements whose gate
may go either way (point_head_refs.GATE_BAND; tests/test_point_head_refs.py bounds their share)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import point_head_refs as ph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BF, F32 = torch.bfloat16, torch.float32
SUM_TOL = 1e-5


def _rb(clouds):
    from pcs_amd.data import ragged_collate
    return ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in clouds])


_CASES = {}


def _case(name):
    """The device's map of a case and its arrays as numpy, built once, never changed."""
    if name not in _CASES:
        from pcs_amd.pointvoxel import point_voxel_map
        from pcs_amd.sparse import sparse_voxels
        from pcs_amd.voxel import voxelize
        grid, level, query = ph.case_clouds(name)
        rb = _rb(level)
        sv = sparse_voxels(rb, voxelize(rb, grid, ph.LO, ph.HI), ph.LO, ph.HI)
        pvm = point_voxel_map(_rb(query), sv, ph.LO, ph.HI)
        order, seg_off, _, inv, _ = pvm.points_by_voxel()
        point, pw, pair_off = pvm.pairs_by_voxel()
        np_ = lambda t: t.cpu().numpy()   # noqa: E731
        _CASES[name] = SimpleNamespace(
            pvm=pvm, points4=ph.flat(query)[0], T=pvm.num_points, V=pvm.num_voxels, own=np_(pvm.own), corner=np_(pvm.corner),
            weight=np_(pvm.weight).astype(np.float64), order=np_(order), seg_off=np_(seg_off), inv=np_(inv).astype(np.float64),
            pair_point=np_(point), pair_weight=np_(pw).astype(np.float64), pair_off=np_(pair_off))
    return _CASES[name]


def _dev(a, dtype=F32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _rel(got, ref):
    ref = np.asarray(ref, np.float64)
    got = got.detach().double().cpu().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)) if ref.size else 0.0


def _sum_excess(got, ref, abs_sum, extra=0.0):
    """max of |got - ref| - (SUM_TOL * abs_sum + extra): <= 0 passes; also the plain error for the log."""
    got = got.detach().double().cpu().numpy()
    ref, abs_sum = np.asarray(ref, np.float64), np.asarray(abs_sum, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref)
    return float((err - (SUM_TOL * abs_sum + extra)).max()), float((err / np.maximum(abs_sum, 1e-300)).max())


def _store_bound(dtype):
    return 1e-5 if dtype == F32 else 8e-3


def test_cases_have_their_edges():
    a, b, c, d = (_case(n) for n in "ABCD")
    assert (a.own >= 0).all() and (a.corner < 0).any()
    assert b.V > 2048 and b.V % 64 != 0
    assert (c.own < 0).any() and (c.corner < 0).all(axis=1).any() and (np.diff(c.seg_off) == 0).any()
    assert np.diff(d.seg_off).max() == 40


# ---- the lift
def _run_lift(m, P, W, b, dV, out_dtype):
    from pcs_amd.pointhead import point_lift_mean
    w = _dev(W).requires_grad_()
    bt = None if b is None else _dev(b).requires_grad_()
    y = point_lift_mean(_dev(P), w, bt, m.pvm, out_dtype=out_dtype)
    y.backward(_dev(dV, out_dtype))
    torch.cuda.synchronize()
    return y.detach(), w.grad, None if bt is None else bt.grad


@pytest.mark.parametrize("i", range(len(ph.LIFT_CASES)), ids=[str(c) for c in ph.LIFT_CASES])
def test_lift_matches_fp64(i):
    name, cin, C, bf, bias = ph.LIFT_CASES[i]
    m = _case(name)
    P = ph.lift_points(m.points4, cin, i)
    W, b = ph.lift_params(i, C, cin, bias)
    dV = ph.rows(i, m.V, C)
    out_dtype = BF if bf else F32
    y, dw, db = _run_lift(m, P, W, b, dV, out_dtype)
    y2, dw2, db2 = _run_lift(m, P, W, b, dV, out_dtype)
    assert y.dtype == out_dtype and tuple(y.shape) == (m.V, C) and tuple(dw.shape) == (C, cin)
    assert torch.equal(y, y2) and torch.equal(dw, dw2) and (db is None or torch.equal(db, db2))
    e = _rel(y, ph.lift_mean(P, cin, W, b, m.order, m.seg_off, m.inv))
    g = ph.lift_mean_bwd(dV, P, cin, W, b, m.order, m.seg_off, m.inv)
    xw, ew = _sum_excess(dw, g["dW"], g["abs_dW"], g["amb_dW"])
    print(f"Y rel err {e:.3e}; dW err / sum|term| {ew:.3e}; ambiguous |term| max {g['amb_dW'].max():.3e}")
    assert e < _store_bound(out_dtype)
    assert xw <= 0
    if bias:
        xb, eb = _sum_excess(db, g["db"], g["abs_db"], g["amb_db"])
        print(f"db err / sum|term| {eb:.3e}")
        assert xb <= 0
    empty = torch.from_numpy(np.diff(m.seg_off) == 0).to(DEV)
    if empty.any():
        assert y[empty].abs().max() == 0                         # written, as zero rows


def test_lift_rejects_bad_inputs():
    from pcs_amd.pointhead import point_lift_mean
    m = _case("D")
    W, b = ph.lift_params(0, 8, 4, True)
    with pytest.raises(ValueError, match="gradient"):
        point_lift_mean(_dev(m.points4).requires_grad_(), _dev(W), _dev(b), m.pvm)
    with pytest.raises(RuntimeError, match="HIP device only"):
        point_lift_mean(torch.from_numpy(m.points4), torch.from_numpy(W), None, m.pvm)
    with pytest.raises(ValueError):
        point_lift_mean(_dev(m.points4), torch.zeros(8, 9, device=DEV), None, m.pvm)          # Cin > 8
    with pytest.raises(ValueError):
        point_lift_mean(_dev(m.points4)[:-1], _dev(W), None, m.pvm)


# ---- the entry points of the head, directly
@pytest.mark.parametrize("i", [0, 6, 8], ids=lambda i: str(ph.HEAD_CASES[i]))
def test_head_entry_points_match_fp64(i):
    import pcs_amd._lib as L
    name, C, K, bf, bias, cw = ph.HEAD_CASES[i]
    m = _case(name)
    X = ph.rows(i, m.V, C)
    W, b = ph.head_params(i, C, K, bias)
    y = ph.labels_for(i, m.T, K)
    cwv = ph.class_weights(i, K) if cw else np.ones(K, np.float32)
    x, w, bt, lab, cwt = _dev(X, BF if bf else F32), _dev(W), _dev(b), torch.from_numpy(y).to(DEV), _dev(cwv)
    code, s = (L.BF16 if bf else L.F32), L.stream_ptr(DEV)
    z = torch.empty(m.V, K, device=DEV)
    L.call("pcs_point_head_project", L.ptr(x), code, m.V, C, L.ptr(w), K, L.ptr(z), s)
    nbytes = L.workspace("pcs_point_head_workspace", m.T, m.V, C, K)
    ws = torch.empty(nbytes // 4, device=DEV)
    counts, wsum = torch.empty(K, dtype=torch.int64, device=DEV), torch.empty(4, device=DEV)
    L.call("pcs_ce_weight_sum", L.ptr(lab), m.T, L.ptr(cwt), K, L.ptr(counts), L.ptr(wsum), s)
    logits, dl = torch.empty(m.T, K, device=DEV), torch.full((m.T, K), 7.0, device=DEV)
    loss, db = torch.empty(1, device=DEV), torch.empty(K, device=DEV)
    L.call("pcs_point_head_logits", L.ptr(z), L.ptr(m.pvm.corner), L.ptr(m.pvm.weight), m.T, K, L.ptr(bt), L.ptr(lab),
           L.ptr(cwt), wsum[2:].data_ptr(), L.ptr(logits), L.ptr(dl), L.ptr(ws), nbytes, L.ptr(loss), L.ptr(db), s)
    only = torch.empty(m.T, K, device=DEV)
    L.call("pcs_point_head_logits", L.ptr(z), L.ptr(m.pvm.corner), L.ptr(m.pvm.weight), m.T, K, L.ptr(bt), None, None, None,
           L.ptr(only), None, None, 0, None, None, s)
    r = ph.head_logits(ph.head_project(X, W), m.corner, m.weight, b, y, cwv)
    ez, el, ed = _rel(z, ph.head_project(X, W)), _rel(logits, r["logits"]), _rel(dl, r["dlogits"])
    xl, e_loss = _sum_excess(loss[0], r["loss"], r["abs_loss"])
    xb, e_db = _sum_excess(db, r["db"], r["abs_db"])
    print(f"Z {ez:.3e}, logits {el:.3e}, dlogits {ed:.3e}, loss {e_loss:.3e}, db {e_db:.3e}")
    assert ez < 1e-5 and el < 1e-5 and ed < 1e-5 and xl <= 0 and xb <= 0
    assert torch.equal(only, logits)
    ignored = torch.from_numpy(y < 0).to(DEV)
    assert ignored.any() and dl[ignored].abs().max() == 0          # exactly zero rows
    none = torch.from_numpy((m.corner < 0).all(axis=1)).to(DEV)
    if none.any():                                                 # no occupied corner: the bias alone
        assert torch.equal(logits[none], (bt if bias else torch.zeros(K, device=DEV)).expand(int(none.sum()), K))
    # the backward from the device's dlogits, against the statement on the same dlogits
    dx, dw = torch.empty_like(x), torch.empty(K, C, device=DEV)
    gs = torch.tensor([0.5], device=DEV)
    L.call("pcs_point_head_bwd", L.ptr(dl), L.ptr(m.pvm.pairs_by_voxel()[0]), L.ptr(m.pvm.pairs_by_voxel()[1]),
           L.ptr(m.pvm.pairs_by_voxel()[2]), L.ptr(x), code, m.V, C, L.ptr(w), K, L.ptr(gs), L.ptr(dx), L.ptr(ws), nbytes,
           L.ptr(dw), s)
    g = ph.head_bwd(dl.double().cpu().numpy(), m.pair_point, m.pair_weight, m.pair_off, X, W, g=0.5)
    ex = _rel(dx, g["dX"])
    xw, ew = _sum_excess(dw, g["dW"], g["abs_dW"])
    print(f"dX {ex:.3e}, dW {ew:.3e}")
    assert ex < _store_bound(x.dtype) and xw <= 0
    touched = np.diff(m.pair_off) > 0
    if (~touched).any():                                           # voxels no point touches: zero rows
        assert dx[torch.from_numpy(~touched).to(DEV)].abs().max() == 0


# ---- the Python functions
def _run_head(m, X, W, b, dl, xdtype):
    from pcs_amd.pointhead import point_head
    x, w = _dev(X, xdtype).requires_grad_(), _dev(W).requires_grad_()
    bt = None if b is None else _dev(b).requires_grad_()
    logits = point_head(x, m.pvm, w, bt)
    logits.backward(_dev(dl))
    torch.cuda.synchronize()
    return logits.detach(), x.grad, w.grad, None if bt is None else bt.grad


def _run_loss(m, X, W, b, y, cwv, xdtype, upstream):
    from pcs_amd.pointhead import point_head_loss
    x, w = _dev(X, xdtype).requires_grad_(), _dev(W).requires_grad_()
    bt = None if b is None else _dev(b).requires_grad_()
    loss, logits = point_head_loss(x, m.pvm, w, bt, torch.from_numpy(y).to(DEV), _dev(cwv), return_logits=True)
    (loss * upstream).backward()
    torch.cuda.synchronize()
    return loss.detach(), logits, x.grad, w.grad, None if bt is None else bt.grad


def _same(a, b):
    return all((s is None and t is None) or torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("i", range(len(ph.HEAD_CASES)), ids=[str(c) for c in ph.HEAD_CASES])
def test_head_matches_fp64(i):
    from pcs_amd.pointhead import point_head, point_head_loss
    name, C, K, bf, bias, cw = ph.HEAD_CASES[i]
    m = _case(name)
    xdtype = BF if bf else F32
    X = ph.rows(i, m.V, C)
    W, b = ph.head_params(i, C, K, bias)
    y = ph.labels_for(i, m.T, K)
    cwv = ph.class_weights(i, K) if cw else None
    dl = ph.rows(100 + i, m.T, K)
    # point_head with an arbitrary upstream gradient
    out = _run_head(m, X, W, b, dl, xdtype)
    assert _same(out, _run_head(m, X, W, b, dl, xdtype))
    logits, dx, dw, db = out
    assert logits.dtype == F32 and tuple(logits.shape) == (m.T, K) and dx.dtype == xdtype and tuple(dx.shape) == (m.V, C)
    g = ph.head_bwd(dl, m.pair_point, m.pair_weight, m.pair_off, X, W)
    el, ex = _rel(logits, ph.point_head(X, m.corner, m.weight, W, b)), _rel(dx, g["dX"])
    xw, ew = _sum_excess(dw, g["dW"], g["abs_dW"])
    print(f"point_head: logits {el:.3e}, dX {ex:.3e}, dW {ew:.3e}")
    assert el < 1e-5 and ex < _store_bound(xdtype) and xw <= 0
    if bias:
        xb, eb = _sum_excess(db, dl.astype(np.float64).sum(0), np.abs(dl.astype(np.float64)).sum(0))
        print(f"point_head: db {eb:.3e}")
        assert xb <= 0
    # point_head_loss with an upstream gradient of 0.5
    out = _run_loss(m, X, W, b, y, cwv, xdtype, 0.5)
    assert _same(out, _run_loss(m, X, W, b, y, cwv, xdtype, 0.5))
    loss, lg, dx, dw, db = out
    assert loss.dim() == 0 and loss.dtype == F32 and not lg.requires_grad and torch.equal(lg, logits)
    r = ph.point_head_loss(X, m.corner, m.weight, W, b, y, cwv, upstream=0.5)
    xl, e_loss = _sum_excess(loss, r["loss"], r["abs_loss"])
    ex = _rel(dx, r["dX"])
    xw, ew = _sum_excess(dw, r["dW"], r["abs_dW"])
    print(f"point_head_loss: loss {e_loss:.3e}, dX {ex:.3e}, dW {ew:.3e}")
    assert xl <= 0 and ex < _store_bound(xdtype) and xw <= 0
    if bias:
        xb, eb = _sum_excess(db, r["db"], r["abs_db"])
        print(f"point_head_loss: db {eb:.3e}")
        assert xb <= 0
    # the same loss from torch's cross-entropy on the fused logits
    with torch.no_grad():
        x, w, bt = _dev(X, xdtype), _dev(W), _dev(b)
        t = F.cross_entropy(point_head(x, m.pvm, w, bt), torch.from_numpy(y).to(DEV), weight=_dev(cwv), ignore_index=-1)
        assert torch.equal(point_head_loss(x, m.pvm, w, bt, torch.from_numpy(y).to(DEV), _dev(cwv)), loss)   # no graph needed
    print(f"loss {loss.item():.7f}, torch on the same logits {t.item():.7f}")
    assert abs(loss.item() - t.item()) <= 1e-6 * abs(t.item())


def test_head_falls_back_above_16_classes():
    from pcs_amd.pointhead import point_head, point_head_loss
    from pcs_amd.pointvoxel import devoxelize
    m, C, K = _case("A"), 64, 17
    X = ph.rows(50, m.V, C)
    W, b = ph.head_params(50, C, K, True)
    y, cwv = torch.from_numpy(ph.labels_for(50, m.T, K)).to(DEV), _dev(ph.class_weights(50, K))
    got, want = [], []
    for fn, res in ((lambda x, w, bt: point_head_loss(x, m.pvm, w, bt, y, cwv, return_logits=True), got),
                    (lambda x, w, bt: (lambda lg: (F.cross_entropy(lg, y, weight=cwv, ignore_index=-1), lg.detach()))(
                        F.linear(devoxelize(x, m.pvm), w, bt)), want)):
        x, w, bt = _dev(X, BF).requires_grad_(), _dev(W).requires_grad_(), _dev(b).requires_grad_()
        loss, lg = fn(x, w, bt)
        loss.backward()
        res.extend([loss.detach(), lg, x.grad, w.grad, bt.grad])
    assert _same(got, want)
    assert torch.equal(point_head(_dev(X, BF), m.pvm, _dev(W), _dev(b)), got[1])
    r = ph.point_head_loss(X, m.corner, m.weight, W, b, y.cpu().numpy(), cwv.cpu().numpy())
    assert _rel(got[1], r["logits"]) < 1e-5 and _sum_excess(got[0], r["loss"], r["abs_loss"])[0] <= 0


def test_every_label_ignored_gives_nan():
    from pcs_amd.pointhead import point_head_loss
    m = _case("A")
    W, b = ph.head_params(3, 64, 5, True)
    x, w, bt = _dev(ph.rows(3, m.V, 64), BF).requires_grad_(), _dev(W).requires_grad_(), _dev(b).requires_grad_()
    for fill in (-1, 5, -7, 1 << 40):                              # none is a class: nothing is read through it
        loss = point_head_loss(x, m.pvm, w, bt, torch.full((m.T,), fill, dtype=torch.int64, device=DEV))
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isnan(loss)


def test_head_rejects_bad_inputs():
    from pcs_amd.pointhead import point_head, point_head_loss
    m = _case("D")
    x, w = torch.zeros(m.V, 8, device=DEV), torch.zeros(2, 8, device=DEV)
    with pytest.raises(RuntimeError, match="HIP device only"):
        point_head(x.cpu(), m.pvm, w.cpu())
    with pytest.raises(ValueError):
        point_head(x, m.pvm, torch.zeros(2, 16, device=DEV))
    with pytest.raises(ValueError):
        point_head(x[:-1], m.pvm, w)
    with pytest.raises(ValueError):
        point_head_loss(x, m.pvm, w, None, torch.zeros(m.T + 1, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        point_head_loss(x, m.pvm, w, None, torch.zeros(m.T, dtype=torch.int64, device=DEV), torch.ones(3, device=DEV))


def test_empty_levels():
    """No voxel: zero rows, logits equal to the bias, zero gradients of the weights; no point: zero
    voxel rows and empty logits."""
    from pcs_amd.pointhead import point_head, point_head_loss, point_lift_mean
    from pcs_amd.pointvoxel import PointVoxelMap
    T, C, K = 5, 16, 3
    none = PointVoxelMap(torch.full((T,), -1, dtype=torch.int32, device=DEV),
                         torch.full((T, 8), -1, dtype=torch.int32, device=DEV), torch.zeros(T, 8, device=DEV), 0)
    lw, lb = (t.requires_grad_() for t in (torch.randn(C, 4, device=DEV), torch.randn(C, device=DEV)))
    v = point_lift_mean(torch.randn(T, 4, device=DEV), lw, lb, none)
    assert tuple(v.shape) == (0, C) and v.dtype == BF
    v.sum().backward()
    assert not lw.grad.any() and not lb.grad.any()
    x = torch.zeros(0, C, device=DEV, dtype=BF).requires_grad_()
    w, b = torch.randn(K, C, device=DEV).requires_grad_(), torch.randn(K, device=DEV).requires_grad_()
    logits = point_head(x, none, w, b)
    assert torch.equal(logits, b.detach().expand(T, K))
    y = torch.tensor([0, 2, -1, 1, 1], device=DEV)
    loss = point_head_loss(x, none, w, b, y)
    loss.backward()
    want = F.cross_entropy(b.detach().expand(T, K), y, ignore_index=-1)
    assert abs(loss.item() - want.item()) <= 1e-6 * abs(want.item())
    assert tuple(x.grad.shape) == (0, C) and not w.grad.any() and b.grad.abs().max() > 0
    V = 7
    nopts = PointVoxelMap(torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, 8, dtype=torch.int32, device=DEV),
                          torch.zeros(0, 8, device=DEV), V)
    v = point_lift_mean(torch.zeros(0, 4, device=DEV), lw, lb, nopts, out_dtype=F32)
    assert tuple(v.shape) == (V, C) and not v.any()
    x = torch.randn(V, C, device=DEV).requires_grad_()
    logits = point_head(x, nopts, w, b)
    assert tuple(logits.shape) == (0, K)
    logits.sum().backward()
    assert not x.grad.any()
    assert torch.isnan(point_head_loss(x, nopts, w, b, torch.zeros(0, dtype=torch.int64, device=DEV)))
