"""tests/point_head_refs.py against torch fp64 autograd of the literal composition (F.linear -> relu ->
mean by index_add_;  point_voxel_refs' interpolation -> F.linear -> F.cross_entropy), the reordering
of the head, and the gate condition of the inputs the GPU test runs.  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import point_head_refs as ph
import point_voxel_refs as pv

TOL = 1e-12


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max() if a.size else 0.0
    assert err <= TOL * max(1.0, np.abs(b).max() if b.size else 0.0), (what, err)


_MAPS = {}


def _map(name):
    if name not in _MAPS:
        _MAPS[name] = ph.cpu_map(name)
    return _MAPS[name]


def test_maps_have_the_edges_the_cases_are_for():
    _, own, corner, weight, V = _map("A")
    assert (own >= 0).all() and (corner < 0).any() and np.allclose(weight.sum(1), 1.0)
    _, own, _, _, V = _map("B")
    assert V > 2048 and V % 64 != 0 and V % 32 != 0
    _, own, corner, _, V = _map("C")
    assert (own < 0).any() and (corner < 0).all(axis=1).any()
    assert (np.bincount(own[own >= 0], minlength=V) == 0).any()          # voxels without points
    _, own, _, _, V = _map("D")
    assert np.bincount(own, minlength=V).max() == 40


@pytest.mark.parametrize("i", range(len(ph.LIFT_CASES)), ids=[str(c) for c in ph.LIFT_CASES])
def test_lift_matches_torch_autograd(i):
    name, cin, C, _, bias = ph.LIFT_CASES[i]
    p4, own, _, _, V = _map(name)
    P = ph.lift_points(p4, cin, i)
    W, b = ph.lift_params(i, C, cin, bias)
    dV = ph.rows(i, V, C)
    w = torch.from_numpy(W).double().requires_grad_()
    bt = None if b is None else torch.from_numpy(b).double().requires_grad_()
    h = torch.relu(F.linear(torch.from_numpy(P).double()[:, :cin], w, bt))
    ok = torch.from_numpy(own >= 0)
    o = torch.from_numpy(own.astype(np.int64))[ok]
    cnt = torch.zeros(V, dtype=torch.float64).index_add_(0, o, torch.ones(len(o), dtype=torch.float64))
    y = torch.zeros(V, C, dtype=torch.float64).index_add_(0, o, h[ok]) / cnt.clamp_min(1.0)[:, None]
    (y * torch.from_numpy(dV).double()).sum().backward()
    _close(ph.point_lift_mean(P, W, b, own, V), y.detach().numpy(), "Y")
    _close(ph.point_lift_mean(P, W, b, own, V), pv.voxel_mean(h.detach().numpy(), own, V), "Y vs voxel_mean")
    g = ph.point_lift_mean_grad(dV, P, W, b, own, V)
    _close(g["dW"], w.grad.numpy(), "dW")
    if bias:
        _close(g["db"], bt.grad.numpy(), "db")
    assert (g["abs_dW"] >= np.abs(g["dW"]) - 1e-12).all() and (g["amb_dW"] >= 0).all()


def _torch_interp(x, corner, weight):
    c = torch.from_numpy(corner.astype(np.int64))
    wt = torch.from_numpy(np.where(corner >= 0, weight, 0.0))
    return (x[c.clamp_min(0)] * wt[:, :, None]).sum(1)


@pytest.mark.parametrize("i", range(len(ph.HEAD_CASES)), ids=[str(c) for c in ph.HEAD_CASES])
def test_head_matches_torch_autograd(i):
    name, C, K, _, bias, cw = ph.HEAD_CASES[i]
    _, _, corner, weight, V = _map(name)
    T = len(corner)
    X = ph.rows(i, V, C)
    W, b = ph.head_params(i, C, K, bias)
    y = ph.labels_for(i, T, K)
    cwv = ph.class_weights(i, K) if cw else None
    assert (y == -1).any() and (y >= 0).any()
    x = torch.from_numpy(X).double().requires_grad_()
    w = torch.from_numpy(W).double().requires_grad_()
    bt = None if b is None else torch.from_numpy(b).double().requires_grad_()
    logits = F.linear(_torch_interp(x, corner, weight), w, bt)
    logits.retain_grad()
    loss = F.cross_entropy(logits, torch.from_numpy(y), weight=None if cwv is None else torch.from_numpy(cwv).double(),
                           ignore_index=-1)
    (0.5 * loss).backward()
    r = ph.point_head_loss(X, corner, weight, W, b, y, cwv, upstream=0.5)
    _close(r["logits"], logits.detach().numpy(), "logits")
    _close(ph.point_head(X, corner, weight, W, b), logits.detach().numpy(), "point_head")
    _close(r["loss"], loss.item(), "loss")
    _close(0.5 * r["dlogits"], logits.grad.numpy(), "dlogits")
    assert not r["dlogits"][y < 0].any()
    _close(r["dX"], x.grad.numpy(), "dX")
    _close(r["dW"], w.grad.numpy(), "dW")
    if bias:
        _close(r["db"], bt.grad.numpy(), "db")
    # an arbitrary upstream dlogits through point_head
    dl = ph.rows(100 + i, T, K)
    x.grad, w.grad = None, None
    F.linear(_torch_interp(x, corner, weight), w, bt).backward(torch.from_numpy(dl).double())
    g = ph.point_head_grad(dl, X, corner, weight, W)
    _close(g["dX"], x.grad.numpy(), "point_head dX")
    _close(g["dW"], w.grad.numpy(), "point_head dW")
    _close(g["db"], dl.astype(np.float64).sum(0), "point_head db")


@pytest.mark.parametrize("name", ["A", "C"])
def test_project_then_interpolate_equals_interpolate_then_project(name):
    _, _, corner, weight, V = _map(name)
    X = ph.rows(7, V, 96)
    W, b = ph.head_params(7, 96, 5, True)
    a = ph.head_logits(ph.head_project(X, W), corner, weight, b)["logits"]
    c = pv.devoxelize(X, corner, weight) @ W.astype(np.float64).T + b.astype(np.float64)
    _close(a, c, "logits")
    none = (corner < 0).all(axis=1)
    if none.any():
        assert np.array_equal(a[none], np.broadcast_to(b.astype(np.float64), a[none].shape))   # the bias alone


def test_no_valid_label_gives_nan():
    _, _, corner, weight, V = _map("D")
    r = ph.point_head_loss(ph.rows(1, V, 8), corner, weight, *ph.head_params(1, 8, 3, True),
                           np.full(len(corner), -1, np.int64))
    assert np.isnan(r["loss"]) and not r["dlogits"].any()
    t = F.cross_entropy(torch.zeros(4, 3), torch.full((4,), -1, dtype=torch.int64), ignore_index=-1)
    assert torch.isnan(t)


@pytest.mark.parametrize("i", range(len(ph.LIFT_CASES)), ids=[str(c) for c in ph.LIFT_CASES])
def test_gate_condition_of_the_gpu_inputs(i):
    """The elements whose gate may go either way are at most 1e-4 of all T * C elements, for exactly
    the inputs of tests/test_gpu_point_head.py's lift cases."""
    name, cin, C, _, bias = ph.LIFT_CASES[i]
    p4, _, _, _, _ = _map(name)
    P = ph.lift_points(p4, cin, i)
    W, b = ph.lift_params(i, C, cin, bias)
    T = len(P)
    every = np.arange(T, dtype=np.int32)                       # every point, whatever voxel holds it
    amb = ph.gate_ambiguous(P, cin, W, b, every, np.array([0, T], np.int64))
    share = amb.sum() / (T * C)
    print(f"ambiguous gates: {int(amb.sum())} of {T * C} ({share:.2e})")
    assert share <= 1e-4
