"""pcs_amd.sparse_norm on the device against tests/sparse_norm_refs.py (numpy float64; proved
against torch.nn.functional.batch_norm in tests/test_sparse_norm_refs.py): forward and backward in
every dtype pairing, training and eval, ReLU and residual on and off, the row and channel counts at
which the kernels change path, and a two-level point-voxel network that trains with it.

Bounds.  y and dx: norm-relative max|a - b| / max|b| at test_gpu_point_voxel._bound (1e-5 for an fp32
store, 8e-3 for a bf16 store).  Column sums (dgamma, dbeta, the running buffers): |dev - ref| <=
1e-5 * sum|terms|, the float64 sum of the absolute terms, so cancellation neither hides nor invents
an error.  The backward reference takes the device's own ReLU gate (y_dev > 0); that this gate is the
float64 sign of the pre-activation away from zero is asserted separately.

The V == 2 cases draw x as 2^-8 n instead of 0.3 + 1.5 n: with two rows BatchNorm's
dx is gamma * rstd * (dz_1 - dz_2) / 2 * eps / (var + eps), for var >> eps the residue of a
cancellation between terms 1 / eps * (var + eps) times larger, which no fp32 evaluation resolves
to 1e-5 of the result (its relative error is about 2^-24 * (var + eps) / eps: 1e-2 at var = 1).
At var ~ eps the expression is well conditioned and the bound means what it means elsewhere.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pcs_amd.sparse_norm  # noqa: F401  (fails here without the layer)
import sparse_norm_refs as sn
from test_gpu_point_voxel import _bound, _clouds, _level, _map, _rb

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BF, F32 = torch.bfloat16, torch.float32
SUM_BOUND = 1e-5
MOMENTUM, EPS = 0.1, 1e-5


def _bf16_exact(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(BF).to(F32).numpy().astype(np.float64)


_INPUTS = {}


def _inputs(V, C):
    """Seeded, bf16-exact float64 inputs of one shape, made once and never changed."""
    if (V, C) not in _INPUTS:
        rng = np.random.default_rng(100003 * V + C)
        centre, spread = (0.0, 2.0 ** -8) if V == 2 else (0.3, 1.5)          # see the module docstring
        d = {"x": _bf16_exact(centre + spread * rng.standard_normal((V, C))),
             "res": _bf16_exact(rng.standard_normal((V, C))),
             "dy": _bf16_exact(rng.standard_normal((V, C))),
             "gamma": rng.uniform(0.5, 1.5, C).astype(np.float32).astype(np.float64),
             "beta": (0.2 * rng.standard_normal(C)).astype(np.float32).astype(np.float64),
             "rm": (0.1 * rng.standard_normal(C)).astype(np.float32).astype(np.float64),
             "rv": rng.uniform(0.5, 2.0, C).astype(np.float32).astype(np.float64)}
        for a in d.values():
            a.setflags(write=False)
        _INPUTS[(V, C)] = d
    return _INPUTS[(V, C)]


def _dev(a, dtype=F32, grad=False):
    return torch.from_numpy(np.array(a)).to(DEV, dtype).requires_grad_(grad)   # a copy: the inputs are read-only


def _run(d, xdt, ydt, training, relu, with_res, momentum=MOMENTUM, grads=(True, True, True, True)):
    """One forward and backward on the device: a dict of CPU float64 arrays."""
    from pcs_amd.sparse_norm import sparse_batch_norm
    x, g, b = _dev(d["x"], xdt, grads[0]), _dev(d["gamma"], F32, grads[1]), _dev(d["beta"], F32, grads[2])
    r = _dev(d["res"], ydt, grads[3]) if with_res else None
    rm, rv = _dev(d["rm"]), _dev(d["rv"])
    y = sparse_batch_norm(x, g, b, rm, rv, training, momentum, EPS, relu, r, ydt)
    assert y.dtype == ydt and y.shape == x.shape
    out = {"y": y.detach()}
    if y.requires_grad:
        y.backward(_dev(d["dy"], ydt))
        for k, t in (("dx", x), ("dgamma", g), ("dbeta", b), ("dres", r)):
            if t is not None and t.grad is not None:
                assert t.grad.dtype == t.dtype and t.grad.shape == t.shape
                out[k] = t.grad
    out["rm"], out["rv"] = rm, rv
    torch.cuda.synchronize()
    return {k: v.double().cpu().numpy() for k, v in out.items()}


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _sum_err(a, b, terms):
    """max over the columns of |dev - ref| / sum|terms| (0 / 0 counts as 0)."""
    return float(np.max(np.abs(a - b) / np.maximum(terms, 1e-300)))


def _check(out, d, xdt, ydt, training, relu, with_res, tag):
    res = d["res"] if with_res else None
    f = sn.forward(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], training, MOMENTUM, EPS, relu, res)
    V = d["x"].shape[0]
    figs = {"y": _rel(out["y"], f["y"])}
    gate = None
    if relu:
        # the device's gate is the float64 sign of pre outside a margin that almost no element is in
        gate = out["y"] > 0
        margin = np.abs(f["pre"]) <= 1e-5 * np.abs(f["pre"]).max()
        assert np.array_equal(gate[~margin], (f["pre"] > 0)[~margin]), tag
        assert margin.mean() <= 0.01, (tag, margin.mean())
    dx, dgamma, dbeta, dz, (t1, t2) = sn.backward(d["dy"], gate, d["x"], d["gamma"], f["mean"], f["rstd"], training)
    figs["dx"] = _rel(out["dx"], dx)
    figs["dgamma"] = _sum_err(out["dgamma"], dgamma, t2)
    figs["dbeta"] = _sum_err(out["dbeta"], dbeta, t1)
    if training:
        ax = np.abs(d["x"]).sum(0) / V
        sq = ((d["x"] - f["mean"]) ** 2).sum(0) / (V - 1)
        figs["running_mean"] = _sum_err(out["rm"], f["running_mean"], (1 - MOMENTUM) * np.abs(d["rm"]) + MOMENTUM * ax)
        figs["running_var"] = _sum_err(out["rv"], f["running_var"], (1 - MOMENTUM) * d["rv"] + MOMENTUM * sq)
    print(tag, " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    if with_res:
        assert np.array_equal(out["dres"], dz), tag          # dz is exact in dy's dtype
    if not training:
        assert np.array_equal(out["rm"], d["rm"]) and np.array_equal(out["rv"], d["rv"]), tag
    assert figs.pop("y") <= _bound(ydt), tag
    assert figs.pop("dx") <= _bound(xdt), tag
    for k, v in figs.items():
        assert v <= SUM_BOUND, (tag, k, v)


ROWS = (2, 65, 257, 3000)    # below one row pass / one block and a one-row tail / many blocks, ragged tail
CASES = ([(V, 64, xdt, ydt, True, True) for V in ROWS for xdt in (BF, F32) for ydt in (BF, F32)]
         + [(V, C, BF, BF, True, True) for C in (8, 96, 256, 1024) for V in ROWS]
         + [(V, 4, F32, F32, True, True) for V in ROWS]
         + [(257, 64, BF, BF, relu, res) for relu, res in ((False, False), (True, False), (False, True))]
         + [(65, 96, F32, BF, False, False), (65, 96, BF, F32, True, False)])


def _id(case):
    V, C, xdt, ydt, relu, res = case
    n = {BF: "bf16", F32: "f32"}
    return f"V{V}-C{C}-{n[xdt]}-{n[ydt]}" + ("-relu" if relu else "") + ("-res" if res else "")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_training_matches_fp64(case):
    V, C, xdt, ydt, relu, with_res = case
    d = _inputs(V, C)
    _check(_run(d, xdt, ydt, True, relu, with_res), d, xdt, ydt, True, relu, with_res, "train " + _id(case))


@pytest.mark.parametrize("case", [(257, 64, BF, BF, True, True), (3000, 96, F32, F32, True, True),
                                  (65, 64, F32, BF, False, False), (1, 64, BF, BF, True, True),
                                  (1, 4, F32, F32, False, True)], ids=_id)
def test_eval_matches_fp64(case):
    """Eval mode, forward and backward (V == 1 included): the running buffers normalise and stay as
    they are; the output is F.batch_norm(training=False) in float64."""
    V, C, xdt, ydt, relu, with_res = case
    d = _inputs(V, C)
    out = _run(d, xdt, ydt, False, relu, with_res)
    _check(out, d, xdt, ydt, False, relu, with_res, "eval " + _id(case))
    t = F.batch_norm(torch.tensor(d["x"]), torch.tensor(d["rm"]), torch.tensor(d["rv"]), torch.tensor(d["gamma"]),
                     torch.tensor(d["beta"]), False, MOMENTUM, EPS)
    t = t + torch.tensor(d["res"]) if with_res else t
    t = torch.relu(t) if relu else t
    assert _rel(out["y"], t.numpy()) <= _bound(ydt)


def test_shifted_mean_variance():
    """x = 100 + 0.01 n in fp32: a sum-of-squares variance is wrong by order 1 here, Welford by about
    (delta / sigma)^2 ~ 4e-7 plus rounding.  momentum = 1 makes running_var the batch's unbiased
    variance."""
    V, C = 3000, 64
    rng = np.random.default_rng(7)
    x = (100.0 + 0.01 * rng.standard_normal((V, C))).astype(np.float32).astype(np.float64)
    d = dict(_inputs(V, C), x=x)
    out = _run(d, F32, F32, True, False, False, momentum=1.0)
    var = x.var(0, ddof=1)
    err = float(np.max(np.abs(out["rv"] - var) / var))
    err_mean = _sum_err(out["rm"], x.mean(0), np.abs(x).sum(0) / V)
    print(f"shifted mean: batch variance rel err {err:.2e}, mean err / mean|x| {err_mean:.2e}")
    assert err <= 1e-3
    assert err_mean <= SUM_BOUND


def test_edge_row_counts_and_bad_arguments():
    from pcs_amd.sparse_norm import SparseBatchNorm, sparse_batch_norm
    C = 64
    g, b, rm, rv = (torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV),
                    torch.ones(C, device=DEV))
    x0 = torch.zeros(0, C, device=DEV, dtype=BF, requires_grad=True)
    y0 = sparse_batch_norm(x0, g, b, rm, rv, False, relu=True, out_dtype=F32)      # V == 0 in eval: empty
    assert y0.shape == (0, C) and y0.dtype == F32
    y0.sum().backward()
    assert x0.grad.shape == (0, C)
    for V in (0, 1):                                                               # training needs two rows
        with pytest.raises(ValueError):
            sparse_batch_norm(torch.zeros(V, C, device=DEV, dtype=BF), g, b, rm, rv, True)
    for C_bad, dt, odt in ((12, BF, BF), (60, BF, BF), (12, F32, BF), (12, BF, F32), (6, F32, F32), (1032, BF, BF),
                           (1028, F32, F32)):
        p = [torch.ones(C_bad, device=DEV) for _ in range(4)]
        with pytest.raises(ValueError):
            sparse_batch_norm(torch.zeros(8, C_bad, device=DEV, dtype=dt), *p, True, out_dtype=odt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sparse_batch_norm(torch.zeros(8, C), g.cpu(), b.cpu(), rm.cpu(), rv.cpu(), True)
    with pytest.raises(ValueError):
        sparse_batch_norm(torch.zeros(8, C, device=DEV, dtype=torch.float16), g, b, rm, rv, True)
    with pytest.raises(ValueError):                                                # residual in out_dtype
        sparse_batch_norm(torch.zeros(8, C, device=DEV, dtype=BF), g, b, rm, rv, True,
                          residual=torch.zeros(8, C, device=DEV), out_dtype=BF)
    for kw in ({"affine": False}, {"track_running_stats": False}, {"momentum": None}):
        with pytest.raises(ValueError):
            SparseBatchNorm(C, **kw)


def test_state_dict_interchange_with_batchnorm1d():
    from pcs_amd.sparse_norm import SparseBatchNorm
    C = 64
    torch.manual_seed(3)
    ref = torch.nn.BatchNorm1d(C)
    with torch.no_grad():
        ref.weight.uniform_(0.5, 1.5), ref.bias.normal_(), ref.running_mean.normal_(), ref.running_var.uniform_(0.5, 2)
        ref.num_batches_tracked.fill_(5)
    m = SparseBatchNorm(C, relu=True)
    assert list(m.state_dict()) == list(ref.state_dict())
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV)
    x = _dev(_inputs(257, C)["x"], BF)
    m(x), m(x)
    assert int(m.num_batches_tracked) == 7 and m.num_batches_tracked.device.type == "cuda"
    m.eval()
    m(x)
    assert int(m.num_batches_tracked) == 7
    back = torch.nn.BatchNorm1d(C)
    back.load_state_dict(m.state_dict())
    for k, v in m.state_dict().items():
        assert torch.equal(back.state_dict()[k], v.cpu()), k
    # the same eval-mode function as the BatchNorm1d that holds the same state
    want = torch.relu(back.double().eval()(x.double().cpu()))
    assert _rel(m(x).detach().double().cpu().numpy(), want.detach().numpy()) <= _bound(BF)


def test_nan_stays_in_its_column():
    V, C = 257, 64
    d = _inputs(V, C)
    clean = _run(d, F32, F32, True, True, True)
    x = d["x"].copy()
    x[100, 5] = np.nan
    dirty = _run(dict(d, x=x), F32, F32, True, True, True)
    assert np.isnan(dirty["y"][:, 5]).all()
    keep = np.arange(C) != 5
    for k in ("y", "dx", "dres"):
        assert np.array_equal(dirty[k][:, keep], clean[k][:, keep]), k
    for k in ("dgamma", "dbeta", "rm", "rv"):
        assert np.array_equal(dirty[k][keep], clean[k][keep]), k
    assert np.isnan(dirty["rm"][5])


@pytest.mark.parametrize("xdt,ydt", [(BF, BF), (F32, BF)])
def test_two_runs_are_bitwise_equal(xdt, ydt):
    d = _inputs(3000, 96)
    a, b = _run(d, xdt, ydt, True, True, True), _run(d, xdt, ydt, True, True, True)
    assert sorted(a) == ["dbeta", "dgamma", "dres", "dx", "rm", "rv", "y"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_needs_input_grad_paths():
    V, C = 257, 64
    d = _inputs(V, C)
    full = _run(d, BF, BF, True, True, True)
    frozen_x = _run(d, BF, BF, True, True, True, grads=(False, True, True, False))
    assert "dx" not in frozen_x and "dres" not in frozen_x
    assert np.array_equal(frozen_x["dgamma"], full["dgamma"]) and np.array_equal(frozen_x["dbeta"], full["dbeta"])
    frozen_p = _run(d, BF, BF, True, True, True, grads=(True, False, False, True))
    assert "dgamma" not in frozen_p and "dbeta" not in frozen_p
    assert np.array_equal(frozen_p["dx"], full["dx"]) and np.array_equal(frozen_p["dres"], full["dres"])
    only_res = _run(d, BF, BF, True, False, True, grads=(False, False, False, True))
    assert np.array_equal(only_res["dres"], d["dy"])           # no gate: the residual's gradient is dy
    none = _run(d, BF, BF, True, True, True, grads=(False, False, False, False))
    assert np.array_equal(none["y"], full["y"])


def test_point_voxel_network_with_batchnorm_trains():
    """voxel_mean -> SparseResBlock -> down + BN+ReLU -> SparseResBlock -> up + BN+ReLU + skip ->
    devoxelize -> a per-point cross-entropy: finite gradients on every parameter, a falling loss,
    running statistics that moved, and a repeatable eval forward."""
    from pcs_amd.pointvoxel import devoxelize, voxel_mean
    from pcs_amd.sparse import SparseDownConv3d, SparseUpConv3d, coarsen
    from pcs_amd.sparse_norm import SparseBatchNorm, SparseResBlock
    torch.manual_seed(0)
    rb, _, _ = _rb(_clouds(21, 2, 16, 0.3))
    _, sv = _level(rb, 16)
    svc, link = coarsen(sv)
    pvm = _map(rb, sv)
    net = torch.nn.ModuleDict({
        "lift": torch.nn.Linear(4, 64), "enc": SparseResBlock(64),
        "down": SparseDownConv3d(64, 64), "bn_down": SparseBatchNorm(64, relu=True), "mid": SparseResBlock(64),
        "up": SparseUpConv3d(64, 64), "bn_up": SparseBatchNorm(64, relu=True), "head": torch.nn.Linear(64, 2)}).to(DEV)
    params = list(net.parameters())
    opt = torch.optim.SGD(params, lr=0.05)
    raw, labels = rb.points.to(DEV).float(), rb.labels.to(DEV)

    def forward():
        e = net["enc"](voxel_mean(torch.relu(net["lift"](raw)), pvm), sv)
        c = net["mid"](net["bn_down"](net["down"](e, link)), svc)
        u = net["bn_up"](net["up"](c, link)) + e
        return net["head"](devoxelize(u, pvm))

    bns = [m for m in net.modules() if isinstance(m, SparseBatchNorm)]
    assert len(bns) == 6
    losses = []
    for _ in range(8):
        loss = F.cross_entropy(forward(), labels, ignore_index=-1)
        opt.zero_grad()
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
        opt.step()
        losses.append(loss.item())
    print("losses", [round(v, 4) for v in losses])
    assert losses[-1] < losses[0]
    for m in bns:
        assert int(m.num_batches_tracked) == 8
        assert m.running_mean.abs().max() > 0 and (m.running_var - 1).abs().max() > 0
        assert torch.isfinite(m.running_mean).all() and torch.isfinite(m.running_var).all()
    net.eval()
    state = [m.running_var.clone() for m in bns]
    with torch.no_grad():
        a, b = forward(), forward()
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert all(torch.equal(s, m.running_var) for s, m in zip(state, bns))
