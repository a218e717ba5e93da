"""tests/sparse_norm_refs.py (the float64 statement of pcs_amd.sparse_norm) against
torch.nn.functional.batch_norm in float64 with autograd: outputs, all four gradients and both
running buffers after one step.  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pcs_amd.sparse_norm  # noqa: F401  (the layer the statement describes: no layer, no test)
import sparse_norm_refs as sn

TOL = 1e-12


def _close(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    err = np.abs(a - b).max() if a.size else 0.0
    assert err <= TOL * max(1.0, np.abs(b).max() if b.size else 0.0), (what, err)


@pytest.mark.parametrize("V", [2, 257])
@pytest.mark.parametrize("C", [4, 96])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_statement_matches_torch_float64(V, C, training, relu, with_res):
    rng = np.random.default_rng(1000 * V + 10 * C + 4 * training + 2 * relu + with_res)
    x = rng.standard_normal((V, C)) * 1.5 + 0.3
    gamma, beta = rng.uniform(0.5, 1.5, C), rng.standard_normal(C) * 0.2
    rm, rv = rng.standard_normal(C) * 0.1, rng.uniform(0.5, 2.0, C)
    res = rng.standard_normal((V, C)) if with_res else None
    dy = rng.standard_normal((V, C))
    momentum, eps = 0.1, 1e-5

    tx, tg, tb = (torch.tensor(a, requires_grad=True) for a in (x, gamma, beta))
    tr = torch.tensor(res, requires_grad=True) if with_res else None
    trm, trv = torch.tensor(rm), torch.tensor(rv)
    ty = F.batch_norm(tx, trm, trv, tg, tb, training, momentum, eps)
    if with_res:
        ty = ty + tr
    if relu:
        ty = torch.relu(ty)
    ty.backward(torch.tensor(dy))

    f = sn.forward(x, gamma, beta, rm, rv, training, momentum, eps, relu, res)
    _close(f["y"], ty.detach().numpy(), "y")
    _close(f["running_mean"], trm.numpy(), "running_mean")
    _close(f["running_var"], trv.numpy(), "running_var")
    if not training:
        assert np.array_equal(f["running_mean"], rm) and np.array_equal(f["running_var"], rv)
    gate = f["y"] > 0 if relu else None
    dx, dgamma, dbeta, dres, _ = sn.backward(dy, gate, x, gamma, f["mean"], f["rstd"], training)
    _close(dx, tx.grad.numpy(), "dx")
    _close(dgamma, tg.grad.numpy(), "dgamma")
    _close(dbeta, tb.grad.numpy(), "dbeta")
    if with_res:
        _close(dres, tr.grad.numpy(), "dresidual")


def test_training_refuses_a_single_row():
    with pytest.raises(ValueError):
        sn.forward(np.zeros((1, 4)), np.ones(4), np.zeros(4), np.zeros(4), np.ones(4), True)
