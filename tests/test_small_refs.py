"""The fp64 references of tests/small_refs.py against torch itself in fp64, on the CPU: what
makes the GPU tests of the small kernels trustworthy.  Every comparison agrees to ~1e-12."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_refs as R

TOL = 1e-11


def _close(a, b, tol=TOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(1.0, float(np.abs(b).max()))
    assert a.shape == b.shape
    assert float(np.abs(a - b).max()) <= tol * scale, float(np.abs(a - b).max())


CHUNKINGS = [(1, 37, 1, 37), (3, 1000, 8, 128), (2, 300 * 7 + 5, 301, 7), (2, 64, 1, 64)]


@pytest.mark.parametrize("B,N,cps,rpc", CHUNKINGS)
@pytest.mark.parametrize("with_moff", [False, True])
def test_bn_forward_reference(B, N, cps, rpc, with_moff):
    C = 5
    g = torch.Generator().manual_seed(N + cps)
    y = torch.randn(B, N, C, generator=g, dtype=torch.float64) * 2.0 + torch.randn(C, generator=g, dtype=torch.float64)
    gamma = torch.randn(C, generator=g, dtype=torch.float64)
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    moff = torch.randn(C, generator=g, dtype=torch.float64) if with_moff else None
    rm0 = torch.randn(C, generator=g, dtype=torch.float64)
    rv0 = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    st = R.welford_partials(y.numpy(), cps, rpc, rounded=False)
    out = R.bn_fwd_from_partials(st, B, N, cps, rpc, gamma.numpy(), beta.numpy(),
                                 None if moff is None else moff.numpy(), rm0.numpy(), rv0.numpy(), 0.1, 1e-5)
    # torch sees the activation with the omitted constant put back; the normalised output is
    # the same, and only running_mean moves by it
    x = y + (moff if moff is not None else 0.0)
    rm, rv = rm0.clone(), rv0.clone()
    z = F.batch_norm(x.reshape(-1, C), rm, rv, gamma, beta, training=True, momentum=0.1, eps=1e-5)
    _close(y.reshape(-1, C).numpy() * out["scale"] + out["shift"], z.numpy())
    _close(out["rmean"], rm.numpy())
    _close(out["rvar"], rv.numpy())
    _close(out["mean"], y.reshape(-1, C).mean(0).numpy())
    _close(out["rstd"], 1.0 / np.sqrt(y.reshape(-1, C).var(0, unbiased=False).numpy() + 1e-5))
    _close(out["scene_sum"], y.sum(1).numpy())
    assert (out["shift_terms"] >= np.abs(out["shift"]) - 1e-15).all()


@pytest.mark.parametrize("B,N,cps,rpc", CHUNKINGS)
def test_bn_backward_reference(B, N, cps, rpc):
    C = 6
    g = torch.Generator().manual_seed(7 * N + cps)
    y = (torch.randn(B, N, C, generator=g, dtype=torch.float64) * 1.5 + 0.3).requires_grad_()
    gamma = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    beta = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    dz = torch.randn(B, N, C, generator=g, dtype=torch.float64)
    z = F.batch_norm(y.reshape(-1, C), None, None, gamma, beta, training=True, eps=1e-5)
    (z * dz.reshape(-1, C)).sum().backward()
    yn = y.detach().numpy()
    mean = yn.reshape(-1, C).mean(0)
    rstd = 1.0 / np.sqrt(yn.reshape(-1, C).var(0) + 1e-5)
    st = R.sum_partials(dz.numpy(), (yn - mean) * rstd, cps, rpc, rounded=False)
    out = R.bn_bwd_from_partials(st, B, N, cps, mean, rstd, gamma.detach().numpy(), yn.sum(1))
    dy = out["alpha"] * dz.numpy() + out["beta_c"] + out["gamma_c"] * yn
    _close(dy, y.grad.numpy())
    _close(out["dgamma"], gamma.grad.numpy())
    _close(out["dbeta"], beta.grad.numpy())
    _close(out["dbias"], y.grad.sum((0, 1)).numpy(), 1e-10)
    _close(out["scene_s1"], dz.sum(1).numpy())
    no_sum = R.bn_bwd_from_partials(st, B, N, cps, mean, rstd, gamma.detach().numpy(), None)
    assert (no_sum["dbias"] == 0).all()
    _close(no_sum["beta_c"], out["beta_c"])


@pytest.mark.parametrize("B,N,Cs,Cg", [(1, 9, 4, 6), (5, 37, 7, 11), (9, 12, 16, 8)])
def test_pool_backward_reference(B, N, Cs, Cg):
    g = torch.Generator().manual_seed(100 * B + Cg)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    col_off, ldw = 3, 3 + Cg + 2
    y_g = rnd(B, N, Cg).requires_grad_()
    g_gamma = rnd(Cg)
    g_gamma[::3] = -g_gamma[::3].abs()                    # both signs: max rows and min rows
    g_gamma[1::3] = g_gamma[1::3].abs()
    g_gamma.requires_grad_()
    g_beta = (rnd(Cg) * 0.5).requires_grad_()
    W = rnd(Cs, ldw).requires_grad_()
    local = rnd(B, N, Cs)
    a5 = torch.relu(F.batch_norm(y_g.reshape(-1, Cg), None, None, g_gamma, g_beta, training=True, eps=1e-5))
    pooled, am = a5.reshape(B, N, Cg).max(1)
    v = pooled @ W[:, col_off:col_off + Cg].T
    y_s1 = local + v[:, None, :]
    # the incoming gradient of y_s1 in the form the library holds it
    alpha, beta, gamma, dz = rnd(Cs), rnd(Cs) * 0.1, rnd(Cs) * 0.1, rnd(B, N, Cs)
    dy_s1 = alpha * dz + beta + gamma * y_s1.detach()
    (y_s1 * dy_s1).sum().backward()

    yn = y_g.detach().numpy()
    mean = yn.reshape(-1, Cg).mean(0)
    rstd = 1.0 / np.sqrt(yn.reshape(-1, Cg).var(0) + 1e-5)
    ysel = np.take_along_axis(yn, am.numpy()[:, None, :], 1)[:, 0]
    out, err = R.pool_bwd_ref(N, alpha.numpy(), beta.numpy(), gamma.numpy(), dz.sum(1).numpy(),
                              y_s1.detach().sum(1).numpy(), W.detach().numpy(), col_off,
                              pooled.detach().numpy(), ysel, mean, rstd, g_gamma.detach().numpy(), yn.sum(1))
    _close(out["csum"], dy_s1.sum(1).numpy())
    _close(out["dW"], W.grad[:, col_off:col_off + Cg].numpy())
    assert (W.grad[:, :col_off] == 0).all() and (W.grad[:, col_off + Cg:] == 0).all()
    _close(out["dgamma"], g_gamma.grad.numpy())
    _close(out["dbeta"], g_beta.grad.numpy())
    dense = out["beta_c"] + out["gamma_c"] * yn
    rows = am.numpy()
    for b in range(B):
        dense[b, rows[b], np.arange(Cg)] += out["sp"][b]
    _close(dense, y_g.grad.numpy())
    _close(out["dbias"], y_g.grad.sum((0, 1)).numpy(), 1e-10)
    for k, e in err.items():
        assert e.shape == out[k].shape and (e >= 0).all() and np.isfinite(e).all(), k


@pytest.mark.parametrize("cps,rpc", [(1, 50), (4, 13), (7, 8)])
def test_pool_forward_reference(cps, rpc):
    """pool_partials + pool_finalize_ref: the max over a scene of relu(y*s + t), taken at the
    first row that attains it, from per-chunk records."""
    B, N, C = 3, 50, 9
    g = torch.Generator().manual_seed(cps)
    y = torch.randint(-4, 5, (B, N, C), generator=g).float()       # many ties
    s = torch.randn(C, generator=g)
    s[::2] = -s[::2].abs()
    t = torch.randn(C, generator=g)
    ref = R.pool_finalize_ref(R.pool_partials(y.numpy(), cps, rpc), B, N, cps, s.numpy(), t.numpy())
    a = torch.relu(y.double() * s.double() + t.double())
    _close(ref["g"], a.max(1).values.numpy())
    rows = ref["am"] - (np.arange(B) * N)[:, None]
    yd = y.double() * torch.sign(s).double()
    first = (yd == yd.max(1, keepdim=True).values).double().argmax(1).numpy()   # first row at the extremum
    assert np.array_equal(rows, first)
    assert np.array_equal(ref["ysel"], np.take_along_axis(y.numpy(), rows[:, None, :], 1)[:, 0])


@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_adam_reference(wd):
    g = torch.Generator().manual_seed(3)
    p = torch.randn(1000, generator=g, dtype=torch.float64).requires_grad_()
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    pr, m, v = p.detach().numpy().copy(), np.zeros(1000), np.zeros(1000)
    for step in range(1, 6):
        gr = torch.randn(1000, generator=g, dtype=torch.float64)
        p.grad = gr.clone()
        opt.step()
        pr, m, v, ge, _ = R.adam_ref(pr, gr.numpy(), m, v, step, 1e-3, 0.9, 0.999, 1e-8, wd)
        assert np.array_equal(ge, gr.numpy())
        _close(pr, p.detach().numpy(), 1e-12)
        st = opt.state[p]
        _close(m, st["exp_avg"].numpy(), 1e-12)
        _close(v, st["exp_avg_sq"].numpy(), 1e-12)
    # a gradient scale is the same step on the scaled gradient
    a = R.adam_ref(pr, gr.numpy(), m, v, 6, 1e-3, 0.9, 0.999, 1e-8, wd, scale=0.37)
    b = R.adam_ref(pr, gr.numpy() * 0.37, m, v, 6, 1e-3, 0.9, 0.999, 1e-8, wd)
    _close(a[0], b[0], 1e-15)


def _head_inputs(M, C, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    y = (rnd(M, 128) * 1.5 + 0.2).requires_grad_()
    s = (torch.rand(128, generator=g, dtype=torch.float64) + 0.5) * torch.where(rnd(128) < -0.67, -1.0, 1.0)
    t, mean, rstd = rnd(128) * 0.5, rnd(128) * 0.3, (rnd(128) * 0.1 + 1.0).abs()
    W = (rnd(C, 128) * 0.1).requires_grad_()
    b = (rnd(C) * 0.2).requires_grad_()
    return g, y, s, t, mean, rstd, W, b


@pytest.mark.parametrize("M,C", [(37, 1), (50, 3), (41, 17), (23, 100)])
@pytest.mark.parametrize("with_wsum", [True, False])
def test_head_reference_ce(M, C, with_wsum):
    """head_ref in CE mode is F.cross_entropy (weights, ignore_index=-1) on seg_conv4 of
    relu(y*s + t) and its gradients; labels outside [0, C) count as ignored."""
    g, y, s, t, mean, rstd, W, b = _head_inputs(M, C, 10 * M + C)
    lab = torch.randint(-1, C, (M,), generator=g)
    cw = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    if C > 2:
        cw[C // 2] = 0.0                                # a class of weight exactly 0
    lab[0] = C - 1                                      # at least one valid row of non-zero weight
    valid = lab >= 0
    D = float(cw[lab[valid]].sum())
    logits = torch.relu(y * s + t) @ W.T + b
    loss = F.cross_entropy(logits, lab, weight=cw, ignore_index=-1)      # mean: sum w nll / D
    loss.backward()
    odd = lab.clone()
    odd[~valid] = torch.tensor([-7, C, C + 5, -1])[torch.arange(int((~valid).sum())) % 4]   # all ignored alike
    ref = R.head_ref(y.detach().numpy(), s.numpy(), t.numpy(), mean.numpy(), rstd.numpy(), W.detach().numpy(),
                     b.detach().numpy(), R.HEAD_CE, labels=odd.numpy(), class_weight=cw.numpy(),
                     wsum=D if with_wsum else None)
    k = 1.0 if with_wsum else D                          # without wsum the gradients are D times torch's
    _close(ref["logits"], logits.detach().numpy())
    _close(ref["loss_sum"] / D, loss.item(), 1e-12)
    _close(ref["dz"] * s.numpy(), y.grad.numpy() * k, 1e-12)
    _close(ref["dW"], W.grad.numpy() * k, 1e-12)
    _close(ref["db"], b.grad.numpy() * k, 1e-12)
    assert (ref["dl"][~valid.numpy()] == 0).all() and (ref["dz"][ref["a"] == 0] == 0).all()
    xh = (y.detach().numpy() - mean.numpy()) * rstd.numpy()
    _close(ref["S1"], ref["dz"].sum(0), 1e-13)
    _close(ref["S2"], (ref["dz"] * xh).sum(0), 1e-13)
    # the absolute sums dominate what they bound, and the bounds are finite and non-negative
    for name in ("logits", "dz", "S1", "S2", "dW", "db"):
        assert (ref["abs_" + name] >= np.abs(ref[name]) - 1e-13).all(), name
    assert ref["abs_loss_sum"] >= abs(ref["loss_sum"])
    for name, e in R.head_bounds(ref, W.detach().numpy(), R.HEAD_CE, 64, bf16_dz=True).items():
        e = np.asarray(e)
        assert np.isfinite(e).all() and (e >= 0).all(), name
        if name in ref:
            assert e.shape == np.shape(ref[name]), name


@pytest.mark.parametrize("M,C", [(37, 2), (29, 65)])
def test_head_reference_bwd(M, C):
    """head_ref in BWD mode is torch.autograd.grad of the logits with the given dlogits."""
    g, y, s, t, mean, rstd, W, b = _head_inputs(M, C, 3 * M + C)
    dlog = torch.randn(M, C, generator=g, dtype=torch.float64)
    logits = torch.relu(y * s + t) @ W.T + b
    gy, gW, gb = torch.autograd.grad(logits, (y, W, b), dlog)
    ref = R.head_ref(y.detach().numpy(), s.numpy(), t.numpy(), mean.numpy(), rstd.numpy(), W.detach().numpy(),
                     b.detach().numpy(), R.HEAD_BWD, dlogits=dlog.numpy())
    _close(ref["logits"], logits.detach().numpy())
    _close(ref["dz"] * s.numpy(), gy.numpy(), 1e-12)
    _close(ref["dW"], gW.numpy(), 1e-12)
    _close(ref["db"], gb.numpy(), 1e-12)
    xh = (y.detach().numpy() - mean.numpy()) * rstd.numpy()
    _close(ref["S2"], (ref["dz"] * xh).sum(0), 1e-13)
    fwd = R.head_ref(y.detach().numpy(), s.numpy(), t.numpy(), None, None, W.detach().numpy(),
                     b.detach().numpy(), R.HEAD_FWD)
    assert np.array_equal(fwd["logits"], ref["logits"]) and "dz" not in fwd


def test_scene_gemv_reference_and_bounds():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 10, generator=g, dtype=torch.float64)
    W = torch.randn(4, 15, generator=g, dtype=torch.float64)
    b = torch.randn(4, generator=g, dtype=torch.float64)
    v, e = R.scene_gemv_ref(x.numpy(), W.numpy(), 2, b.numpy())
    _close(v, F.linear(x, W[:, 2:12], b).numpy())
    assert e.shape == v.shape and (e > 0).all()
    assert R.sum_bound(4, 2.0) == 4 * 2.0 ** -24 * 2.0
    assert R.round_bound(1.0, -3.0) == 2.0 ** -23 * 4.0
    with pytest.raises(AssertionError):
        R.assert_within(np.array([1.0, np.nan]), np.array([1.0, 1.0]), np.array([1e-3, 1e-3]), "nan")
    with pytest.raises(AssertionError):
        R.assert_within(np.array([1.1]), np.array([1.0]), np.array([1e-3]), "far")
    R.assert_within(np.array([1.0005]), np.array([1.0]), np.array([1e-3]), "near")
