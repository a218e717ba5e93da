"""CPU proofs of tests/bwd_refs.py, the fp64 restatements test_gpu_bwd_unfused.py holds the
unfused backward GEMMs to:

* against torch autograd in fp64 on conv1x1 -> BatchNorm1d(train) -> ReLU -> dropout -> conv1x1 ->
  BatchNorm1d(train) over B scenes, with the BN-backward coefficients of small_refs.bn_bwd_coefs;
* the bf16 rounding against torch's;
* the sensitivity of every value case of the GPU file: a reference perturbed the way a subtly
  wrong kernel would be (a row of a slice dropped or counted twice, a keep bit flipped, a
  coefficient vector offset by one 8-column chunk inside a 64-column tile, the ReLU mask's > 0
  turned into >= 0) differs from the true one by more than both bounds together somewhere, so
  no output could satisfy both.  Only reference data is perturbed;
* the share of midpoint-flagged operand elements of the bf16 value cases;
* the exactness conditions of the integer data."""
import functools

import numpy as np
import pytest
import torch

import bwd_refs as R
import small_refs as S


@functools.lru_cache(maxsize=None)
def wbase(case):
    d = R.wgrad_data(case, "value")
    return d, R.wgrad_reference(case, d)


@functools.lru_cache(maxsize=None)
def gbase(case):
    d = R.gemm_data(case, "value")
    return d, R.gemm_reference(case, d)


# ---------------------------------------------------------------------------------------
# bf16 rounding
# ---------------------------------------------------------------------------------------
def test_bf16_round_matches_torch():
    r = np.random.default_rng(0)
    x = np.concatenate([r.standard_normal(20000) * 10.0 ** r.integers(-6, 6, 20000),
                        [0.0, 1.0, -1.0, 1.00390625, 1.01171875, 255.5, 256.0, 257.0, 3.0 * 2.0 ** -130]]).astype(np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).double().numpy()
    keep = np.abs(x) >= 2.0 ** -120           # the restatement covers the normal range
    assert np.array_equal(R.bf16_round(x)[keep], want[keep])
    _, dist, q = R.bf16_parts(np.array([1.00390625, 1.0, 1.005]))
    assert dist[0] == 0.0 and dist[1] == q[1] / 2 and 0 < dist[2] < q[2] / 2


# ---------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------
def _autograd_problem(seed, B=3, N=11, C0=5, C1=16, C2=8):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    x0 = rn(B * N, C0)
    W1, W2 = rn(C1, C0).requires_grad_(), rn(C2, C1).requires_grad_()
    g1, b1 = (rn(C1) + 1.5).requires_grad_(), rn(C1).requires_grad_()
    g2, b2 = (rn(C2) + 1.5).requires_grad_(), rn(C2).requires_grad_()
    keep = torch.rand(B * N, C1, generator=g) < 0.7
    ks, eps = 1.0 / 0.7, 1e-5
    y1 = x0 @ W1.T
    y1.retain_grad()
    o1 = torch.nn.functional.batch_norm(y1, None, None, g1, b1, True, 0.1, eps)
    o1.retain_grad()
    ad = torch.relu(o1) * keep * ks
    y2 = ad @ W2.T
    y2.retain_grad()
    o2 = torch.nn.functional.batch_norm(y2, None, None, g2, b2, True, 0.1, eps)
    G, H = rn(B * N, C2), rn(B * N, C1)
    ((o2 * G).sum() + (ad * H).sum()).backward()
    n = lambda t: t.detach().numpy()   # noqa: E731
    M = B * N

    def bn(y, gam, bet):
        mean, var = n(y).mean(0), n(y).var(0)
        rstd = 1.0 / np.sqrt(var + eps)
        return mean, rstd, n(gam) * rstd, n(bet) - mean * n(gam) * rstd

    m1, r1, s1, t1 = bn(y1, g1, b1)
    m2, r2, _, _ = bn(y2, g2, b2)
    c2 = S.bn_bwd_coefs(n(G).sum(0), (n(G) * (n(y2) - m2) * r2).sum(0), None, float(M), m2, r2, n(g2))
    sh = lambda a: a.reshape(B, N, -1)   # noqa: E731
    return dict(B=B, N=N, M=M, G=sh(n(G)), H=sh(n(H)), y1=sh(n(y1)), y2=sh(n(y2)), keep=sh(n(keep)), ks=ks,
                c2=c2, s1=s1, t1=t1, m1=m1, r1=r1, g1=n(g1), W2=n(W2), dW2=n(W2.grad), dy2=sh(n(y2.grad)),
                do1=sh(n(o1.grad)), dg1=n(g1.grad), db1=n(b1.grad), dy1=sh(n(y1.grad)))


@pytest.mark.parametrize("seed", [1, 2])
def test_refs_reproduce_autograd(seed):
    p = _autograd_problem(seed)
    c2 = p["c2"]
    w = R.wgrad_ref(p["G"], p["y2"], c2["alpha"], c2["beta_c"], c2["gamma_c"], p["y1"], p["s1"], p["t1"], p["keep"],
                    p["ks"], R.PRO_BWD, R.PRO_BNRELU, "f32")
    assert np.abs(w["dy"] - p["dy2"]).max() < 1e-10
    assert np.abs(w["dW"] - p["dW2"]).max() < 1e-10
    # dy_mode RAW on the finished dy, x_mode RAW on the finished x: the same product
    w2 = R.wgrad_ref(p["dy2"], None, None, None, None, w["x"], None, None, None, 1.0, R.PRO_RAW, R.PRO_RAW, "f32")
    assert np.abs(w2["dW"] - p["dW2"]).max() < 1e-10
    d = R.dgrad_ref(p["G"], p["y2"], c2["alpha"], c2["beta_c"], c2["gamma_c"], p["W2"].T, p["H"], p["y1"], p["s1"],
                    p["t1"], p["keep"], p["ks"], p["m1"], p["r1"], "f32")
    assert np.abs(d["dz"] - p["do1"]).max() < 1e-10
    assert np.abs(d["raw"] - p["dy2"] @ p["W2"]).max() < 1e-10
    c1 = S.bn_bwd_coefs(d["S1"].sum(0), d["S2"].sum(0), None, float(p["M"]), p["m1"], p["r1"], p["g1"])
    assert np.abs(c1["dgamma"] - p["dg1"]).max() < 1e-10
    assert np.abs(c1["dbeta"] - p["db1"]).max() < 1e-10
    dy1 = c1["alpha"] * d["dz"] + c1["beta_c"] + c1["gamma_c"] * p["y1"]
    assert np.abs(dy1 - p["dy1"]).max() < 1e-10


def test_dgrad_ref_optional_operands():
    p = _autograd_problem(3)
    c2 = p["c2"]
    args = (p["G"], p["y2"], c2["alpha"], c2["beta_c"], c2["gamma_c"], p["W2"].T)
    one, zero = np.ones_like(p["s1"]), np.zeros_like(p["s1"])
    a = R.dgrad_ref(*args, None, p["y1"], None, None, None, 1.0, None, None, "f32")
    b = R.dgrad_ref(*args, np.zeros_like(p["H"]), p["y1"], one, zero, np.ones_like(p["keep"]), 1.0, zero, one, "f32")
    assert np.array_equal(a["dz"], b["dz"]) and np.array_equal(a["S1"], b["S1"])
    assert not a["S2"].any() and b["S2"].any()
    assert np.array_equal(a["gate"], p["y1"] > 0)


# ---------------------------------------------------------------------------------------
# sensitivity
# ---------------------------------------------------------------------------------------
def rejects(ref, pert, names):
    """Some element of some output differs by more than the two bounds together."""
    for nm, bn in names:
        gap = np.abs(ref[nm] - pert[nm]) - (ref[bn] + pert[bn])
        if (gap > 0).any():
            return True
    return False


def rolled(v, tile, width):
    """v with one 8-column chunk of offset inside the columns [tile*width, (tile+1)*width)."""
    v = v.copy()
    lo = tile * width
    v[lo:lo + width] = np.roll(v[lo:lo + width], 8)
    return v


def _row_weights(N, step):
    rows = {"last row dropped": (1, N - 1, 0.0), "first row dropped": (1, 0, 0.0), "row counted twice": (2, N - 1, 2.0)}
    if N > step:
        rows["first row of the second step dropped"] = (0, step, 0.0)
    for name, (b, n, wgt) in rows.items():
        w = np.ones((R.B, N))
        w[b, n] = wgt
        yield name, w


@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=R.wcase_id)
def test_wgrad_value_case_rejects_perturbed_references(case):
    d, ref = wbase(case)
    names = [("dW", "bound")]
    missed = []
    for name, w in _row_weights(case.N, R.wstep(case.cls)):
        if not rejects(ref, R.wgrad_reference(case, d, row_weight=w), names):
            missed.append(name)
    coefs = (["alpha", "beta", "gamma"] if case.dy_mode == R.PRO_BWD else []) + \
            (["s", "t"] if case.x_mode == R.PRO_BNRELU else [])
    for k in coefs:
        C = len(d[k])
        if not rejects(ref, R.wgrad_reference(case, dict(d, **{k: rolled(d[k], C // 64 - 1, 64)})), names):
            missed.append(f"{k} rolled")
    if case.mask:
        b, n = 1, case.N - 1
        x = np.maximum(d["X"][b, n] * d["s"] + d["t"], 0.0)
        opened = np.flatnonzero(x > 0)
        k = opened[np.argsort(x[opened])[len(opened) // 2]]        # the median open channel of the row
        keep = d["keep"].copy()
        keep[b, n, k] ^= True
        if not rejects(ref, R.wgrad_reference(case, dict(d, keep=keep)), names):
            missed.append("keep bit flipped")
    assert not missed, missed


@pytest.mark.parametrize("case", R.GEMM_CASES, ids=R.gcase_id)
def test_gemm_value_case_rejects_perturbed_references(case):
    d, ref = gbase(case)
    dgrad = case.epi == R.EPI_DGRAD
    names = [("dz", "e_dz"), ("S1", "e_S1"), ("S2", "e_S2")] if dgrad else [("raw", "e_raw")]
    missed = []
    for k in ("alpha", "beta", "gamma"):
        width = min(case.K, 64)
        if not rejects(ref, R.gemm_reference(case, dict(d, **{k: rolled(d[k], case.K // width - 1, width)})), names):
            missed.append(f"{k} rolled")
    if dgrad:
        assert ref["zmin"] >= R.ZGAP and ref["zeros"] > 0
        if not rejects(ref, R.gemm_reference(case, d, ge=True), names[:1]):
            missed.append(">= 0")
        sums = names[1:2] if d["rstd"] is None else names[1:]
        for name, w in _row_weights(case.N, 128):
            if not rejects(ref, R.gemm_reference(case, d, row_weight=w), sums):
                missed.append(name)
    if d["keep"] is not None:
        b, n = 1, case.N - 1
        v = np.abs(ref["raw"][b, n] + (0.0 if d["addend"] is None else d["addend"][b, n])) * ref["gate"][b, n]
        opened = np.flatnonzero(v > 0)
        k = opened[np.argsort(v[opened])[len(opened) // 2]]        # the median open column of the row
        keep = d["keep"].copy()
        keep[b, n, k] ^= True
        if not rejects(ref, R.gemm_reference(case, dict(d, keep=keep)), names[:1]):
            missed.append("keep bit flipped")
    assert not missed, missed


# ---------------------------------------------------------------------------------------
# midpoint flags
# ---------------------------------------------------------------------------------------
def test_midpoint_flags_are_rare():
    worst = 0.0
    for case in R.WGRAD_CASES:
        if R.dtype_of(case) == "bf16":
            worst = max(worst, wbase(case)[1]["flagged"])
    for case in R.GEMM_CASES:
        if R.dtype_of(case) == "bf16":
            worst = max(worst, gbase(case)[1]["flagged"])
    assert 0.0 < worst <= 1e-3, worst
    for case in R.WGRAD_CASES + R.GEMM_CASES:
        if R.dtype_of(case) == "f32":
            ref = wbase(case)[1] if isinstance(case, R.WCase) else gbase(case)[1]
            assert ref["flagged"] == 0.0


# ---------------------------------------------------------------------------------------
# exact data
# ---------------------------------------------------------------------------------------
def _exact_in_bf16(a, what):
    a = np.asarray(a)
    assert np.abs(a).max() <= 256 and np.array_equal(a, np.rint(a)) and np.array_equal(R.bf16_round(a), a), what


@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=R.wcase_id)
def test_wgrad_exact_data_is_exact(case):
    d = R.wgrad_data(case, "exact")
    ref = R.wgrad_reference(case, d)
    if case.dy_mode == R.PRO_BWD:
        _exact_in_bf16(d["gamma"] * d["Y"] + d["beta"], "gamma Y + beta")
        _exact_in_bf16(d["alpha"] * d["dZ"], "alpha dZ")
    _exact_in_bf16(ref["dy"], "dy")
    _exact_in_bf16(ref["x"], "x")
    M = R.B * case.N
    total = np.abs(ref["dy"]).reshape(M, -1).T @ np.abs(ref["x"]).reshape(M, -1)
    assert total.max() < 2 ** 24 and np.array_equal(ref["dW"], np.rint(ref["dW"]))
    assert ref["flagged"] == 0.0 and np.abs(ref["dW"]).max() > 0


@pytest.mark.parametrize("case", R.GEMM_CASES, ids=R.gcase_id)
def test_gemm_exact_data_is_exact(case):
    d = R.gemm_data(case, "exact")
    ref = R.gemm_reference(case, d)
    _exact_in_bf16(d["gamma"] * d["Y"] + d["beta"], "gamma Y + beta")
    _exact_in_bf16(ref["dy"], "dy")
    assert set(np.unique(d["W"])) <= {-1.0, 0.0, 1.0}
    assert (np.abs(ref["dy"]) @ np.abs(d["W"]).T).max() <= 256      # every partial sum along K is below this
    _exact_in_bf16(ref["raw"], "raw")
    if case.epi == R.EPI_RAW:
        return
    _exact_in_bf16(ref["dz"], "dz")
    assert ref["zeros"] > 0 and not ref["dz"][~ref["gate"]].any()
    dz, Yp = np.abs(ref["dz"]), np.abs(d["Yp"])
    assert dz.sum(1).max() < 2 ** 24 and (dz * Yp).sum(1).max() < 2 ** 24
    if d["rstd"] is not None:
        assert set(np.unique(d["rstd"])) <= {0.5, 1.0, 2.0} and np.array_equal(d["mean"], np.rint(d["mean"]))
        terms = dz * np.abs(d["Yp"] - d["mean"]) * d["rstd"]               # multiples of 1/2
        assert np.array_equal(2 * terms, np.rint(2 * terms)) and (2 * terms).sum(1).max() < 2 ** 24
        assert (np.abs(d["mean"]) * dz.sum(1)).max() < 2 ** 24
