"""CPU proofs of tests/fused_bwd_refs.py, the fp64 restatements test_gpu_fused_bwd_direct.py holds
the fused and folded backward kernels to:

* the folded references, with WaT, H and c unrounded, against torch autograd in fp64 on
  conv1x1 (+ per-scene bias) -> BatchNorm1d(train) with the BN-backward coefficients of
  small_refs.bn_bwd_coefs: seg_conv1's local half (dX, dW) and conv5's input gradient (dz, S1, S2);
* the sensitivity of every value case of the GPU file: a reference perturbed the way a subtly
  wrong kernel would be differs from the true one by more than both bounds together somewhere
  (test_bwd_refs.rejects).  The perturbations: the first or last row of a slice dropped or counted
  twice (the one-row tail slice included), a keep bit flipped, every coefficient vector offset by
  one 8-column chunk inside a tile, pa / pb exchanged with es / et, > 0 turned into >= 0, the
  scene bias / cvec / S_b of the neighbouring scene, H transposed;
* the share of midpoint-flagged operand elements of the bf16 value cases;
* the exactness conditions of the integer data, and zeros in every gate."""
import functools

import numpy as np
import pytest
import torch

import fused_bwd_refs as F
import small_refs as S
from test_bwd_refs import rejects, rolled

R = F.R


@functools.lru_cache(maxsize=None)
def bn_base(case):
    d = F.bn_data(case, "value")
    return d, F.bn_reference(case, d)


@functools.lru_cache(maxsize=None)
def folded_base(case):
    d = F.folded_data(case, "value")
    return d, F.folded_ref(d, geometry=F.folded_geometry(case))


@functools.lru_cache(maxsize=None)
def cat_base(case):
    d = F.cat_data(case, "value")
    return d, F.cat_reference(case, d)


@functools.lru_cache(maxsize=None)
def wc5_base(case):
    d = R.wgrad_data(case, "value")
    return d, R.wgrad_reference(case, d)


# ---------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_folded_ref_reproduces_autograd(seed):
    """seg_conv1's local half: x = relu(X s + t), Y' = x W^T + sbias[b], BatchNorm(train); autograd's
    dL/dx and dL/dW are dX and dW of the folded form with WaT and H unrounded."""
    Bc, N = 3, 11
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    X, s, t = rn(Bc * N, F.F_CIN), rn(F.F_CIN) + 1.5, rn(F.F_CIN)
    x = torch.relu(X * s + t).requires_grad_()
    W = rn(F.F_COUT, F.F_CIN).requires_grad_()
    sb = rn(Bc, F.F_COUT)
    y = x @ W.T + sb.repeat_interleave(N, 0)
    gam = rn(F.F_COUT) + 1.5
    o = torch.nn.functional.batch_norm(y, None, None, gam, torch.zeros_like(gam), True, 0.1, 1e-5)
    G = rn(Bc * N, F.F_COUT)
    (o * G).sum().backward()
    n = lambda a: a.detach().numpy()   # noqa: E731
    mean, rstd = n(y).mean(0), 1.0 / np.sqrt(n(y).var(0) + 1e-5)
    c = S.bn_bwd_coefs(n(G).sum(0), (n(G) * (n(y) - mean) * rstd).sum(0), None, float(Bc * N), mean, rstd, n(gam))
    Wf = np.zeros((F.F_COUT, F.F_LDW))
    Wf[:, :F.F_CIN] = n(W)
    sh = lambda a: a.reshape(Bc, N, -1)   # noqa: E731
    d = dict(dZ=sh(n(G)), X=sh(n(X)), s=n(s), t=n(t), alpha=c["alpha"], beta=c["beta_c"], gamma=c["gamma_c"], W=Wf,
             sbias=n(sb), WaT=(c["alpha"][:, None] * n(W)).T, H=n(W).T @ (c["gamma_c"][:, None] * n(W)))
    ref = F.folded_ref(d, dtype="f32")
    assert np.abs(ref["dX"] - sh(n(x.grad))).max() < 1e-9
    assert np.abs(ref["dW"] - n(W.grad)).max() < 1e-9


@pytest.mark.parametrize("seed", [3, 4])
def test_cat_ref_reproduces_autograd(seed):
    """conv5's input gradient: z4 = y4 pa + pb, a4 = relu(z4), y5 = a4 W5^T, BatchNorm(train);
    autograd's dL/dz4 is the EPI_DGRAD output with es = pa, et = pb, Yp = y4, and S1 / S2 are its
    per-scene sums."""
    Bc, N, K2, K1 = 3, 13, 8, 16
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    y4, pa, pb = rn(Bc * N, K2), rn(K2) + 1.5, rn(K2)
    z4 = (y4 * pa + pb).requires_grad_()
    W5 = rn(K1, K2)
    y5 = torch.relu(z4) @ W5.T
    gam = rn(K1) + 1.5
    o = torch.nn.functional.batch_norm(y5, None, None, gam, torch.zeros_like(gam), True, 0.1, 1e-5)
    G = rn(Bc * N, K1)
    (o * G).sum().backward()
    n = lambda t: t.detach().numpy()   # noqa: E731
    mean, rstd = n(y5).mean(0), 1.0 / np.sqrt(n(y5).var(0) + 1e-5)
    c = S.bn_bwd_coefs(n(G).sum(0), (n(G) * (n(y5) - mean) * rstd).sum(0), None, float(Bc * N), mean, rstd, n(gam))
    W5n = n(W5)
    m4, r4 = rn(K2).numpy(), np.abs(rn(K2).numpy()) + 0.5
    sh = lambda a: a.reshape(Bc, N, -1)   # noqa: E731
    case = F.CCase("catf", K1, K2, K2, "plain", N, 0)
    d = dict(dZ=sh(n(G)), y=sh(n(y4)), pa=n(pa), pb=n(pb), bias=c["beta_c"] @ W5n,
             W=np.concatenate([(c["alpha"][:, None] * W5n).T, W5n.T @ (c["gamma_c"][:, None] * W5n)], 1),
             Yp=sh(n(y4)), es=n(pa), et=n(pb), mean=m4, rstd=r4, addend=None, keep=None, keep_scale=1.0)
    ref = F.cat_reference(case, d)
    want = sh(n(z4.grad))
    assert np.abs(ref["dz"] - want).max() < 1e-9
    assert np.abs(ref["S1"] - want.sum(1)).max() < 1e-9
    assert np.abs(ref["S2"] - (want * (sh(n(y4)) - m4) * r4).sum(1)).max() < 1e-9


# ---------------------------------------------------------------------------------------
# sensitivity
# ---------------------------------------------------------------------------------------
def slice_rows(N, rps, n):
    """Row perturbations at the edges of the slices of a scene: (name, scene, row, weight)."""
    sl = [(lo, hi) for lo, hi in F.slices(N, rps, n) if hi > lo]
    lo, hi = sl[-1]                                   # the tail slice (one row at the N = k step + 1 edges)
    rows = {"first row of the tail slice dropped": (1, lo, 0.0), "last row of the tail slice dropped": (2, hi - 1, 0.0),
            "last row of the tail slice counted twice": (0, hi - 1, 2.0), "first row dropped": (2, 0, 0.0),
            "first row counted twice": (1, 0, 2.0), "last row of the first slice dropped": (0, sl[0][1] - 1, 0.0)}
    for name, (b, r, wgt) in rows.items():
        yield name, b, r, wgt


def weights(Bc, N, b, r, wgt):
    w = np.ones((Bc, N))
    w[b, r] = wgt
    return w


def flipped(keep, b, n, strength):
    """keep with the bit of the median open column (by strength > 0) of row (b, n) flipped."""
    opened = np.flatnonzero(strength > 0)
    k = opened[np.argsort(strength[opened])[len(opened) // 2]]
    keep = keep.copy()
    keep[b, n, k] ^= True
    return keep


@pytest.mark.parametrize("case", F.BN_CASES, ids=R.gcase_id)
def test_bn_value_case_rejects_perturbed_references(case):
    d, ref = bn_base(case)
    dz_names, st_names, dw_names = [("dz", "e_dz")], [("S1", "e_S1"), ("S2", "e_S2")], [("dW", "e_dW")]
    missed = []
    cps, rpc = F.bn_geometry(case)
    for name, b, r, wgt in slice_rows(case.N, rpc, cps):
        p = F.bn_reference(case, d, row_weight=weights(F.B, case.N, b, r, wgt))
        if not (rejects(ref, p, st_names) and rejects(ref, p, dw_names)):
            missed.append(name)
    for k in ("alpha", "beta", "gamma"):
        width = min(case.K, 64)
        p = F.bn_reference(case, dict(d, **{k: rolled(d[k], case.K // width - 1, width)}))
        if not (rejects(ref, p, dz_names) and rejects(ref, p, dw_names)):
            missed.append(f"{k} rolled")
    for k in ("es", "et"):
        p = F.bn_reference(case, dict(d, **{k: rolled(d[k], case.Ncols // 64 - 1, 64)}))
        if not (rejects(ref, p, dz_names) and rejects(ref, p, dw_names)):
            missed.append(f"{k} rolled")
    for k in ("mean", "rstd"):
        if not rejects(ref, F.bn_reference(case, dict(d, **{k: rolled(d[k], case.Ncols // 64 - 1, 64)})), st_names[1:]):
            missed.append(f"{k} rolled")
    assert ref["zmin"] >= R.ZGAP and ref["zeros"] > 0
    if not rejects(ref, F.bn_reference(case, d, ge=True), dz_names):
        missed.append(">= 0")
    if d["keep"] is not None:
        b, n = 1, case.N - 1
        keep = flipped(d["keep"], b, n, np.abs(ref["raw"][b, n]) * ref["gate"][b, n])
        p = F.bn_reference(case, dict(d, keep=keep))
        if not (rejects(ref, p, dz_names) and rejects(ref, p, dw_names)):
            missed.append("keep bit flipped")
    assert not missed, missed


@pytest.mark.parametrize("case", F.FOLDED_CASES, ids=F.fcase_id)
def test_folded_value_case_rejects_perturbed_references(case):
    d, ref = folded_base(case)
    dx, dw = [("dX", "e_dX")], [("dW", "e_dW")]
    missed = []
    sps, rps = F.folded_geometry(case)
    slabs = [("slab_R", "e_slab_R"), ("slab_G", "e_slab_G"), ("slab_S", "e_slab_S")]
    for name, b, r, wgt in slice_rows(case.N, rps, sps):
        p = F.folded_ref(d, row_weight=weights(case.B, case.N, b, r, wgt), geometry=(sps, rps))
        # every slab shows a row; dW does too unless M is large (B = 16: 65552 rows in one sum)
        if not (all(rejects(ref, p, [nm]) for nm in slabs) and (case.B > F.B or rejects(ref, p, dw))):
            missed.append(name)
    for k in ("alpha", "beta", "gamma"):
        if not rejects(ref, F.folded_ref(dict(d, **{k: rolled(d[k], 7, 64)})), dw):
            missed.append(f"{k} rolled (dW)")
    for k in ("beta", "gamma"):                      # through cvec
        if not rejects(ref, F.folded_ref(dict(d, **{k: rolled(d[k], 7, 64)})), dx):
            missed.append(f"{k} rolled (dX)")
    for k in ("s", "t"):
        p = F.folded_ref(dict(d, **{k: rolled(d[k], 0, 64)}))
        if not (rejects(ref, p, dx) and rejects(ref, p, dw)):
            missed.append(f"{k} rolled")
    perturbed = {"WaT rolled": dict(WaT=np.roll(d["WaT"], 8, 1)), "H transposed": dict(H=d["H"].T.copy()),
                 "cvec of the neighbouring scene": dict(cvec_shift=1), ">= 0": dict(ge=True)}
    for name, kw in perturbed.items():
        if not rejects(ref, F.folded_ref(d, **kw), dx):
            missed.append(name)
    if not rejects(ref, F.folded_ref(d, sb_shift=1), dw):
        missed.append("S_b credited to the neighbouring scene")
    p = F.folded_ref(dict(d, sbias=np.roll(d["sbias"], 1, 0)))
    if not (rejects(ref, p, dx) and rejects(ref, p, dw)):
        missed.append("scene_bias of the neighbouring scene")
    assert ref["zeros"] > 0
    assert not missed, missed


def _swapped(d):
    return dict(d, pa=d["es"], pb=d["et"], es=d["pa"], et=d["pb"])


@pytest.mark.parametrize("case", F.CAT_CASES, ids=F.ccase_id)
def test_cat_value_case_rejects_perturbed_references(case):
    d, ref = cat_base(case)
    dz, s1 = [("dz", "e_dz")], [("S1", "e_S1")]
    sums = s1 if d["rstd"] is None else s1 + [("S2", "e_S2")]
    missed = []
    cps, rpc = F.cat_geometry(case)
    for name, b, r, wgt in slice_rows(case.N, rpc, cps):
        if not rejects(ref, F.cat_reference(case, d, row_weight=weights(F.B, case.N, b, r, wgt)), sums):
            missed.append(name)
    for k in ("pa", "pb"):
        width = min(case.K2, 64)
        if not rejects(ref, F.cat_reference(case, dict(d, **{k: rolled(d[k], case.K2 // width - 1, width)})), dz):
            missed.append(f"{k} rolled")
    for k in ("es", "et", "bias"):
        if not rejects(ref, F.cat_reference(case, dict(d, **{k: rolled(d[k], case.Ncols // 64 - 1, 64)})), dz):
            missed.append(f"{k} rolled")
    if d["rstd"] is not None:
        for k in ("mean", "rstd"):
            if not rejects(ref, F.cat_reference(case, dict(d, **{k: rolled(d[k], case.Ncols // 64 - 1, 64)})), sums[1:]):
                missed.append(f"{k} rolled")
    assert ref["zmin"] >= R.ZGAP and ref["zeros"] > 0
    if not rejects(ref, F.cat_reference(case, d, ge=True), dz):
        missed.append(">= 0")
    if case.K2 == case.Ncols:
        if not rejects(ref, F.cat_reference(case, _swapped(d)), dz):
            missed.append("pa / pb exchanged with es / et")
        W = d["W"].copy()
        W[:, case.K1:] = W[:, case.K1:].T
        if not rejects(ref, F.cat_reference(case, dict(d, W=W)), dz):
            missed.append("H transposed")
    if d["keep"] is not None:
        b, n = 1, case.N - 1
        v = np.abs(ref["raw"][b, n] + d["bias"] + (0.0 if d["addend"] is None else d["addend"][b, n])) * ref["gate"][b, n]
        if not rejects(ref, F.cat_reference(case, dict(d, keep=flipped(d["keep"], b, n, v))), dz):
            missed.append("keep bit flipped")
    assert not missed, missed


@pytest.mark.parametrize("case", F.WC5_CASES, ids=R.wcase_id)
def test_wgrad_c5_value_case_rejects_perturbed_references(case):
    d, ref = wc5_base(case)
    names = [("dW", "bound")]
    missed = []
    sps, rps = F.wc5_geometry(case)
    for name, b, r, wgt in slice_rows(case.N, rps, sps):
        if not rejects(ref, R.wgrad_reference(case, d, row_weight=weights(F.B, case.N, b, r, wgt)), names):
            missed.append(name)
    for k in ("s", "t"):
        if not rejects(ref, R.wgrad_reference(case, dict(d, **{k: rolled(d[k], 1, 64)})), names):
            missed.append(f"{k} rolled")
    assert not missed, missed


@pytest.mark.parametrize("case", F.FOLD_CASES, ids=F.foldcase_id)
def test_fold_value_case_rejects_perturbed_references(case):
    d = F.fold_data(case, "value")
    ref = F.fold_ref(case, d)
    missed = []
    for k, names in (("alpha", [("WsT", "e_WsT")]), ("beta", [("c", "e_c")]), ("gamma", [("H", "e_H")])):
        if not rejects(ref, F.fold_ref(case, dict(d, **{k: rolled(d[k], case.Cout // 64 - 1, 64)})), names):
            missed.append(f"{k} rolled")
    W = d["W"].copy()
    W[-1, :case.Cin] = 0.0                            # the last row of W left out of the sums
    if not rejects(ref, F.fold_ref(case, dict(d, W=W)), [("H", "e_H"), ("c", "e_c")]):
        missed.append("last row of W dropped")
    assert not missed, missed


# ---------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------
def test_case_geometries_are_the_edges_they_name():
    g = {c.N: F.bn_geometry(c) for c in F.BN_CASES if c.cls == "bn64"}
    assert g[257] == (2, 192) and g[65] == (1, 128) and g[64] == (1, 64)      # 192 + 65 rows: a step and a row
    g = {c.N: F.bn_geometry(c) for c in F.BN_CASES if c.cls == "seg4"}
    assert g[129] == (2, 80) and g[17] == (1, 32) and g[48] == (1, 48) and g[64] == (1, 64)
    assert F.folded_geometry(F.FCase("folded", 16, 4097)) == (16, 320) and -(-4097 // 320) == 13
    assert F.folded_geometry(F.FCase("folded", 3, 257)) == (2, 192)
    g = {(c.cls, c.N, c.sps): F.wc5_geometry(c) for c in F.WC5_CASES if c.Cout == 256}
    assert g[("c5", 129, 0)] == (2, 128) and g[("c5", 387, 3)] == (3, 192) and g[("c5", 130, 4)] == (4, 64)
    g = {(c.N, c.cps): F.cat_geometry(c) for c in F.CAT_CASES if c.cls == "c5"}
    assert g[(261, 2)] == (2, 256) and g[(129, 0)][1] % 128 == 0


# ---------------------------------------------------------------------------------------
# midpoint flags
# ---------------------------------------------------------------------------------------
def test_midpoint_flags_are_rare():
    worst = 0.0
    for case in F.BN_CASES:
        worst = max(worst, bn_base(case)[1]["flagged"])
    for case in F.FOLDED_CASES:
        worst = max(worst, folded_base(case)[1]["flagged"])
    for case in F.WC5_CASES:
        worst = max(worst, wc5_base(case)[1]["flagged"])
    for case in F.CAT_CASES:
        f = cat_base(case)[1]["flagged"]
        if F.cdtype(case) == "f32":
            assert f == 0.0
        else:
            worst = max(worst, f)
    assert 0.0 < worst <= 1e-3, worst
    for case in F.FOLD_CASES:
        ref = F.fold_ref(case, F.fold_data(case, "value"))
        if case.dtype == "f32":
            assert ref["flagged"] == 0.0 and ref["flagged_H"] == 0.0
        else:                                         # WsT: one fp32 rounding; H: fold_ref's docstring
            assert ref["flagged"] <= 1e-3 and ref["flagged_H"] <= 2 * (case.Cout + 1) * 2.0 ** -16 * 1.1


# ---------------------------------------------------------------------------------------
# exact data
# ---------------------------------------------------------------------------------------
def _exact_in_bf16(a, what):
    a = np.asarray(a)
    assert np.abs(a).max() <= 256 and np.array_equal(a, np.rint(a)) and np.array_equal(R.bf16_round(a), a), what


@pytest.mark.parametrize("case", F.BN_CASES, ids=R.gcase_id)
def test_bn_exact_data_is_exact(case):
    d = F.bn_data(case, "exact")
    ref = F.bn_reference(case, d)
    _exact_in_bf16(d["gamma"] * d["Y"] + d["beta"], "gamma Y + beta")
    for k in ("dy", "x", "raw", "dz"):
        _exact_in_bf16(ref[k], k)
    assert (np.abs(ref["dy"]) @ np.abs(d["W"]).T).max() <= 256
    assert ref["zeros"] > 0 and not ref["dz"][~ref["gate"]].any() and ref["flagged"] == 0.0
    dz, Yp = np.abs(ref["dz"]), np.abs(d["Yp"])
    assert dz.sum(1).max() < 2 ** 24 and (dz * Yp).sum(1).max() < 2 ** 24
    assert (np.abs(d["mean"]) * dz.sum(1)).max() < 2 ** 24 and set(np.unique(d["rstd"])) <= {0.5, 1.0, 2.0}
    M = F.B * case.N
    assert (np.abs(ref["dy"]).reshape(M, -1).T @ np.abs(ref["x"]).reshape(M, -1)).max() < 2 ** 24
    assert np.array_equal(ref["dW"], np.rint(ref["dW"])) and np.abs(ref["dW"]).max() > 0
    if case.cls == "seg4":                            # es keep_scale and et keep_scale are formed first
        _exact_in_bf16(d["es"] * d["keep_scale"], "es ks")
        _exact_in_bf16(d["et"] * d["keep_scale"], "et ks")


@pytest.mark.parametrize("case", F.FOLDED_CASES, ids=F.fcase_id)
def test_folded_exact_data_is_exact(case):
    d = F.folded_data(case, "exact")
    F.folded_exactness(d, F.folded_ref(d))
    assert not np.array_equal(d["H"], d["H"].T)


@pytest.mark.parametrize("case", F.CAT_CASES, ids=F.ccase_id)
def test_cat_exact_data_is_exact(case):
    d = F.cat_data(case, "exact")
    ref = F.cat_reference(case, d)
    for k in ("dy", "raw", "dz"):
        _exact_in_bf16(ref[k], k)
    assert set(np.unique(d["W"])) <= {-1.0, 0.0, 1.0}
    assert (np.abs(ref["dy"]) @ np.abs(d["W"]).T + np.abs(d["bias"])).max() <= 256
    assert ref["zeros"] > 0 and not ref["dz"][~ref["gate"]].any() and ref["flagged"] == 0.0
    dz = np.abs(ref["dz"])
    assert dz.sum(1).max() < 2 ** 24
    if d["rstd"] is not None:
        terms = dz * np.abs(d["Yp"] - d["mean"]) * d["rstd"]               # multiples of 1/2
        assert np.array_equal(2 * terms, np.rint(2 * terms)) and (2 * terms).sum(1).max() < 2 ** 24
        assert (dz * np.abs(d["Yp"])).sum(1).max() < 2 ** 24 and (np.abs(d["mean"]) * dz.sum(1)).max() < 2 ** 24


@pytest.mark.parametrize("case", F.WC5_CASES, ids=R.wcase_id)
def test_wgrad_c5_exact_data_is_exact(case):
    d = R.wgrad_data(case, "exact")
    ref = R.wgrad_reference(case, d)
    _exact_in_bf16(ref["dy"], "dy")
    _exact_in_bf16(ref["x"], "x")
    M = F.B * case.N
    assert (np.abs(ref["dy"]).reshape(M, -1).T @ np.abs(ref["x"]).reshape(M, -1)).max() < 2 ** 24
    assert ref["flagged"] == 0.0 and np.abs(ref["dW"]).max() > 0


@pytest.mark.parametrize("case", F.FOLD_CASES, ids=F.foldcase_id)
def test_fold_exact_data_is_exact(case):
    d = F.fold_data(case, "exact")
    ref = F.fold_ref(case, d)
    W = np.abs(d["W"][:, :case.Cin])
    assert (W.T @ (np.abs(d["gamma"])[:, None] * W)).max() < 128 and (np.abs(d["beta"]) @ W).max() < 2 ** 24
    for k in ("WsT", "H", "c"):                       # multiples of 1/4 below 128: exact in bf16 and fp32
        assert np.array_equal(4 * ref[k], np.rint(4 * ref[k])) and np.array_equal(R.bf16_round(ref[k]), ref[k]), k
    assert ref["flagged"] == 0.0


def test_every_dgrad_case_has_zeros_in_its_gate():
    for kind in F.KINDS:
        for case in F.BN_CASES:
            d = F.bn_data(case, kind)
            z = d["Yp"] * d["es"] + d["et"]
            assert (z == 0).any(), (case, kind)
        for case in F.CAT_CASES:
            d = F.cat_data(case, kind)
            z = d["Yp"] * d["es"] + d["et"]
            assert (z == 0).any(), (case, kind)
