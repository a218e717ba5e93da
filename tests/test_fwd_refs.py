"""CPU proofs of tests/fwd_refs.py, the fp64 restatement test_gpu_fwd_gemm.py holds the forward
pcs_gemm kernels to:

* against torch in fp64: F.conv1d on relu(batch_norm) with an explicit dropout mask, the per-scene
  bias, per-chunk statistics that merge (small_refs.bn_fwd_from_partials) to batch_norm's mean and
  variance, relu(bn(.)) on the way out, max / min over the points with their indices; the
  refactored dgrad_from against autograd of the folded form;
* every exact case is exact;
* the sensitivity of every case of the GPU file: a reference perturbed the way a subtly wrong
  kernel would be differs from the true one by more than both bounds together somewhere (value
  data), or at all (exact data).  Only reference data is perturbed.  What a perturbation cannot
  touch is spelled out in `applicable`, with the reason;
* the share of midpoint-flagged operand elements."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fwd_refs as R
import small_refs as S
from bwd_refs import x_operand, dgrad_from
from test_bwd_refs import rejects, rolled, _exact_in_bf16

KINDS = ["exact", "value"]


@functools.lru_cache(maxsize=None)
def base(case, kind):
    d = R.fwd_data(case, kind)
    return d, R.fwd_reference(case, d)


# ---------------------------------------------------------------------------------------
# torch
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,K,Nc,N,rpc", [(1, 16, 8, 11, 6), (2, 5, 24, 7, 3)])
def test_refs_reproduce_torch(seed, K, Nc, N, rpc):
    B, eps, ks = 3, 1e-5, 1.0 / 0.7
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    y0, W, bias, sb = rn(B, K, N), rn(Nc, K), rn(Nc), rn(B, Nc)
    g0, b0, g1, b1 = rn(K) + 1.5, rn(K), rn(Nc) - 0.2, rn(Nc)         # g1 of both signs
    keep = torch.rand(B, K, N, generator=g) < 0.7
    x = torch.relu(F.batch_norm(y0, None, None, g0, b0, True, 0.1, eps)) * keep * ks
    n = lambda t: t.numpy()   # noqa: E731
    pm = lambda t: n(t).transpose(0, 2, 1)   # noqa: E731   [B, C, N] -> [B, N, C]
    m0, v0 = n(y0).mean((0, 2)), n(y0).var((0, 2))
    s = n(g0) / np.sqrt(v0 + eps)
    t = n(b0) - m0 * s
    op = x_operand(pm(y0), s, t, pm(keep), ks, R.PRO_BNRELU, "f32")
    assert np.abs(op["v"] - pm(x)).max() < 1e-12
    cps = -(-N // rpc)
    for bb, sbb, y in ((None, None, F.conv1d(x, W[:, :, None])), (bias, None, F.conv1d(x, W[:, :, None], bias)),
                       (bias, sb, F.conv1d(x, W[:, :, None]) + sb[:, :, None])):
        nb, nsb = (None if bb is None else n(bb)), (None if sbb is None else n(sbb))
        ref = R.fwd_ref(op, n(W), nb, nsb, None, None, R.EPI_FWD, "f32")
        assert np.abs(ref["C"] - pm(y)).max() < 1e-11
        assert np.abs(R.fwd_ref(op, n(W), nb, nsb, None, None, R.EPI_RAW, "f32")["C"]
                      - pm(F.conv1d(x, W[:, :, None]))).max() < 1e-11
        # chunk statistics -> batch_norm's mean / variance -> relu(bn(y)) on the way out
        st = R.stats_ref(ref["C"], cps, rpc, R.EPI_FWD)
        fin = S.bn_fwd_from_partials(np.stack([st["mean"], st["M2"]], -1), B, N, cps, rpc, n(g1), n(b1), None, None,
                                     None, 0.1, eps)
        assert np.abs(fin["mean"] - n(y).mean((0, 2))).max() < 1e-12
        assert np.abs(fin["rstd"] - 1.0 / np.sqrt(n(y).var((0, 2)) + eps)).max() < 1e-10
        a = torch.relu(F.batch_norm(y, None, None, g1, b1, True, 0.1, eps))
        out = R.fwd_ref(op, n(W), nb, nsb, fin["scale"], fin["shift"], R.EPI_BNRELU, "f32")
        assert np.abs(out["C"] - pm(a)).max() < 1e-10
        cs = R.stats_ref(out["C"], cps, rpc, R.EPI_BNRELU)
        assert np.abs(cs["mean"].reshape(B, cps, Nc).sum(1) - n(a).sum(2)).max() < 1e-10 and not cs["M2"].any()
        # max-pool: chunk records -> the scene's max (scale > 0) or min (scale < 0) and its row
        pf = S.pool_finalize_ref(R.pool_ref(ref["C"], cps, rpc), B, N, cps, fin["scale"], fin["shift"])
        y32 = torch.from_numpy(np.asarray(ref["C"], np.float32).transpose(0, 2, 1).copy())
        mx, mn = y32.max(2), y32.min(2)
        pos = fin["scale"] > 0
        assert np.array_equal(pf["ysel"], np.where(pos, n(mx.values), n(mn.values)))
        assert np.array_equal(pf["am"] - (np.arange(B) * N)[:, None], np.where(pos, n(mx.indices), n(mn.indices)))


@pytest.mark.parametrize("seed", [1, 2])
def test_dgrad_from_reproduces_autograd_of_the_folded_form(seed):
    """dz is the gradient at o = gamma (Yp - mean) rstd + beta of sum(relu(o) keep keep_scale v) with
    v = x H^T + bias + addend held constant; S1 and S2 are its gradients at beta and gamma."""
    B, N, K, Nc, ks = 3, 9, 12, 8, 2.0
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    A, s, t, H, bias, add, Yp = rn(B, N, K), rn(K), rn(K), rn(Nc, K), rn(Nc), rn(B, N, Nc), rn(B, N, Nc)
    gamma, beta = (rn(Nc) + 0.3).requires_grad_(), rn(Nc).requires_grad_()
    mean, rstd = rn(Nc), rn(Nc).abs() + 0.5
    keep = torch.rand(B, N, Nc, generator=g) < 0.6
    v = torch.relu(A * s + t) @ H.T + bias + add
    o = gamma * (Yp - mean) * rstd + beta
    o.retain_grad()
    (torch.relu(o) * keep * ks * v).sum().backward()
    n = lambda x: x.detach().numpy()   # noqa: E731
    es = n(gamma * rstd)
    et = n(beta) - n(mean) * es
    op = x_operand(n(A), n(s), n(t), None, 1.0, R.PRO_BNRELU, "f32")
    d = dgrad_from(op, n(H), n(add), n(Yp), es, et, n(keep), ks, n(mean), n(rstd), "f32", bias=n(bias))
    assert np.abs(d["dz"] - n(o.grad)).max() < 1e-11
    assert np.abs(d["S1"].sum(0) - n(beta.grad)).max() < 1e-10
    assert np.abs(d["S2"].sum(0) - n(gamma.grad)).max() < 1e-10
    raw = dgrad_from(x_operand(n(A), None, None, None, 1.0, R.PRO_RAW, "f32"), n(H), None, None, None, None, None, 1.0,
                     None, None, "f32")
    assert np.abs(raw["raw"] - n(A @ H.T)).max() < 1e-12


def test_geometry_has_no_empty_chunk():
    for case in R.FWD_CASES:
        cps, rpc = R.geometry(case)
        assert rpc % R.tile_of(case) == 0 and (cps - 1) * rpc < case.N <= cps * rpc, case
        assert not case.cps or cps == case.cps, case


def test_every_instantiation_of_the_cases_was_recorded_running():
    """profiles/fwd_gemm_kernels.txt is the sorted list of distinct kernel names of one kernel trace
    of tests/test_gpu_fwd_gemm.py alone: every instantiation the cases are meant to reach ran."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fwd_gemm_kernels.txt")
    with open(path) as f:
        ran = f.read()
    want = {R.kernel_of(c) for c in R.FWD_CASES}
    assert not [k for k in want if k + "(" not in ran]


# ---------------------------------------------------------------------------------------
# exact data
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FWD_CASES, ids=R.case_id)
def test_exact_data_is_exact(case):
    d, ref = base(case, "exact")
    if case.pro == R.PRO_BNRELU:
        assert np.array_equal(d["s"], np.ones_like(d["s"])) and d["keep_scale"] in (1.0, 2.0)
    _exact_in_bf16(ref["x"], "x")
    assert np.abs(ref["x"]).max() <= 12 and set(np.unique(d["W"])) <= {-1.0, 0.0, 1.0}
    assert (np.abs(ref["x"]) @ np.abs(d["W"]).T).max() <= 96          # every partial sum along K is below this
    assert ref["flagged"] == 0.0
    if case.epi == R.EPI_DGRAD:
        _exact_in_bf16(ref["raw"] + (0.0 if d["bias"] is None else d["bias"]), "acc + bias")
        _exact_in_bf16(ref["dz"], "dz")
        assert ref["zeros"] > 0 and not ref["dz"][~ref["gate"]].any() and ref["dz"].any()
        dz = np.abs(ref["dz"])
        assert dz.sum(1).max() < 2 ** 24 and (dz * np.abs(d["Yp"])).sum(1).max() < 2 ** 24
        if d["rstd"] is not None:
            terms = dz * np.abs(d["Yp"] - d["mean"]) * d["rstd"]
            assert np.array_equal(2 * terms, np.rint(2 * terms)) and (2 * terms).sum(1).max() < 2 ** 24
        return
    _exact_in_bf16(ref["C"], "C")
    if case.epi == R.EPI_BNRELU:
        y = R.fwd_ref(R.fwd_operand(case, d), d["W"], d["bias"], None, None, None, R.EPI_FWD, "f32")["C"]
        _exact_in_bf16(y, "y")
        _exact_in_bf16(y * d["es"], "y es")
        assert np.abs(ref["C"]).sum(1).max() < 2 ** 24                   # the column sums are exact
    assert ref["C"].any()


# ---------------------------------------------------------------------------------------
# sensitivity
# ---------------------------------------------------------------------------------------
def differs(kind, ref, pert, names):
    if kind == "value":
        return rejects(ref, pert, names)
    return any(not np.array_equal(ref[nm], pert[nm]) for nm, _ in names)


def bit_reversed(keep):
    """The keep bits with the bit order reversed within every byte."""
    return keep.reshape(*keep.shape[:-1], -1, 8)[..., ::-1].reshape(keep.shape)


def swap_chunk(d, lo):
    es, et = d["es"].copy(), d["et"].copy()
    es[lo:lo + 8], et[lo:lo + 8] = d["et"][lo:lo + 8], d["es"][lo:lo + 8]
    return dict(d, es=es, et=et)


def applicable(case, kind, d):
    """The perturbations that can touch the case.  Left out, with the reason:
      bias for scene_bias      needs a scene_bias;
      mask bits                need dropout bits (a_mask of the prologue, c_mask of EPI_DGRAD);
      rounded before scale     needs bf16 and a_mask; the exact data's keep_scale is 2, a power of
                               two, which commutes with the rounding: value data only;
      ReLU dropped             needs PRO_BNRELU (prologue) or EPI_BNRELU (epilogue);
      s / t rolled             (by one 8-column chunk inside the last 64-wide tile) needs PRO_BNRELU;
                               the exact data's s is 1 throughout: s on value data only;
      es / et swapped          needs es and et in the arithmetic (EPI_BNRELU, or EPI_DGRAD unless
                               `noes`); with the pool only sign(es) is read;
      statistics rows          need statistics; a row cannot be dropped from a one-row chunk, nor
                               doubled in a full last chunk (N = chunks * rows per chunk); in a
                               one-row chunk a doubled row leaves mean and M2 = 0 as they are; the
                               boundary moves only between two chunks;
      last-occurrence argmax   needs the pool and a chunk of more than one row.
    PRO_RAW + EPI_FWD `nostats` is touched by none of them: it is the plain product plus bias."""
    f = R.flags_of(case)
    cps, rpc = R.geometry(case)
    last = case.N - (cps - 1) * rpc                       # rows of the last chunk
    out = []
    if f["scene_bias"]:
        out.append("bias for scene_bias")
    if d["keep"] is not None or d["ckeep"] is not None:
        out += ["mask bit order", "mask shifted by 4"]
    if d["keep"] is not None and R.dtype_of(case) == "bf16" and kind == "value":
        out.append("rounded before scale")
    if case.pro == R.PRO_BNRELU:
        out += ["prologue ReLU dropped", "t rolled"] + (["s rolled"] if kind == "value" else [])
    if case.epi == R.EPI_BNRELU:
        out.append("epilogue ReLU dropped")
    if case.epi in (R.EPI_BNRELU, R.EPI_DGRAD) and d["es"] is not None:
        out.append("es / et swapped")
    if case.epi == R.EPI_DGRAD:
        out += ["S row dropped", "S row doubled"]
    if f["stats"]:
        if last >= 2:
            out.append("row dropped")
        if last < rpc and (last >= 2 or case.epi == R.EPI_BNRELU):
            out.append("row doubled")
        if cps > 1:
            out.append("boundary - 1")
            if last >= 2:
                out.append("boundary + 1")
    if f["pool"] and case.N > 1:
        out.append("last argmax")
    return out


def perturbed(case, kind, name, d, ref):
    """True when the perturbed reference is told apart from ref."""
    dgrad = case.epi == R.EPI_DGRAD
    names = [("dz", "e_dz"), ("S1", "e_S1"), ("S2", "e_S2")] if dgrad else [("C", "e_C")]
    cps, rpc = R.geometry(case)
    dt = R.dtype_of(case)
    ref_of = lambda dd, **kw: differs(kind, ref, R.fwd_reference(case, dd, **kw), names)   # noqa: E731
    if name == "bias for scene_bias":
        return ref_of(dict(d, scene_bias=None))
    if name in ("mask bit order", "mask shifted by 4"):
        k = "keep" if d["keep"] is not None else "ckeep"
        return ref_of(dict(d, **{k: bit_reversed(d[k]) if name == "mask bit order" else np.roll(d[k], 4, axis=-1)}))
    if name == "rounded before scale":
        return ref_of(d, pre_round=True)
    if name == "prologue ReLU dropped":
        return ref_of(d, pro_relu=False)
    if name == "epilogue ReLU dropped":
        return ref_of(d, epi_relu=False)
    if name in ("s rolled", "t rolled"):
        k, width = name[0], min(case.K, 64)
        return ref_of(dict(d, **{k: rolled(d[k], case.K // width - 1, width)}))
    if name == "es / et swapped":
        return ref_of(swap_chunk(d, case.Ncols - 64 + 8))
    if name in ("S row dropped", "S row doubled"):
        w = np.ones((R.B, case.N))
        w[1, case.N - 1] = 0.0 if name == "S row dropped" else 2.0
        return differs(kind, ref, R.fwd_reference(case, d, row_weight=w), names[1:2] if d["rstd"] is None else names[1:])
    C = R.stored(ref["C"], dt)
    if name == "last argmax":
        return not np.array_equal(R.pool_ref(C, cps, rpc).view(np.int32), R.pool_ref(C, cps, rpc, last=True).view(np.int32))
    kw = {"row dropped": dict(row=(case.N - 1, 0)), "row doubled": dict(row=(case.N - 1, 2)),
          "boundary - 1": dict(boundary=-1), "boundary + 1": dict(boundary=1)}[name]
    snames = [("mean", "e_mean"), ("M2", "e_M2")]
    # the statistics' bounds are those of the value test for both kinds of data
    return rejects(R.stats_ref(C, cps, rpc, case.epi), R.stats_ref(C, cps, rpc, case.epi, **kw), snames)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.FWD_CASES, ids=R.case_id)
def test_case_rejects_perturbed_references(case, kind):
    d, ref = base(case, kind)
    todo = applicable(case, kind, d)
    if case.epi == R.EPI_DGRAD:
        assert ref["zmin"] >= (1.0 if kind == "exact" else R.ZGAP) and ref["zeros"] > 0
    missed = [name for name in todo if not perturbed(case, kind, name, d, ref)]
    assert not missed, missed
    if not todo:
        assert (case.pro, case.epi, case.variant) == (R.PRO_RAW, R.EPI_FWD, "nostats"), case


def test_value_data_keeps_both_relus_away_from_zero():
    for case in R.FWD_CASES:
        if case.pro == R.PRO_BNRELU:
            d = base(case, "value")[0]
            z = d["A"] * d["s"] + d["t"]
            assert (z == 0).any() and np.abs(z[z != 0]).min() >= R.ZGAP, case
            assert not d["A"][z == 0].any(), "exact zeros only from A = t = 0"
        if case.epi != R.EPI_DGRAD:
            d = base(case, "value")[0]
            assert not d["W"][case.Ncols - 3].any() and np.abs(d["W"]).sum(1).min() == 0.0
        if case.epi == R.EPI_BNRELU:
            d = base(case, "value")[0]
            z = R.fwd_ref(R.fwd_operand(case, d), d["W"], d["bias"], None, d["es"], d["et"], R.EPI_BNRELU, "f32",
                          epi_relu=False)["C"]
            zc = np.arange(case.Ncols) == case.Ncols - 3
            assert not z[..., zc].any() and np.abs(z[..., ~zc]).min() >= R.ZGAP, case
            assert 0.2 < (z > 0).mean() < 0.8, "the epilogue's ReLU is open and closed about as often"


# ---------------------------------------------------------------------------------------
# midpoint flags
# ---------------------------------------------------------------------------------------
def test_midpoint_flags_are_rare():
    worst = 0.0
    for case in R.FWD_CASES:
        fl = base(case, "value")[1]["flagged"]
        if R.dtype_of(case) == "f32" or case.pro == R.PRO_RAW:
            assert fl == 0.0, case
        else:
            assert fl <= 1e-3, (case, fl)
            worst = max(worst, fl)
    assert worst > 0.0
