"""fp64 restatements of the fused and folded backward kernels, from their descriptions in
include/pcs.h (not a test module), on top of tests/bwd_refs.py:

  pcs_dgrad_wgrad_bn      dgrad_wgrad_bn_kernel<64,64>, <128,64> (plain, mask, addend) and fused_seg4
                          at 256x512 / 128x256 (plain, mask): dz, S1, S2 = bwd_refs.dgrad_ref, dW =
                          bwd_refs.wgrad_ref with X = Yp, s = es, t = et, keep = c_mask;
  pcs_dgrad_wgrad_folded  seg_conv1's local half: folded_ref below;
  pcs_gemm PCS_PRO_CAT    conv5's folded input gradient (fused_c5, and the generic kernel in f32 and
                          bf16): bwd_refs.dgrad_from on the concatenated staged operand;
  pcs_wgrad (RAW, BNRELU) at Cin = 128 (wgrad_c5 and, with PCS_FLAG_GENERIC, wgrad_kernel): wgrad_ref;
  pcs_bn_fold             fold_ref below.

tests/test_fused_bwd_refs.py proves them against torch autograd in fp64 and shows that the bounds
reject perturbed references; tests/test_gpu_fused_bwd_direct.py compares the kernels with them.
The case lists both files walk are here.  B = 3 scenes (one folded case has 16).

Bounds, element-wise, first order in 2^-24 with bwd_refs.SLACK for the higher orders, none tuned on
GPU output.  Those of dz / S1 / S2 / dW of the PRO_BWD and PRO_CAT kernels are bwd_refs' (its
docstring); fused_seg4 multiplies es and et by keep_scale first (x_operand's folded form).  The
fused kernels (fused_bwd, fused_seg4, fused_c5) keep the accumulator in fp32 up to the store, so
dgrad_from's 2^-8 |acc| term for a bf16 pass through LDS is left out for them (lds_round = False):
their dz carries the one rounding of the store.  What is new:

  folded dX   v = [dz | x] [WaT | H]^T + cvec[b] is one fp32 accumulation of K = 576 products on an
              accumulator that starts at cvec[b]: sum_bound(577, |dz| |WaT|^T + |x| |H|^T + |cvec|),
              plus x's staging error through |H|, plus cvec's own error, a chain of 512 fma whose
              terms fma(gamma, sbias, beta) are rounded once: sum_bound(514, (|gamma sbias| +
              |beta|)^T |W|); then one rounding to bf16, 2^-8 (|v| + the above).  H's row c is
              output column c (as every W [Ncols, K] of pcs_gemm), which for the symmetric H of
              pcs_bn_fold is the header's x H;
  folded dW   fma(alpha, R, fma(beta, S, gamma (W G + sum_b sbias[b] S_b))) from fp32 sums over
              the slices: R = dz^T x and G = x^T x over all M rows (sum_bound(M + 1, .) whatever
              the slicing, plus x's staging error), S_b over the N rows of a scene, S over the B
              scenes, W G a chain of 64 fma, sum_b a chain of B, and four roundings of the final
              expression, each at most U times the sum T of the absolute terms;
  pcs_bn_fold WsT = fl(W alpha) (one rounding), c a sum of Cout fma in four parts (Cout + 3), H a
              chain of Cout fma on terms fl(W gamma) (Cout + 1); in bf16 WsT and H are one rounding
              of that fp32 value (bwd_refs' midpoint flags), c stays fp32.
"""
from collections import namedtuple

import numpy as np

import bwd_refs as R
from bwd_refs import (B, BF16_U, EPI_DGRAD, PRO_BNRELU, PRO_BWD, PRO_RAW, SLACK, U, ZGAP, GCase, WCase,  # noqa: F401
                      assert_within, bf16_parts, bf16_round, dgrad_from, dy_operand, f64, pack_bits, sum_bound,
                      wgrad_ref, x_operand)

KINDS = ("exact", "value")


# ---------------------------------------------------------------------------------------
# route.h's split formula (split_rows), restated
# ---------------------------------------------------------------------------------------
def split_rows(target, scenes, ncb, rows, step, min_steps, fixed=0):
    """(splits, rows per split, non-empty splits) of route::split_rows."""
    sps = fixed if fixed > 0 else -(-target // (scenes * ncb))
    sps = max(1, min(sps, -(-rows // (min_steps * step))))
    rps = -(-(-(-rows // sps)) // step) * step
    return sps, rps, -(-rows // rps)


def slices(N, rps, n):
    """[lo, hi) of n slices of rps rows over a scene of N rows (trailing ones may be empty)."""
    return [(min(i * rps, N), min((i + 1) * rps, N)) for i in range(n)]


def _stored(a, dtype):
    return f64(np.asarray(a, np.float32)) if dtype == "f32" else bf16_round(a)


def _f32(a):
    return f64(np.asarray(a, np.float32))


def _rng(case, kind):
    return np.random.default_rng([int(x) if not isinstance(x, str) else sum(map(ord, x)) for x in case]
                                 + [kind == "exact", 77])


def _sign(r, n):
    return np.where(r.random(n) < 0.25, -1.0, 1.0)


def gapped(r, Y, s, t, dt, zero_rate=0.05):
    """Y (as stored) changed so that Y s + t is exactly 0 in places (Y = 0 in columns whose t is 0:
    every 16th; t is changed in place) and at least ZGAP away from 0 everywhere else."""
    t[::16] = 0.0
    z = Y * s + t
    Y = np.where(np.abs(z) < ZGAP, _stored((np.where(z >= 0, 0.05, -0.05) - t) / s, dt), Y)
    Y[..., ::16] = np.where(r.random(Y[..., ::16].shape) < zero_rate, 0.0, Y[..., ::16])
    Y[:, 0, ::16] = 0.0                       # every scene's first row: zeros also at N = 1
    z = Y * s + t
    assert (np.abs(z[z != 0]) >= ZGAP).all() and (z == 0).any()
    return Y


# ---------------------------------------------------------------------------------------
# pcs_dgrad_wgrad_bn
# ---------------------------------------------------------------------------------------
# cls: "bn64" / "bn128" (dgrad_wgrad_bn_kernel<64,64> / <128,64>, 64-row steps) and "seg4"
# (fused_seg4, 16-row steps); K = Cout, Ncols = Cin as in the pcs_gemm arguments
BN_SHAPES = {"bn64": [(64, 64)], "bn128": [(128, 64)], "seg4": [(256, 512), (128, 256)]}
BN_N = {"bn64": (1, 63, 64, 65, 257), "bn128": (1, 63, 64, 65, 257), "seg4": (1, 15, 16, 17, 48, 64, 129)}


def _bn_cases():
    out = []
    for cls, shapes in BN_SHAPES.items():
        for K, Nc in shapes:
            for v in ("plain", "cmask") + (("addend",) if cls != "seg4" else ()):
                out += [GCase(cls, K, Nc, EPI_DGRAD, v, n, 0) for n in BN_N[cls]]
    return out


BN_CASES = _bn_cases()


def bn_geometry(case):
    """(chunks per scene, rows per chunk) of route::bn_route."""
    if case.cls == "seg4":
        _, rps, cnt = split_rows(256, B, case.Ncols // 256, case.N, 16, 8)
    else:
        _, rps, cnt = split_rows(512 if case.K == 64 else 256, B, 1, case.N, 64, 4)
    return cnt, rps


def bn_data(case, kind):
    return R.gemm_data(case, kind)


def bn_reference(case, d, ge=False, row_weight=None):
    """dz, S1, S2 (dgrad_ref) and dW (wgrad_ref on X = Yp, s = es, t = et, keep = c_mask)."""
    out = R.gemm_reference(case, d, ge=ge, row_weight=row_weight, lds_round=False)
    w = wgrad_ref(d["dZ"], d["Y"], d["alpha"], d["beta"], d["gamma"], d["Yp"], d["es"], d["et"], d["keep"],
                  d["keep_scale"], PRO_BWD, PRO_BNRELU, "bf16", row_weight=row_weight, folded=case.cls == "seg4")
    out.update(dW=w["dW"], e_dW=w["bound"], x=w["x"], flagged=max(out["flagged"], w["flagged"]))
    return out


# ---------------------------------------------------------------------------------------
# pcs_dgrad_wgrad_folded
# ---------------------------------------------------------------------------------------
FCase = namedtuple("FCase", "cls B N")
F_COUT, F_CIN, F_LDW = 512, 64, 1088
# (16, 4097): 16 slices per scene of 320 rows, of which the last three are empty
FOLDED_CASES = [FCase("folded", B, n) for n in (1, 63, 64, 65, 256, 257)] + [FCase("folded", 16, 4097)]


def fcase_id(c):
    return f"folded-B{c.B}-N{c.N}"


def folded_geometry(case):
    """(slices per scene, rows per slice) of fused_bwd.hip's splits_of."""
    sps = max(1, min(-(-256 // case.B), -(-case.N // 256)))
    return sps, -(-(-(-case.N // sps)) // 64) * 64


def folded_data(case, kind):
    """dz [B, N, 512], X [B, N, 64], s, t, alpha, beta, gamma, W [512, 1088] (fp32; the kernel reads
    columns 0..63), sbias [B, 512], and the folded operands WaT [64, 512], H [64, 64] as bf16 values
    built here: WaT = (diag(alpha) W)^T, H = W^T diag(gamma) W plus an antisymmetric part, so that
    a kernel reading H transposed is wrong.  Exact data: one +-1 per row of W (eight per column),
    integers everywhere, every sum below 2^24 (asserted by folded_ref)."""
    r = _rng(case, kind)
    Bc, N = case.B, case.N
    W = np.zeros((F_COUT, F_LDW))
    if kind == "exact":
        col = r.permutation(np.repeat(np.arange(F_CIN), F_COUT // F_CIN))
        W[np.arange(F_COUT), col] = r.choice([-1.0, 1.0], F_COUT)
        W[:, F_CIN:] = 1.0 * r.integers(-3, 4, (F_COUT, F_LDW - F_CIN))
        E = np.triu(1.0 * (r.random((F_CIN, F_CIN)) < 0.05), 1)
        d = dict(dZ=1.0 * r.integers(-2, 3, (Bc, N, F_COUT)), X=1.0 * r.integers(-3, 4, (Bc, N, F_CIN)),
                 s=np.ones(F_CIN), t=1.0 * r.integers(-2, 3, F_CIN), alpha=r.choice([1.0, -1.0, 2.0, -2.0], F_COUT),
                 beta=1.0 * r.integers(-2, 3, F_COUT), gamma=r.choice([0.0, 1.0, -1.0], F_COUT),
                 sbias=1.0 * r.integers(-2, 3, (Bc, F_COUT)))
    else:
        s = _f32(r.uniform(0.5, 1.5, F_CIN) * _sign(r, F_CIN))
        t = _f32(0.3 * r.standard_normal(F_CIN))
        # scenes of different scale, so that S_b (and sbias's share of dW) differs between scenes by
        # more than the bound of a sum over all M rows
        scale = np.linspace(0.4, 1.6, Bc)[r.permutation(Bc)][:, None, None]
        X = gapped(r, bf16_round(scale * r.standard_normal((Bc, N, F_CIN))), s, t, "bf16")
        W[:, :F_CIN] = bf16_round(r.standard_normal((F_COUT, F_CIN)) / 8.0)
        W[:, F_CIN:] = _f32(r.standard_normal((F_COUT, F_LDW - F_CIN)))
        E = np.triu(0.05 * r.standard_normal((F_CIN, F_CIN)), 1)
        d = dict(dZ=bf16_round(0.1 * r.standard_normal((Bc, N, F_COUT))), X=X, s=s, t=t,
                 alpha=_f32(r.uniform(0.5, 1.5, F_COUT) * _sign(r, F_COUT)), beta=_f32(0.05 * r.standard_normal(F_COUT)),
                 gamma=_f32(0.1 * r.standard_normal(F_COUT)), sbias=_f32(0.5 * r.standard_normal((Bc, F_COUT))))
    Wl = W[:, :F_CIN]
    d.update(W=W, WaT=bf16_round((d["alpha"][:, None] * Wl).T), H=bf16_round(Wl.T @ (d["gamma"][:, None] * Wl) + E - E.T))
    return d


def folded_ref(d, dtype="bf16", WaT=None, H=None, cvec_shift=0, sb_shift=0, ge=False, row_weight=None, geometry=None):
    """The header's folded formula in fp64 on the operands as passed (x staged to dtype):
        dX[b, n] = dz WaT^T + x H^T + cvec[b],        cvec[b] = W^T (beta + gamma sbias[b])
        dW       = diag(alpha) R + beta (x) S + diag(gamma) (W G + sum_b sbias[b] (x) S_b)
    with R = dz^T x, G = x^T x, S_b the column sums of x over scene b.  WaT / H default to the data's.
    Perturbed references of the sensitivity tests only: cvec_shift rolls the scenes of cvec,
    sb_shift those of S_b in the sbias term, ge opens the ReLU at 0 (x = 1 there), row_weight
    [B, N] weighs the rows of R, G and S_b.  geometry = (slices per scene, rows per slice): also the
    per-slice partials slab_R / slab_G / slab_S [B * slices, ...] the kernel leaves in its workspace
    (sums over a slice's rows only, so one row more or less shows even where M is large)."""
    dZ, Wl = f64(d["dZ"]), f64(d["W"])[:, :F_CIN]
    WaT = f64(d["WaT"] if WaT is None else WaT)
    H = f64(d["H"] if H is None else H)
    al, be, ga, sb = f64(d["alpha"]), f64(d["beta"]), f64(d["gamma"]), f64(d["sbias"])
    Bc, N, _ = dZ.shape
    M = Bc * N
    xo = x_operand(d["X"], d["s"], d["t"], None, 1.0, PRO_BNRELU, dtype)
    x, xe = xo["v"], xo["err"]
    if ge:
        x = np.where(f64(d["X"]) * f64(d["s"]) + f64(d["t"]) == 0, 1.0, x)
    # input gradient
    cv = (be + ga * sb) @ Wl
    e_cv = sum_bound(F_COUT + 2, (np.abs(be) + np.abs(ga * sb)) @ np.abs(Wl)) * SLACK
    cvu, e_cvu = np.roll(cv, cvec_shift, 0)[:, None], np.roll(e_cv, cvec_shift, 0)[:, None]
    v = dZ @ WaT.T + x @ H.T + cvu
    e_v = (sum_bound(F_COUT + F_CIN + 1, np.abs(dZ) @ np.abs(WaT).T + np.abs(x) @ np.abs(H).T + np.abs(cvu)) * SLACK
           + xe @ np.abs(H).T + e_cvu)
    out = dict(dX=v, e_dX=e_v + (BF16_U * (np.abs(v) + e_v) if dtype != "f32" else 0.0), x=x, cvec=cv,
               flagged=float(xo["flag"].mean()), zeros=int((xo["v"] == 0).sum()))
    # weight gradient
    w = np.ones((Bc, N)) if row_weight is None else f64(row_weight)
    xw, xew = x * w[..., None], xe * w[..., None]
    x2, xw2, xe2, dz2 = x.reshape(M, -1), xw.reshape(M, -1), xew.reshape(M, -1), dZ.reshape(M, -1)
    Rm, Gm, Sb = dz2.T @ xw2, x2.T @ xw2, xw.sum(1)
    e_R = sum_bound(M + 1, np.abs(dz2).T @ np.abs(xw2)) * SLACK + np.abs(dz2).T @ xe2
    e_G = (sum_bound(M + 1, np.abs(x2).T @ np.abs(xw2)) + np.abs(x2).T @ xe2 + xe2.T @ np.abs(x2)) * SLACK
    e_Sb = sum_bound(N + 1, np.abs(xw).sum(1)) * SLACK + xew.sum(1)
    S, aS = Sb.sum(0), np.abs(Sb).sum(0)
    e_S = e_Sb.sum(0) + sum_bound(Bc, aS) * SLACK
    Sbs = np.roll(Sb, sb_shift, 0)
    wg, a_wg = Wl @ Gm, np.abs(Wl) @ np.abs(Gm)
    e_wg = sum_bound(F_CIN + 1, a_wg) * SLACK + np.abs(Wl) @ e_G
    sbs, a_sbs = sb.T @ Sbs, np.abs(sb).T @ np.abs(Sbs)
    e_sbs = sum_bound(Bc + 1, a_sbs) * SLACK + np.abs(sb).T @ np.roll(e_Sb, sb_shift, 0)
    A, Bt, G_ = np.abs(al)[:, None], np.abs(be)[:, None], np.abs(ga)[:, None]
    dW = al[:, None] * Rm + be[:, None] * S + ga[:, None] * (wg + sbs)
    T = A * np.abs(Rm) + Bt * aS + G_ * (a_wg + a_sbs)
    out.update(dW=dW, e_dW=A * e_R + Bt * e_S + G_ * (e_wg + e_sbs) + 4.0 * U * T * SLACK, R=Rm, G=Gm, Sb=Sb, T=T,
               absR=np.abs(dz2).T @ np.abs(x2), absG=np.abs(x2).T @ np.abs(x2), a_wg=a_wg, e_cvec=e_cv, e_Sb=e_Sb)
    if geometry is not None:
        sps, rps = geometry
        sl = {k: [] for k in ("slab_R", "e_slab_R", "slab_G", "e_slab_G", "slab_S", "e_slab_S")}
        for b in range(Bc):
            for lo, hi in slices(N, rps, sps):
                z, xs, xws, es = dZ[b, lo:hi], x[b, lo:hi], xw[b, lo:hi], xew[b, lo:hi]
                n1 = hi - lo + 1
                sl["slab_R"].append(z.T @ xws)
                sl["e_slab_R"].append(sum_bound(n1, np.abs(z).T @ np.abs(xws)) * SLACK + np.abs(z).T @ es)
                sl["slab_G"].append(xs.T @ xws)
                sl["e_slab_G"].append((sum_bound(n1, np.abs(xs).T @ np.abs(xws)) + np.abs(xs).T @ es + es.T @ np.abs(xs)) * SLACK)
                sl["slab_S"].append(xws.sum(0))
                sl["e_slab_S"].append(sum_bound(n1, np.abs(xws).sum(0)) * SLACK + es.sum(0))
        out.update({k: np.stack(v) for k, v in sl.items()})
    return out


def folded_exactness(d, ref):
    """The conditions under which a correct kernel reproduces folded_ref bit for bit: every stored
    bf16 value an integer of magnitude <= 256, every partial sum below 2^24."""
    def ints(a, lim, what):
        a = f64(a)
        assert np.array_equal(a, np.rint(a)) and np.abs(a).max() <= lim, what
    for k in ("dZ", "WaT", "H"):
        ints(d[k], 256, k)
    for k in ("alpha", "beta", "gamma", "sbias"):
        ints(d[k], 256, k)
    ints(d["W"][:, :F_CIN], 1, "W")
    ints(ref["x"], 256, "x")
    ints(ref["dX"], 256, "dX")
    ints(ref["cvec"], 2 ** 24, "cvec")
    dZ = f64(d["dZ"])
    part = (np.abs(dZ) @ np.abs(f64(d["WaT"])).T + np.abs(ref["x"]) @ np.abs(f64(d["H"])).T
            + np.abs(ref["cvec"])[:, None])
    assert part.max() <= 256, "dX partial sums"
    assert max(ref["absR"].max(), ref["absG"].max(), ref["a_wg"].max(), ref["T"].max()) < 2 ** 24, "dW partial sums"
    assert ref["flagged"] == 0.0 and np.abs(ref["dW"]).max() > 0


# ---------------------------------------------------------------------------------------
# pcs_gemm, PCS_PRO_CAT / PCS_EPI_DGRAD
# ---------------------------------------------------------------------------------------
# cls: "c5" (fused_c5: bf16, default flags), "catg" (gemm_nt_kernel<bf16_t>, PCS_FLAG_GENERIC), "catf" (fp32)
CCase = namedtuple("CCase", "cls K1 K2 Ncols variant N cps")


def ccase_id(c):
    return f"{c.cls}-K{c.K1}+{c.K2}xN{c.Ncols}-{c.variant}-N{c.N}-cps{c.cps}"


def cdtype(case):
    return "f32" if case.cls == "catf" else "bf16"


def _cat_cases():
    out = []
    for v in ("plain", "norstd"):
        out += [CCase("c5", 1024, 128, 128, v, n, 0) for n in (1, 31, 32, 33, 127, 128, 129, 2 * 128 + 5)]
        out.append(CCase("c5", 1024, 128, 128, v, 2 * 128 + 5, 2))
    for cls in ("catg", "catf"):
        for K1 in (32, 64):
            for K2 in (32, 64):
                for Nc in (64, 128):
                    out += [CCase(cls, K1, K2, Nc, v, 133, 0) for v in ("plain", "cmask_addend")]
        out += [CCase(cls, 64, 64, 64, v, 133, 0) for v in ("cmask", "addend", "norstd")]
        out += [CCase(cls, 64, 64, 64, "cmask", n, 0) for n in (1, 127, 128, 129, 2 * 128 + 5)]
        out.append(CCase(cls, 64, 64, 64, "cmask", 2 * 128 + 5, 2))
    return out


CAT_CASES = _cat_cases()


def cat_geometry(case):
    """(chunks per scene, rows per chunk) of route::gemm_class for these shapes (128-row tile)."""
    if case.cls == "c5":
        _, rps, cnt = split_rows(256, B, 1, case.N, 128, 1, case.cps)
    else:
        _, rps, cnt = split_rows(2048, B, max(case.Ncols // 128, 1), case.N, 128, 1, case.cps)
    return cnt, rps


def cat_data(case, kind):
    """dz [B, N, K1] (A), y [B, N, K2] (A2: through pa / pb), W = [Ws | H] [Ncols, K1 + K2], bias,
    Yp with es / et, mean / rstd, addend, keep.  The fused_c5 kernel needs Yp = A2 (conv5: both
    are y4), so there Yp is y; elsewhere Yp is a tensor of its own.  pa / pb differ from es / et.
    Exact data: eight +-1 per row of W (five in Ws, three in H), |dz| <= 2, x <= 8: |acc| <= 40,
    |bias| <= 4, |addend| <= 32, keep_scale 2: |dz'| <= 152."""
    r = _rng(case, kind)
    dt = cdtype(case)
    N, K1, K2, Nc = case.N, case.K1, case.K2, case.Ncols
    own = case.cls != "c5"
    if kind == "exact":
        W = np.zeros((Nc, K1 + K2))
        for n in range(Nc):
            W[n, r.choice(K1, 5, replace=False)] = r.choice([-1.0, 1.0], 5)
            W[n, K1 + r.choice(K2, 3, replace=False)] = r.choice([-1.0, 1.0], 3)
        y = 1.0 * r.integers(-3, 4, (B, N, K2))
        d = dict(dZ=1.0 * r.integers(-2, 3, (B, N, K1)), y=y, pa=r.choice([1.0, -1.0, 2.0], K2),
                 pb=1.0 * r.integers(-2, 3, K2), W=W, bias=1.0 * r.integers(-4, 5, Nc),
                 Yp=1.0 * r.integers(-4, 5, (B, N, Nc)) if own else y, es=r.choice([1.0, -1.0, 2.0], Nc),
                 et=1.0 * r.integers(-2, 3, Nc), mean=1.0 * r.integers(-2, 3, Nc), rstd=r.choice([0.5, 1.0, 2.0], Nc),
                 addend=1.0 * r.integers(-32, 33, (B, N, Nc)), keep=r.random((B, N, Nc)) < 0.5, keep_scale=2.0)
    else:
        es = _f32(r.uniform(0.5, 1.5, Nc) * _sign(r, Nc))
        et = _f32(0.5 * r.standard_normal(Nc))
        Yp = gapped(r, _stored(r.standard_normal((B, N, Nc)), dt), es, et, dt)
        y = _stored(r.standard_normal((B, N, K2)), dt) if own else Yp
        K = K1 + K2
        d = dict(dZ=_stored(0.1 * r.standard_normal((B, N, K1)), dt), y=y,
                 pa=_f32(r.uniform(0.5, 1.5, K2) * _sign(r, K2)), pb=_f32(0.3 * r.standard_normal(K2)),
                 W=_stored(r.standard_normal((Nc, K)) * np.r_[np.full(K1, 1.0 / np.sqrt(K)), np.full(K2, 0.1 / np.sqrt(K2))], dt),
                 bias=_f32(0.2 * r.standard_normal(Nc)), Yp=Yp, es=es, et=et, mean=_f32(0.3 * r.standard_normal(Nc)),
                 rstd=_f32(np.abs(1.0 + 0.1 * r.standard_normal(Nc))),
                 addend=_stored(0.1 * r.standard_normal((B, N, Nc)), dt), keep=r.random((B, N, Nc)) < 0.7,
                 keep_scale=float(np.float32(1.0 / 0.7)))
    v = case.variant
    if v not in ("cmask", "cmask_addend"):
        d["keep"], d["keep_scale"] = None, 1.0
    if v not in ("addend", "cmask_addend"):
        d["addend"] = None
    if v == "norstd":
        d["mean"] = d["rstd"] = None
    return d


def cat_reference(case, d, ge=False, row_weight=None, x_ge=False):
    """dgrad_from on [dz | x_operand(y, pa, pb)] with W = [Ws | H] and bias.  x_ge (a perturbed
    reference): the prologue's ReLU open at 0 (x = 1 there)."""
    dt = cdtype(case)
    xo = x_operand(d["y"], d["pa"], d["pb"], None, 1.0, PRO_BNRELU, dt)
    xv = xo["v"]
    if x_ge:
        xv = np.where(f64(d["y"]) * f64(d["pa"]) + f64(d["pb"]) == 0, 1.0, xv)
    dz = f64(d["dZ"])
    op = dict(v=np.concatenate([dz, xv], -1), err=np.concatenate([np.zeros_like(dz), xo["err"]], -1),
              flag=np.concatenate([np.zeros(dz.shape, bool), xo["flag"]], -1))
    out = dgrad_from(op, d["W"], d["addend"], d["Yp"], d["es"], d["et"], d["keep"], d["keep_scale"], d["mean"],
                     d["rstd"], dt, bias=d["bias"], ge=ge, row_weight=row_weight, lds_round=case.cls != "c5")
    out["flagged"] = float(xo["flag"].mean())
    return out


# ---------------------------------------------------------------------------------------
# pcs_wgrad (RAW, BNRELU), Cin = 128
# ---------------------------------------------------------------------------------------
# cls: "c5" (wgrad_c5_kernel: 32-row steps, slices of 64-row multiples) and "c5g" (the same calls
# with PCS_FLAG_GENERIC: wgrad_kernel<bf16_t>)
def _wc5_cases():
    out = []
    for cls in ("c5", "c5g"):
        for Cout in (256, 512):
            out += [WCase(cls, Cout, 128, PRO_RAW, PRO_BNRELU, False, n, 0, 0) for n in (1, 31, 32, 33, 63, 64, 65, 129)]
            out.append(WCase(cls, Cout, 128, PRO_RAW, PRO_BNRELU, False, 6 * 64 + 3, 3, 0))   # 192, 192, 3 rows
    # four caller-set slices of 64 rows over 130: the fourth starts past the scene's end
    out += [WCase("c5", Cout, 128, PRO_RAW, PRO_BNRELU, False, 130, 4, 0) for Cout in (256, 512)]
    return out


WC5_CASES = _wc5_cases()


def wc5_geometry(case):
    """(slices per scene, rows per slice) of route::wgrad_route."""
    if case.sps:
        sps = case.sps
    elif case.cls == "c5":
        sps = split_rows(512, B, case.Cout // 256, case.N, 32, 4)[0]
    else:
        sps = split_rows(1024, B, (case.Cout // 128) * (case.Cin // 128), case.N, 64, 4)[0]
    return sps, -(-(-(-case.N // sps)) // 64) * 64


# ---------------------------------------------------------------------------------------
# pcs_bn_fold
# ---------------------------------------------------------------------------------------
FoldCase = namedtuple("FoldCase", "dtype Cout Cin ldw variant")      # variant: full | nowst | noc
FOLD_CASES = [FoldCase(dt, *sh, v) for dt in ("f32", "bf16") for sh in ((512, 64, 1088), (1024, 128, 128), (64, 64, 64))
              for v in ("full", "nowst", "noc")]


def foldcase_id(c):
    return f"{c.dtype}-{c.Cout}x{c.Cin}-ldw{c.ldw}-{c.variant}"


def fold_data(case, kind):
    r = np.random.default_rng([sum(map(ord, case.dtype + case.variant)), case.Cout, case.Cin, kind == "exact"])
    Co, Ci = case.Cout, case.Cin
    W = np.zeros((Co, case.ldw))
    if kind == "exact":      # sparse +-1 / +-2 rows, small integer coefficients: every value an integer <= 256
        for k in range(Co):
            W[k, r.choice(Ci, 2, replace=False)] = r.choice([-2.0, -1.0, 1.0, 2.0], 2)
        W[:, Ci:] = 7.0
        return dict(W=W, alpha=r.choice([1.0, -1.0, 2.0, -2.0, 0.5], Co), beta=1.0 * r.integers(-2, 3, Co),
                    gamma=r.choice([0.0, 1.0, -1.0, 0.5], Co))
    # one sign per row of W and gamma > 0: no term of H cancels, so its fp32 evaluation error stays
    # small against the bf16 spacing and few elements are flagged (WsT and c see both signs)
    W[:, :Ci] = _f32(np.abs(r.standard_normal((Co, Ci))) * _sign(r, Co)[:, None] / np.sqrt(Ci))
    W[:, Ci:] = 7.0
    return dict(W=W, alpha=_f32(r.uniform(0.5, 1.5, Co) * _sign(r, Co)), beta=_f32(0.05 * r.standard_normal(Co)),
                gamma=_f32(0.02 + 0.1 * np.abs(r.standard_normal(Co))))


def fold_ref(case, d):
    """WsT [Cin, Cout] = (diag(alpha) W)^T, c [Cin] = W^T beta, H [Cin, Cin] = W^T diag(gamma) W with
    their bounds e_<name>; the shares of flagged elements of WsT and of H.  H's fp32 value is off by
    up to (Cout + 1) U sum |terms|, which against a bf16 spacing of 2^-8 to 2^-7 relative flags up
    to 2 (Cout + 1) 2^-16 of its elements where no term cancels (3 % at Cout = 1024): these are
    outputs, compared exactly where not flagged, and stay out of the operands' flag cap."""
    W = f64(d["W"])[:, :case.Cin]
    al, be, ga = f64(d["alpha"]), f64(d["beta"]), f64(d["gamma"])
    Co = case.Cout
    ws = (al[:, None] * W).T
    h, ah = W.T @ (ga[:, None] * W), np.abs(W).T @ (np.abs(ga)[:, None] * np.abs(W))
    s_ws = R._stage(ws, U * np.abs(ws), case.dtype)
    s_h = R._stage(h, sum_bound(Co + 1, ah) * SLACK, case.dtype)
    return dict(WsT=s_ws["v"], e_WsT=s_ws["err"], H=s_h["v"], e_H=s_h["err"], c=be @ W,
                e_c=sum_bound(Co + 3, np.abs(be) @ np.abs(W)) * SLACK,
                flagged=float(s_ws["flag"].mean()), flagged_H=float(s_h["flag"].mean()))
