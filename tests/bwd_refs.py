"""fp64 restatements of the unfused backward GEMMs, from their descriptions in include/pcs.h (not a
test module): pcs_wgrad with dy_mode PCS_PRO_BWD / PCS_PRO_RAW and pcs_gemm with PCS_PRO_BWD and
PCS_EPI_DGRAD / PCS_EPI_RAW.  tests/test_bwd_refs.py proves them against torch autograd in fp64 on
the CPU; tests/test_gpu_bwd_unfused.py compares the kernels with them.  The case lists both files
walk are here too, so that the CPU file can check the sensitivity of exactly the cases the GPU
file runs.  x_operand and dgrad_from (the EPI_DGRAD / EPI_RAW epilogue on any staged operand, of
which dgrad_ref is the PRO_BWD case) also serve the forward restatement, tests/fwd_refs.py.

Everything is NumPy float64 on arrays shaped [B, N, C] that hold the values as stored (fp32 or
bf16).  For bf16 the references round dy and x to bf16 (round to nearest even, straight from
fp64) where the kernels stage them: after the affine step, after the keep scale.

Bounds (none tuned on GPU output), element-wise, first order in 2^-24 with a 2^-10 relative
slack for the higher orders:

  staged operand, fp32   the roundings that form it: dy = fma(alpha, dZ, fma(gamma, Y, beta)) is
                         off by at most U (|gamma Y + beta| + |dy|), x = relu(fma(X, s, t)) by
                         U |x|, and the keep scale adds another U |x|;
  staged operand, bf16   the kernel rounds its fp32 value, the reference the fp64 one: they agree
                         unless the fp64 value lies within that fp32 evaluation error of a bf16
                         rounding midpoint.  Those elements are flagged and allowed one bf16 ulp;
  dW                     sum_bound over the M rows reduced on |dy|^T |x|, plus the operand errors;
  acc = dy W^T           sum_bound over K on |dy| |W|^T, plus the operand error;
  dz, raw (bf16)         2^-8 |acc| for the accumulator's rounding to bf16 before addend and mask,
                         2^-8 |dz| for the store;
  S1, S2                 sums over a scene of the dz the kernels hold before the store (an fp32
                         value): sum_bound over its N rows plus the summed errors of those dz;
                         S2's terms are |dz| (|Yp| + |mean|) |rstd|, which covers both
                         sum dz (Yp - mean) rstd and rstd (sum dz Yp - mean S1).
"""
from collections import namedtuple

import numpy as np

from small_refs import U, ULP, f64, sum_bound, round_bound, assert_within  # noqa: F401  (re-exported)

PRO_RAW, PRO_BNRELU, PRO_BWD = 0, 1, 2
EPI_DGRAD, EPI_RAW = 1, 2
BF16_U = 2.0 ** -8            # unit roundoff of bf16 (8 significant bits)
SLACK = 1.0 + 2.0 ** -10      # second-order terms of the first-order bounds
ZGAP = 1e-3                   # |es Yp + et| of the value data is 0 exactly or at least this


# ---------------------------------------------------------------------------------------
# bf16
# ---------------------------------------------------------------------------------------
def bf16_parts(v):
    """(r, dist, q): v rounded to bf16 (nearest even, from fp64 in one step), the distance from v
    to the nearest rounding midpoint, and the bf16 spacing q at v (normal range)."""
    v = f64(v)
    _, e = np.frexp(v)                       # |v| = m 2^e with m in [0.5, 1)
    q = np.ldexp(1.0, np.maximum(e, -125) - 8)
    u = v / q
    return np.rint(u) * q, np.abs(u - np.floor(u) - 0.5) * q, q


def bf16_round(v):
    return bf16_parts(v)[0]


def _stage(v, err, dtype):
    """The staged operand of the reference and the bound on |kernel's staged value - it|."""
    if dtype == "f32":
        return dict(v=v, err=err * SLACK, flag=np.zeros(v.shape, bool))
    r, dist, q = bf16_parts(v)
    flag = dist <= err * SLACK
    return dict(v=r, err=np.where(flag, q, 0.0), flag=flag)


def dy_operand(dZ, Y, alpha, beta, gamma, mode, dtype):
    """dy = alpha dZ + beta + gamma Y (PRO_BWD) or dZ as stored (PRO_RAW), as staged."""
    dZ = f64(dZ)
    if mode == PRO_RAW:
        return dict(v=dZ, err=np.zeros_like(dZ), flag=np.zeros(dZ.shape, bool))
    assert mode == PRO_BWD
    a, b, g, Y = f64(alpha), f64(beta), f64(gamma), f64(Y)
    inner = g * Y + b
    v = a * dZ + inner
    return _stage(v, U * (np.abs(inner) + np.abs(v)), dtype)


def x_operand(X, s, t, keep, keep_scale, mode, dtype, folded=False):
    """x = relu(X s + t) keep keep_scale (PRO_BNRELU; keep None: no dropout) or X (PRO_RAW).
    folded: the kernel multiplies s and t by keep_scale first (the streaming forward kernel), which
    rounds each of them once before the fma: U keep_scale (|X s| + |t|) + U |x| where the ReLU is
    open (the data keep X s + t exactly 0, with X = t = 0, or ZGAP away from it, so it opens for
    the same elements)."""
    X = f64(X)
    if mode == PRO_RAW:
        return dict(v=X, err=np.zeros_like(X), flag=np.zeros(X.shape, bool))
    assert mode == PRO_BNRELU
    x = np.maximum(X * f64(s) + f64(t), 0.0)
    err = U * x
    if keep is not None:
        k = np.asarray(keep, bool) * float(keep_scale)
        if folded:
            err = U * (x > 0) * k * (np.abs(X * f64(s)) + np.abs(f64(t))) + U * x * k
        x = x * k
        if not folded:
            err = 2.0 * U * x
    return _stage(x, err, dtype)


# ---------------------------------------------------------------------------------------
# pcs_wgrad
# ---------------------------------------------------------------------------------------
def wgrad_ref(dZ, Y, alpha, beta, gamma, X, s, t, keep, keep_scale, dy_mode, x_mode, dtype, row_weight=None,
              folded=False):
    """dW[n, k] = sum_m dy[m, n] x[m, k] over all B*N rows; arrays [B, N, C].  row_weight [B, N]
    (None = 1) multiplies each row's term: 0 drops a row, 2 counts it twice (perturbed references
    of the sensitivity tests only); folded as x_operand's.  Returns dW, its bound, the staged
    operands and the share of flagged operand elements."""
    dy = dy_operand(dZ, Y, alpha, beta, gamma, dy_mode, dtype)
    x = x_operand(X, s, t, keep, keep_scale, x_mode, dtype, folded=folded)
    B, N, Cout = dy["v"].shape
    M = B * N
    w = np.ones((B, N)) if row_weight is None else f64(row_weight)
    dyv = (dy["v"] * w[..., None]).reshape(M, Cout)
    dye = (dy["err"] * w[..., None]).reshape(M, Cout)
    xv, xe = x["v"].reshape(M, -1), x["err"].reshape(M, -1)
    dW = dyv.T @ xv
    bound = (sum_bound(M, np.abs(dyv).T @ np.abs(xv)) * SLACK + dye.T @ (np.abs(xv) + xe) + np.abs(dyv).T @ xe)
    nflag = int(dy["flag"].sum()) + int(x["flag"].sum())
    return dict(dW=dW, bound=bound, dy=dy["v"], x=x["v"], flagged=nflag / (dy["flag"].size + x["flag"].size))


# ---------------------------------------------------------------------------------------
# pcs_gemm, PCS_PRO_BWD
# ---------------------------------------------------------------------------------------
def dgrad_ref(dZ, Y, alpha, beta, gamma, W, addend, Yp, es, et, keep, keep_scale, mean, rstd, dtype,
              ge=False, row_weight=None, lds_round=True):
    """The PCS_PRO_BWD input gradient: dgrad_from on dy = alpha dZ + beta + gamma Y as staged."""
    return dgrad_from(dy_operand(dZ, Y, alpha, beta, gamma, PRO_BWD, dtype), W, addend, Yp, es, et, keep,
                      keep_scale, mean, rstd, dtype, ge=ge, row_weight=row_weight, lds_round=lds_round)


def dgrad_from(dy, W, addend, Yp, es, et, keep, keep_scale, mean, rstd, dtype, bias=None, ge=False,
               row_weight=None, lds_round=True):
    """The PCS_EPI_DGRAD / PCS_EPI_RAW epilogue on a staged operand dy (the v / err / flag dict of
    dy_operand or x_operand): v = dy W^T (+ bias) (+ addend), dz = (es Yp + et > 0 ? v keep keep_scale
    : 0) (es = et = None: Yp > 0; keep None: no dropout), per-scene S1 = sum dz and
    S2 = sum dz (Yp - mean) rstd (0 when rstd is None), and raw = dy W^T (the PCS_EPI_RAW output).
    W [Ncols, K], bias [Ncols]; the rest [B, N, C].  The bias joins the accumulator before it is
    rounded to the storage dtype (one more fp32 add).  ge turns the mask into >= 0 and row_weight
    [B, N] weighs the rows of S1 / S2 (perturbed references of the sensitivity tests only).
    lds_round = False: a fused kernel whose accumulator stays fp32 up to the store.  Returns
    the values, their bounds as e_<name>, zmin = the smallest non-zero |es Yp + et| and the share
    of flagged dy elements."""
    W = f64(W)
    bf = dtype != "f32" and lds_round
    acc = dy["v"] @ W.T
    e_acc = sum_bound(W.shape[1], np.abs(dy["v"]) @ np.abs(W).T) * SLACK + dy["err"] @ np.abs(W).T
    r_acc = BF16_U * (np.abs(acc) + e_acc) if bf else 0.0       # bf16: the tile passes through LDS as bf16
    out = dict(raw=acc, e_raw=e_acc + r_acc, dy=dy["v"], flagged=float(dy["flag"].mean()))
    if Yp is None:
        return out
    Yp = f64(Yp)
    if bias is not None:
        acc = acc + f64(bias)
        e_acc = e_acc + U * np.abs(acc) * SLACK
        r_acc = BF16_U * (np.abs(acc) + e_acc) if bf else 0.0
    v, e_v = acc, e_acc + r_acc
    if addend is not None:
        v = acc + f64(addend)
        e_v = e_v + U * np.abs(v) * SLACK
    if keep is not None:
        k = np.asarray(keep, bool) * float(keep_scale)
        v, e_v = v * k, (e_v * k + U * np.abs(v * k)) * SLACK
    z = Yp if es is None else Yp * f64(es) + f64(et)
    gate = (z >= 0) if ge else (z > 0)
    pre, e_pre = np.where(gate, v, 0.0), np.where(gate, e_v, 0.0)
    nz = np.abs(z[z != 0])
    w = 1.0 if row_weight is None else f64(row_weight)[..., None]
    N = Yp.shape[1]
    out.update(dz=pre, e_dz=e_pre + (BF16_U * (np.abs(pre) + e_pre) if dtype != "f32" else 0.0), gate=gate,
               zmin=float(nz.min()) if nz.size else np.inf, zeros=int((z == 0).sum()),
               S1=(w * pre).sum(1), e_S1=(w * e_pre).sum(1) + sum_bound(N, (w * np.abs(pre)).sum(1)) * SLACK)
    if rstd is None:
        out.update(S2=np.zeros_like(out["S1"]), e_S2=np.zeros_like(out["S1"]))
    else:
        mean, rstd = f64(mean), f64(rstd)
        xhat, xabs = (Yp - mean) * rstd, (np.abs(Yp) + np.abs(mean)) * np.abs(rstd)
        out.update(S2=(w * pre * xhat).sum(1),
                   e_S2=(w * e_pre * xabs).sum(1) + sum_bound(N + 3, (w * np.abs(pre) * xabs).sum(1)) * SLACK)
    return out


# ---------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------
# cls: "f32" (wgrad_kernel<float> / gemm_nt_kernel<float>), "bf16g" (the same kernels in bf16,
# PCS_FLAG_GENERIC), "big" (bf16, default flags, shapes of the 256x256 kernels) and, for pcs_gemm,
# "seam" (bf16, default flags, a wide-class shape whose operands send it to the generic kernel)
WCase = namedtuple("WCase", "cls Cout Cin dy_mode x_mode mask N sps ldw_pad")
GCase = namedtuple("GCase", "cls K Ncols epi variant N cps")
B = 3
VARIANTS = ("plain", "cmask", "addend", "cmask_addend", "noes", "norstd", "nostats")


def dtype_of(case):
    return "f32" if case.cls == "f32" else "bf16"


def wstep(cls):
    return 16 if cls == "f32" else 64


def wcase_id(c):
    m = {PRO_RAW: "raw", PRO_BNRELU: "bnrelu", PRO_BWD: "bwd"}
    return (f"{c.cls}-{c.Cout}x{c.Cin}-{m[c.dy_mode]}_{m[c.x_mode]}{'_mask' if c.mask else ''}-N{c.N}"
            f"-sps{c.sps}-pad{c.ldw_pad}")


def gcase_id(c):
    return f"{c.cls}-K{c.K}xN{c.Ncols}-{'dgrad' if c.epi == EPI_DGRAD else 'raw'}-{c.variant}-N{c.N}-cps{c.cps}"


def _wgrad_cases():
    modes = [(PRO_BWD, PRO_BNRELU, False), (PRO_BWD, PRO_BNRELU, True), (PRO_BWD, PRO_RAW, False),
             (PRO_RAW, PRO_BNRELU, False)]
    shapes = [(64, 64), (128, 64), (64, 128), (128, 128), (192, 192), (256, 128)]
    out = []
    for cls in ("f32", "bf16g"):
        st = wstep(cls)
        for sh in shapes + ([(256, 256), (256, 512)] if cls == "bf16g" else []):
            out += [WCase(cls, *sh, dy, x, mk, 2 * st + 5, 0, 0) for dy, x, mk in modes]
        out.append(WCase(cls, 64, 64, PRO_RAW, PRO_BNRELU, True, 2 * st + 5, 0, 0))   # dispatched, no caller yet
        # every N edge, the library's own splits (two per scene at 4 step + 1), padded rows
        out += [WCase(cls, 128, 64, PRO_BWD, PRO_BNRELU, True, n, 0, 24) for n in (1, st - 1, st, st + 1, 4 * st + 1)]
        # three caller-set slices of 2 step, 2 step and 3 rows
        out.append(WCase(cls, 128, 64, PRO_BWD, PRO_BNRELU, True, 6 * st + 3, 3, 24))
    st = 64
    for sh in ((256, 256), (256, 512)):
        out += [WCase("big", *sh, PRO_BWD, PRO_BNRELU, mk, 2 * st + 5, 0, 0) for mk in (False, True)]
        out.append(WCase("big", *sh, PRO_BWD, PRO_RAW, False, 2 * st + 5, 0, 0))     # lands on wgrad_kernel
    out += [WCase("big", 256, 256, PRO_BWD, PRO_BNRELU, True, n, 0, 24) for n in (1, st - 1, st, st + 1, 4 * st + 1)]
    out.append(WCase("big", 256, 256, PRO_BWD, PRO_BNRELU, False, 8 * st + 1, 0, 24))  # two slices per scene
    out.append(WCase("big", 256, 256, PRO_BWD, PRO_BNRELU, True, 6 * st + 3, 3, 24))
    return out


def _gemm_cases():
    out = []
    for cls in ("f32", "bf16g"):
        ks = 16 if cls == "f32" else 32
        for sh in ((ks, 64), (64, 64), (128, 64), (64, 128), (128, 256)):
            out += [GCase(cls, *sh, EPI_DGRAD, v, 133, 0) for v in ("plain", "cmask_addend")]
        out.append(GCase(cls, 512, 64, EPI_RAW, "plain", 133, 0))
        out.append(GCase(cls, 64, 128, EPI_RAW, "plain", 133, 0))                    # the 128-column tile
        out += [GCase(cls, 64, 128, EPI_DGRAD, v, 133, 0) for v in VARIANTS if v not in ("plain", "cmask_addend")]
        out += [GCase(cls, 128, 64, EPI_DGRAD, "cmask", n, 0) for n in (1, 127, 128, 129, 2 * 128 + 5)]
        out.append(GCase(cls, 128, 64, EPI_DGRAD, "cmask", 2 * 128 + 5, 2))
    for sh in ((256, 256), (256, 512)):                       # gemm_big_kernel
        out += [GCase("big", *sh, EPI_DGRAD, v, 257, 0) for v in ("plain", "cmask", "addend", "nostats")]
    out += [GCase("big", 256, 256, EPI_DGRAD, "cmask", n, 0) for n in (255, 256, 3 * 256 + 7)]
    out.append(GCase("big", 256, 256, EPI_DGRAD, "addend", 3 * 256 + 7, 2))
    out.append(GCase("big", 256, 256, EPI_RAW, "plain", 257, 0))
    for v in ("cmask_addend", "noes", "norstd"):              # wide class on gemm_nt_kernel
        out.append(GCase("seam", 256, 512, EPI_DGRAD, v, 3 * 256 + 7, 0))
    out += [GCase("seam", 256, 512, EPI_DGRAD, "cmask_addend", n, 0) for n in (255, 257)]
    out.append(GCase("seam", 256, 512, EPI_DGRAD, "noes", 3 * 256 + 7, 2))
    return out


WGRAD_CASES = _wgrad_cases()
GEMM_CASES = _gemm_cases()


# ---------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------
def _stored(a, dtype):
    """a as the storage dtype holds it (fp64 array)."""
    return f64(np.asarray(a, np.float32)) if dtype == "f32" else bf16_round(a)


def _seed(case, kind):
    return [int(x) if not isinstance(x, str) else sum(map(ord, x)) for x in case] + [kind == "exact"]


def wgrad_data(case, kind):
    """Operands of one pcs_wgrad case: "value" (Gaussian, scaled like the model's activations) or
    "exact" (small integers and powers of two: dy, x and every sum are exact in bf16 / fp32, so a
    correct kernel reproduces the fp64 reference bit for bit whatever its summation order).
    keep is None when the case has no x_mask."""
    r = np.random.default_rng(_seed(case, kind))
    dt = dtype_of(case)
    N, Cout, Cin = case.N, case.Cout, case.Cin
    if kind == "exact":
        d = dict(dZ=2.0 * r.integers(-4, 5, (B, N, Cout)), Y=2.0 * r.integers(-3, 4, (B, N, Cout)),
                 alpha=r.choice([1.0, -1.0, 2.0, -2.0, 0.5, -0.5], Cout), beta=1.0 * r.integers(-3, 4, Cout),
                 gamma=r.choice([0.0, 0.5, -0.5, 1.0, -1.0], Cout), X=1.0 * r.integers(-6, 7, (B, N, Cin)),
                 s=np.ones(Cin), t=1.0 * r.integers(-3, 4, Cin), keep=r.random((B, N, Cin)) < 0.5, keep_scale=2.0)
    else:
        sign = lambda n: np.where(r.random(n) < 0.25, -1.0, 1.0)   # noqa: E731
        d = dict(dZ=_stored(0.1 * r.standard_normal((B, N, Cout)), dt), Y=_stored(r.standard_normal((B, N, Cout)), dt),
                 alpha=r.uniform(0.5, 1.5, Cout) * sign(Cout), beta=0.05 * r.standard_normal(Cout),
                 gamma=0.1 * r.standard_normal(Cout), X=_stored(r.standard_normal((B, N, Cin)), dt),
                 s=r.uniform(0.5, 1.5, Cin) * sign(Cin), t=0.3 * r.standard_normal(Cin),
                 keep=r.random((B, N, Cin)) < 0.7, keep_scale=1.0 / 0.7)
    for k in ("alpha", "beta", "gamma", "s", "t"):
        d[k] = f64(np.asarray(d[k], np.float32))
    d["keep_scale"] = float(np.float32(d["keep_scale"]))
    if not case.mask:
        d["keep"], d["keep_scale"] = None, 1.0
    return d


def wgrad_reference(case, d, **kw):
    return wgrad_ref(d["dZ"], d["Y"], d["alpha"], d["beta"], d["gamma"], d["X"], d["s"], d["t"], d["keep"],
                     d["keep_scale"], case.dy_mode, case.x_mode, dtype_of(case), **kw)


def gemm_data(case, kind):
    """Operands of one pcs_gemm PRO_BWD case; the variant decides which optional ones are None.
    Exact data: |dy| <= 12 and eight +-1 entries per row of W, so every partial sum of |dy| |W| is
    at most 96, with |addend| <= 32 and keep_scale = 2 the stored dz at most 256; Yp es + et hits 0
    often.  Value data: Yp es + et is exactly 0 (Yp = 0 where et = 0) in some places and at least
    ZGAP away from it everywhere else, so no fp32 rounding flips the mask against the reference."""
    r = np.random.default_rng(_seed(case, kind))
    dt = dtype_of(case)
    N, K, Nc = case.N, case.K, case.Ncols
    if kind == "exact":
        W = np.zeros((Nc, K))
        for n in range(Nc):
            W[n, r.choice(K, 8, replace=False)] = r.choice([-1.0, 1.0], 8)
        d = dict(dZ=2.0 * r.integers(-2, 3, (B, N, K)), Y=2.0 * r.integers(-1, 2, (B, N, K)),
                 alpha=r.choice([1.0, -1.0, 2.0, -2.0, 0.5, -0.5], K), beta=1.0 * r.integers(-2, 3, K),
                 gamma=r.choice([0.0, 0.5, -0.5, 1.0, -1.0], K), W=W, addend=1.0 * r.integers(-32, 33, (B, N, Nc)),
                 Yp=1.0 * r.integers(-4, 5, (B, N, Nc)), es=r.choice([1.0, -1.0, 2.0], Nc),
                 et=1.0 * r.integers(-2, 3, Nc), mean=1.0 * r.integers(-2, 3, Nc), rstd=r.choice([0.5, 1.0, 2.0], Nc),
                 keep=r.random((B, N, Nc)) < 0.5, keep_scale=2.0)
    else:
        sign = lambda n: np.where(r.random(n) < 0.25, -1.0, 1.0)   # noqa: E731
        es = f64((r.uniform(0.5, 1.5, Nc) * sign(Nc)).astype(np.float32))
        et = f64((0.5 * r.standard_normal(Nc)).astype(np.float32))
        et[::16] = 0.0
        Yp = _stored(r.standard_normal((B, N, Nc)), dt)
        if case.variant == "noes":
            Yp = np.where(np.abs(Yp) < ZGAP, 0.05, Yp)
            Yp[r.random(Yp.shape) < 0.02] = 0.0
        else:
            z = Yp * es + et
            Yp = np.where(np.abs(z) < ZGAP, _stored((np.where(z >= 0, 0.05, -0.05) - et) / es, dt), Yp)
            Yp[:, :, ::16] = np.where(r.random((B, N, len(et[::16]))) < 0.05, 0.0, Yp[:, :, ::16])
        Yp[:, 0, ::16] = 0.0                  # every scene's first row: zeros also at N = 1
        d = dict(dZ=_stored(0.1 * r.standard_normal((B, N, K)), dt), Y=_stored(r.standard_normal((B, N, K)), dt),
                 alpha=r.uniform(0.5, 1.5, K) * sign(K), beta=0.05 * r.standard_normal(K),
                 gamma=0.1 * r.standard_normal(K), W=_stored(r.standard_normal((Nc, K)) / np.sqrt(K), dt),
                 addend=_stored(0.1 * r.standard_normal((B, N, Nc)), dt), Yp=Yp, es=es, et=et,
                 mean=0.3 * r.standard_normal(Nc), rstd=np.abs(1.0 + 0.1 * r.standard_normal(Nc)),
                 keep=r.random((B, N, Nc)) < 0.7, keep_scale=1.0 / 0.7)
    for k in ("alpha", "beta", "gamma", "mean", "rstd"):
        d[k] = f64(np.asarray(d[k], np.float32))
    d["keep_scale"] = float(np.float32(d["keep_scale"]))
    v = case.variant
    if v not in ("cmask", "cmask_addend"):
        d["keep"], d["keep_scale"] = None, 1.0
    if v not in ("addend", "cmask_addend"):
        d["addend"] = None
    if v == "noes":
        d["es"] = d["et"] = None
    if v == "norstd":
        d["mean"] = d["rstd"] = None
    if case.epi == EPI_RAW:
        d["Yp"] = None
    return d


def gemm_reference(case, d, **kw):
    return dgrad_ref(d["dZ"], d["Y"], d["alpha"], d["beta"], d["gamma"], d["W"], d["addend"], d["Yp"], d["es"],
                     d["et"], d["keep"], d["keep_scale"], d["mean"], d["rstd"], dtype_of(case), **kw)


def pack_bits(keep):
    """[..., C] bool -> [..., C/8] uint8, bit i of byte j = channel 8 j + i."""
    return np.packbits(np.asarray(keep, bool), axis=-1, bitorder="little")
