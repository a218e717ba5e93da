"""fp64 restatements of the small glue kernels of csrc/small.hip and of the segmentation head,
from their descriptions in include/pcs.h (not a test module).  tests/test_small_refs.py proves
them against torch in fp64 on the CPU; the GPU tests (test_gpu_small_kernels.py,
test_gpu_conv1.py, test_gpu_colstats.py, test_gpu_head.py) compare the kernels with them.

Everything is NumPy float64.  The partial generators build the per-chunk records the GEMM
epilogues hand to the finalize kernels; they compute in fp64 and round to fp32 last
(``rounded=True``), so a reference fed the rounded records consumes exactly what the kernel
reads.
"""
import numpy as np

U = 2.0 ** -24          # fp32 unit roundoff (half an ulp, relative)
ULP = 2.0 ** -23        # one rounding fp64 -> fp32, as a safe relative bound
POOL_NONE = 0x7fffffff  # "no candidate" row of a max-pool record


def f64(x):
    return None if x is None else np.asarray(x, dtype=np.float64)


def chunk_bounds(N, cps, rpc):
    """[(lo, hi)] rows of the cps chunks of one scene (the last one may be ragged)."""
    out = [(j * rpc, min((j + 1) * rpc, N)) for j in range(cps)]
    assert all(hi > lo for lo, hi in out) and out[-1][1] == N, (N, cps, rpc)
    return out


# ---------------------------------------------------------------------------------------
# error bounds
# ---------------------------------------------------------------------------------------
def sum_bound(nterms, abs_sum):
    """Bound on an fp32 sum of ``nterms`` terms (products included: fused or rounded, each term
    then passes through at most nterms roundings), whatever the summation order:
    nterms * 2^-24 * sum |terms|."""
    return nterms * U * f64(abs_sum)


def round_bound(*abs_terms):
    """One rounding of an fp64 result to fp32: 2^-23 times the sum of the absolute terms the
    result is a sum or difference of (for a single term: 2^-23 relative)."""
    return ULP * sum(np.abs(f64(t)) for t in abs_terms)


def assert_within(got, ref, bound, what=""):
    got, ref, bound = f64(got), f64(ref), f64(bound)
    err = np.abs(got - ref)
    bad = ~(err <= bound)           # a NaN fails
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(np.isnan(err), np.inf, err - bound)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.size} outside the bound; worst at {i}: "
                             f"got {got[i]!r} ref {ref[i]!r} err {err[i]:.3e} bound {np.broadcast_to(bound, err.shape)[i]:.3e}")
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


# ---------------------------------------------------------------------------------------
# partial generators: y [B, N, C] fp64 and a chunking -> per-chunk records [B*cps, C, k]
# ---------------------------------------------------------------------------------------
def welford_partials(y, cps, rpc, rounded=True):
    """(mean, M2) of every chunk."""
    y = f64(y)
    B, N, C = y.shape
    out = np.empty((B, cps, C, 2))
    for j, (lo, hi) in enumerate(chunk_bounds(N, cps, rpc)):
        m = y[:, lo:hi].mean(1)
        out[:, j, :, 0] = m
        out[:, j, :, 1] = ((y[:, lo:hi] - m[:, None]) ** 2).sum(1)
    out = out.reshape(B * cps, C, 2)
    return out.astype(np.float32) if rounded else out


def sum_partials(dz, xhat, cps, rpc, rounded=True):
    """(S1 = sum dz, S2 = sum dz * xhat) of every chunk."""
    dz, xhat = f64(dz), f64(xhat)
    B, N, C = dz.shape
    out = np.empty((B, cps, C, 2))
    for j, (lo, hi) in enumerate(chunk_bounds(N, cps, rpc)):
        out[:, j, :, 0] = dz[:, lo:hi].sum(1)
        out[:, j, :, 1] = (dz[:, lo:hi] * xhat[:, lo:hi]).sum(1)
    out = out.reshape(B * cps, C, 2)
    return out.astype(np.float32) if rounded else out


def pool_partials(y, cps, rpc):
    """(max, argmax, min, argmin) of every chunk as fp32 [B*cps, C, 4]; the rows are global
    (b*N + n), first occurrence, stored as int32 bits in slots 1 and 3.  y is rounded to fp32
    first (the records carry stored values)."""
    y = np.asarray(y, dtype=np.float32)
    B, N, C = y.shape
    out = np.empty((B, cps, C, 4), np.float32)
    idx = out.view(np.int32)
    base = (np.arange(B, dtype=np.int64) * N)[:, None]
    for j, (lo, hi) in enumerate(chunk_bounds(N, cps, rpc)):
        out[:, j, :, 0] = y[:, lo:hi].max(1)
        idx[:, j, :, 1] = base + lo + y[:, lo:hi].argmax(1)
        out[:, j, :, 2] = y[:, lo:hi].min(1)
        idx[:, j, :, 3] = base + lo + y[:, lo:hi].argmin(1)
    return out.reshape(B * cps, C, 4)


# ---------------------------------------------------------------------------------------
# BatchNorm finalize
# ---------------------------------------------------------------------------------------
def bn_fwd_from_partials(stats, B, N, cps, rpc, gamma, beta, moff, rmean, rvar, momentum, eps):
    """pcs_bn_fwd_finalize: batch mean / biased variance over the B*N rows from per-chunk
    (mean, M2), the fused affine y*scale + shift, the running-buffer update (unbiased variance;
    mean_offset added to running_mean only) and the per-scene sums of y."""
    st = f64(stats).reshape(B, cps, -1, 2)
    gamma, beta = f64(gamma), f64(beta)
    nb = np.array([hi - lo for lo, hi in chunk_bounds(N, cps, rpc)], np.float64)[None, :, None]
    M = float(B * N)
    scene_sum = (nb * st[..., 0]).sum(1)
    mean = scene_sum.sum(0) / M
    m2 = st[..., 1].sum((0, 1)) + (nb * (st[..., 0] - mean) ** 2).sum((0, 1))
    var = m2 / M
    rstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * rstd
    out = dict(mean=mean, rstd=rstd, scale=scale, shift=beta - mean * scale, scene_sum=scene_sum,
               shift_terms=np.abs(beta) + np.abs(mean * scale))
    if rmean is not None:
        unb = m2 / (M - 1) if M > 1 else m2
        tm = mean + (f64(moff) if moff is not None else 0.0)
        out["rmean"] = (1.0 - momentum) * f64(rmean) + momentum * tm
        out["rvar"] = (1.0 - momentum) * f64(rvar) + momentum * unb
        out["rmean_terms"] = np.abs((1.0 - momentum) * f64(rmean)) + np.abs(momentum * tm)
    return out


def bn_eval_ref(gamma, beta, rmean, rvar, moff, eps):
    """pcs_bn_eval_coefs: scale / shift from the running buffers, for stored activations that
    omit mean_offset."""
    scale = f64(gamma) / np.sqrt(f64(rvar) + eps)
    mu = f64(rmean) - (f64(moff) if moff is not None else 0.0)
    return dict(scale=scale, shift=f64(beta) - mu * scale, shift_terms=np.abs(f64(beta)) + np.abs(mu * scale))


def bn_bwd_coefs(S1, S2, Sy, M, mean, rstd, gamma):
    """dy = alpha*dz + beta_c + gamma_c*y of a train-mode BatchNorm from S1 = sum dz,
    S2 = sum dz*xhat; dbias = sum over the rows of dy = alpha*S1 + M*beta_c + gamma_c*Sy."""
    al = gamma * rstd
    ga = -gamma * rstd * rstd * S2 / M
    b1, b2 = -gamma * rstd * S1 / M, -ga * mean
    be = b1 + b2
    out = dict(alpha=al, gamma_c=ga, beta_c=be, dgamma=S2, dbeta=S1,
               beta_c_terms=np.abs(b1) + np.abs(b2))
    if Sy is not None:
        out["dbias"] = al * S1 + M * be + ga * Sy
        out["dbias_terms"] = np.abs(al * S1) + np.abs(M * be) + np.abs(ga * Sy)
    else:
        out["dbias"] = np.zeros_like(al)
        out["dbias_terms"] = np.zeros_like(al)
    return out


def bn_bwd_from_partials(stats, B, N, cps, mean, rstd, gamma, scene_sum):
    """pcs_bn_bwd_finalize from per-chunk (S1, S2); scene_sum [B, C] (sum y per scene) or None
    (then dbias is 0)."""
    st = f64(stats).reshape(B, cps, -1, 2)
    scene_s1 = st[..., 0].sum(1)
    Sy = f64(scene_sum).sum(0) if scene_sum is not None else None
    out = bn_bwd_coefs(scene_s1.sum(0), st[..., 1].sum((0, 1)), Sy, float(B * N), f64(mean), f64(rstd), f64(gamma))
    out["scene_s1"] = scene_s1
    return out


# ---------------------------------------------------------------------------------------
# global max-pool
# ---------------------------------------------------------------------------------------
def pool_finalize_ref(pool, B, N, cps, s, t):
    """pcs_pool_finalize on finite records: the max (s > 0) or min (s < 0) over a scene's chunk
    records, ties to the smaller row; s == 0 keeps the max and names the scene's first row; a
    row outside the scene (the "none" sentinel) becomes the scene's first row.  Returns
    g = relu(y*s + t) in fp64, am (int64), ysel (fp32, exact) and z = y*s + t."""
    rec = np.asarray(pool, np.float32).reshape(B, cps, -1, 4)
    idx = rec.view(np.int32).astype(np.int64)
    s, t = f64(s), f64(t)
    C = rec.shape[2]
    ysel = np.empty((B, C), np.float32)
    am = np.empty((B, C), np.int64)
    for b in range(B):
        for c in range(C):
            mx = max(range(cps), key=lambda j: (rec[b, j, c, 0], -idx[b, j, c, 1]))
            mn = min(range(cps), key=lambda j: (rec[b, j, c, 2], idx[b, j, c, 3]))
            if s[c] > 0:
                ysel[b, c], am[b, c] = rec[b, mx, c, 0], idx[b, mx, c, 1]
            elif s[c] < 0:
                ysel[b, c], am[b, c] = rec[b, mn, c, 2], idx[b, mn, c, 3]
            else:
                ysel[b, c], am[b, c] = rec[b, mx, c, 0], b * N
            if not (b * N <= am[b, c] < (b + 1) * N):
                am[b, c] = b * N
    with np.errstate(invalid="ignore"):
        z = ysel.astype(np.float64) * s + t
    return dict(g=np.maximum(z, 0.0), am=am, ysel=ysel, z=z)


def pool_bwd_ref(N, s1_alpha, s1_beta, s1_gamma, s1_scene_s1, s1_scene_sum, W, col_off, g, ysel,
                 g_mean, g_rstd, g_gamma, g_scene_sum):
    """pcs_pool_bwd.  Returns (out, err): the fp64 results and, for each, the bound on the
    kernel's error that its fp32 sums allow (sum_bound), propagated linearly into what is
    derived from them (dg -> sp, S1, S2 -> alpha, beta_c, gamma_c, dbias), plus the final
    rounding to fp32 (round_bound)."""
    a, b_, gm1 = f64(s1_alpha), f64(s1_beta), f64(s1_gamma)
    s1, sy1, g, ysel = f64(s1_scene_s1), f64(s1_scene_sum), f64(g), f64(ysel)
    mu, r, gam, gsum = f64(g_mean), f64(g_rstd), f64(g_gamma), f64(g_scene_sum)
    B, Cg = g.shape
    Cs = a.shape[0]
    Wg = f64(W)[:, col_off:col_off + Cg]
    M = float(B * N)
    # csum[b, n] = sum over the rows of scene b of dy_seg1[:, n]: three fp32 terms
    csum = a * s1 + N * b_ + gm1 * sy1
    e_csum = sum_bound(3, np.abs(a * s1) + np.abs(N * b_) + np.abs(gm1 * sy1))
    dW = csum.T @ g                                     # [Cs, Cg], B terms from the fp32 csum
    e_dW = sum_bound(B, np.abs(csum).T @ np.abs(g)) + e_csum.T @ np.abs(g)
    dg = csum @ Wg                                      # [B, Cg], Cs terms
    e_dg = sum_bound(Cs, np.abs(csum) @ np.abs(Wg)) + e_csum @ np.abs(Wg)
    gate = g > 0
    dz, e_dz = np.where(gate, dg, 0.0), np.where(gate, e_dg, 0.0)
    xhat = (ysel - mu) * r
    S1, S2, Sy = dz.sum(0), (dz * xhat).sum(0), gsum.sum(0)
    e_S1, e_S2 = e_dz.sum(0), (e_dz * np.abs(xhat)).sum(0)
    out = bn_bwd_coefs(S1, S2, Sy, M, mu, r, gam)
    al = out["alpha"]
    out.update(csum=csum, dW=dW, sp=al * dz)
    p_ga = np.abs(gam) * r * r * e_S2 / M               # propagated, before the last rounding
    p_be = np.abs(gam) * r * e_S1 / M + p_ga * np.abs(mu)
    err = dict(
        csum=e_csum, dW=e_dW,
        sp=np.abs(al) * e_dz + round_bound(al * dz),
        alpha=round_bound(al),
        gamma_c=p_ga + round_bound(out["gamma_c"]),
        beta_c=p_be + round_bound(out["beta_c_terms"]),
        dgamma=e_S2 + round_bound(S2), dbeta=e_S1 + round_bound(S1),
        dbias=np.abs(al) * e_S1 + M * p_be + p_ga * np.abs(Sy) + round_bound(out["dbias_terms"]))
    return out, err


def scene_gemv_ref(g, W, col_off, bias):
    """pcs_scene_gemv, uncentred: v[b, n] = bias[n] + sum_k W[n, col_off + k] g[b, k]; also the
    bound on an fp32 evaluation (Kg products and the bias)."""
    g = f64(g)
    Wg = f64(W)[:, col_off:col_off + g.shape[1]]
    bb = f64(bias) if bias is not None else np.zeros(Wg.shape[0])
    v = g @ Wg.T + bb
    return v, sum_bound(g.shape[1] + 1, np.abs(g) @ np.abs(Wg).T + np.abs(bb))


# ---------------------------------------------------------------------------------------
# segmentation head
# ---------------------------------------------------------------------------------------
HEAD_FWD, HEAD_CE, HEAD_BWD = 0, 1, 2
# expf / logf error in ulps (2^-23 relative each).  The ROCm install documents neither in its
# shipped math documentation, so 2 ulp each is assumed.
EXP_ULPS = LOG_ULPS = 2.0


def head_ref(Y, s, t, mean, rstd, W, bias, mode, labels=None, class_weight=None, wsum=None, dlogits=None):
    """pcs_head: seg_conv4 on a = relu(Y*s + t), and by mode the weighted cross entropy with its
    gradient (HEAD_CE; labels outside [0, C) are ignored, wsum None = 1) or caller-supplied
    dlogits (HEAD_BWD), then the backward: dz = (a > 0) * (dl W), S1 = sum_m dz,
    S2 = sum_m dz * (Y - mean) * rstd, dW = dl^T a, db = sum_m dl.

    Returns a dict of the fp64 results and, as ``abs_<name>``, the sum of the absolute terms each
    one is a sum of (what its rounding errors scale with).  CE also returns the per-row pieces
    (valid, w, lse, mx, p, nll) that head_bounds propagates through exp and log."""
    Y, s, t, W, bias = f64(Y), f64(s), f64(t), f64(W), f64(bias)
    z = Y * s + t
    a = np.maximum(z, 0.0)
    out = dict(z=z, a=a, logits=a @ W.T + bias, abs_logits=np.abs(a) @ np.abs(W).T + np.abs(bias))
    if mode == HEAD_FWD:
        return out
    lg = out["logits"]
    M, C = lg.shape
    if mode == HEAD_CE:
        lab = np.asarray(labels, np.int64)
        valid = (lab >= 0) & (lab < C)
        li = np.where(valid, lab, 0)
        w = np.where(valid, f64(class_weight)[li], 0.0)
        g = 1.0 if wsum is None else 1.0 / float(wsum)
        mx = lg.max(1)
        lse = mx + np.log(np.exp(lg - mx[:, None]).sum(1))
        p = np.exp(lg - lse[:, None])
        onehot = np.zeros((M, C))
        onehot[np.arange(M), li] = 1.0
        nll = lse - lg[np.arange(M), li]
        dl = (w * g)[:, None] * (p - onehot)
        out.update(valid=valid, label=li, w=w, gscale=g, mx=mx, lse=lse, p=p, onehot=onehot, nll=nll,
                   row_loss=w * nll, loss_sum=float((w * nll).sum()), abs_loss_sum=float((w * np.abs(nll)).sum()))
    else:
        dl = f64(dlogits)
        assert dl.shape == (M, C)
    mean, rstd = f64(mean), f64(rstd)
    gate = a > 0
    dz = np.where(gate, dl @ W, 0.0)
    xhat = (Y - mean) * rstd
    # S2 is evaluated as sum dz*xhat or as rstd*(sum dz*Y - mean*sum dz): the terms of either
    xabs = (np.abs(Y) + np.abs(mean)) * np.abs(rstd)
    out.update(dl=dl, dz=dz, xhat=xhat, xabs=xabs, abs_dz=np.where(gate, np.abs(dl) @ np.abs(W), 0.0),
               S1=dz.sum(0), S2=(dz * xhat).sum(0), abs_S1=np.abs(dz).sum(0), abs_S2=(np.abs(dz) * xabs).sum(0),
               dW=dl.T @ a, db=dl.sum(0), abs_dW=np.abs(dl).T @ np.abs(a), abs_db=np.abs(dl).sum(0))
    return out


def head_bounds(ref, W, mode, rows_per_chunk, bf16_dz=False):
    """Bounds on an fp32 evaluation of head_ref's outputs (any summation order), from its
    absolute sums; first order in 2^-24, propagated linearly.

    a       one rounding (the fma of Y*s + t);
    logits  128 products and the bias on the rounded a;
    CE      lse = mx + log(sum exp(z - mx)): 1-Lipschitz in the logits, the rounding of z - mx
            (relative U*|z - mx| on each exp term), EXP_ULPS per exp, C - 1 additions, LOG_ULPS on
            the log, one rounding of the sum; p = exp(z - lse): the argument's error e enters as
            expm1(e); dl = (w/wsum)*(p - onehot): the reciprocal, two products, one difference;
            loss: the row's w*(lse - z_l), then a sum of at most rows_per_chunk terms per chunk;
    dz      a C-term chain on the inexact dl (plus 2^-8 |ref| for a bf16 store);
    S1, S2, dW, db  sums of at most rows_per_chunk terms per chunk, of the inexact dz / dl / a."""
    W = np.abs(f64(W))
    C = W.shape[0]
    e_a = round_bound(ref["a"])
    e_z = sum_bound(W.shape[1] + 1, ref["abs_logits"]) + e_a @ W.T
    out = dict(a=e_a, logits=e_z)
    if mode == HEAD_FWD:
        return out
    if mode == HEAD_CE:
        lg, mx, lse, p, w = ref["logits"], ref["mx"], ref["lse"], ref["p"], ref["w"]
        M = lg.shape[0]
        pm = np.exp(lg - mx[:, None])
        pm /= pm.sum(1, keepdims=True)
        e_log = (U * (pm * np.abs(lg - mx[:, None])).sum(1) + EXP_ULPS * ULP + (C - 1) * U
                 + LOG_ULPS * ULP * np.abs(lse - mx))
        e_lse = e_z.max(1) + e_log + round_bound(mx, lse - mx)
        e_arg = e_z + e_lse[:, None] + round_bound(lg - lse[:, None])
        e_p = p * (np.expm1(e_arg) + EXP_ULPS * ULP)
        wg = np.abs(w * ref["gscale"])[:, None]
        e_dl = wg * e_p + 4.0 * ULP * np.abs(ref["dl"])
        e_row = w * (e_lse + e_z[np.arange(M), ref["label"]] + round_bound(ref["nll"])) + round_bound(ref["row_loss"])
        out["loss_sum"] = float(e_row.sum() + sum_bound(rows_per_chunk, ref["abs_loss_sum"]))
    else:
        e_dl = np.zeros_like(ref["dl"])
    gate = ref["a"] > 0
    e_dz = np.where(gate, sum_bound(C, ref["abs_dz"]) + e_dl @ W, 0.0)
    n = rows_per_chunk
    out.update(dl=e_dl, dz=e_dz + (2.0 ** -8 * np.abs(ref["dz"]) if bf16_dz else 0.0),
               S1=sum_bound(n, ref["abs_S1"]) + e_dz.sum(0),
               S2=sum_bound(n + 3, ref["abs_S2"]) + (e_dz * ref["xabs"]).sum(0),
               dW=sum_bound(n, ref["abs_dW"]) + e_dl.T @ np.abs(ref["a"]) + np.abs(ref["dl"]).T @ e_a,
               db=sum_bound(n, ref["abs_db"]) + e_dl.sum(0))
    return out


# ---------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------
def adam_ref(p, g, m, v, step, lr, b1, b2, eps, wd, scale=None):
    """One torch.optim.Adam step (coupled weight decay, amsgrad off) in fp64.  With a scale the
    effective gradient is g * scale.  Returns (p, m, v, g_eff, upd) with upd = lr/bc1 * m/denom."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    ge = g if scale is None else g * float(scale)
    gi = ge + wd * p
    m = b1 * m + (1.0 - b1) * gi
    v = b2 * v + (1.0 - b2) * gi * gi
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    upd = (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
    return p - upd, m, v, ge, upd
