"""fp64 restatement of the forward half of pcs_gemm as include/pcs.h describes it (not a test
module): PCS_PRO_RAW / PCS_PRO_BNRELU operands through PCS_EPI_FWD, PCS_EPI_BNRELU, PCS_EPI_RAW and
the folded PCS_EPI_DGRAD, with the per-chunk statistics, column sums and max-pool records.
tests/test_fwd_refs.py proves it against torch in fp64 on the CPU; tests/test_gpu_fwd_gemm.py
compares every forward kernel behind pcs_gemm with it.  The case list both files walk is here.

Everything is NumPy float64 on arrays shaped [B, N, C] that hold the values as stored (fp32 or
bf16).  The operand is bwd_refs.x_operand (x = A, or x = relu(A s + t) [keep keep_scale], rounded
to bf16 after the keep scale, with its midpoint flags), the folded input gradient is
bwd_refs.dgrad_from on that operand.

Bounds (none tuned on GPU output), element-wise, first order in 2^-24 (U) with the 2^-10 relative
SLACK of bwd_refs for the higher orders:

  acc = x W^T         sum_bound(K, |x| |W|^T): K fused multiply-adds in any order, plus the operand
                      error through |W| (fp32: the roundings that form x; bf16: one bf16 spacing on
                      the flagged elements, nothing elsewhere);
  y = acc + b         b = scene_bias[scene] if given, else bias if given: one fp32 add, U |y|;
  z = y es + et       one fma: |es| e_y + U |z|.  This is gemm_nt_kernel and gemm_big_kernel.  Only
                      the streaming kernel folds the bias into the shift, z = fma(acc, es, et + b es):
                      |es| e_acc + U (|b es| + |et + b es| + |z|), and only its cases are held to that
                      form (fwd_ref(folded=True)); without a bias the two forms are the same;
  a = relu(z)         ReLU is 1-Lipschitz: e_a = e_z (the value data also keep z at least ZGAP from
                      0 outside the constant column, where it is exactly 0);
  store               fp32: the value the last step rounded.  bf16: 2^-8 (|v| + e_v).  The reference
                      is the unrounded v;
  folded operand      the streaming kernel multiplies s and t by keep_scale before the fma; see
                      bwd_refs.x_operand(folded=True).  The data keep A s + t exactly 0 (A = t = 0)
                      or at least ZGAP away from 0, so the prologue's ReLU opens for the same
                      elements whichever way it is evaluated;
  EPI_DGRAD           bwd_refs.dgrad_from (the bias joins the accumulator before it is rounded).

Statistics and max-pool records are functions of the values a kernel stored, so they are checked
against the kernel's own stored C (stats_ref, pool_ref on `got`), as tests/test_gpu_conv1.py does:
chunk means within 1e-5 max|C|, chunk M2 within 1e-4 M2 (the project's bounds for fp32 Welford
partials; a constant column must give M2 = 0 exactly), EPI_BNRELU column sums within
sum_bound(rows, sum |C|), pool records exactly (values equal, rows the first occurrence).  On the
CPU the same functions run on the reference output rounded to the storage dtype."""
from collections import namedtuple

import numpy as np

import bwd_refs as R
from bwd_refs import (BF16_U, SLACK, ZGAP, B, PRO_RAW, PRO_BNRELU, EPI_DGRAD, EPI_RAW,  # noqa: F401
                      U, f64, sum_bound, assert_within, bf16_round, pack_bits, dtype_of)
from small_refs import chunk_bounds, welford_partials, pool_partials, sum_partials

EPI_FWD, EPI_BNRELU = 0, 3
FCase = namedtuple("FCase", "cls K Ncols pro epi variant N cps")
FWD_VARIANTS = ("plain", "bias", "scene_bias", "both", "mask", "pool", "pool_es", "mask_pool", "nostats", "nullC")
DGRAD_VARIANTS = ("plain", "cmask_addend", "bias", "noes", "norstd")
# rows per step and output columns per workgroup of fwd_stream_kernel (FsCfg in csrc/fwd_stream.hip),
# and the grid it aims at
STREAM = {(64, 512): (64, 512, 256), (512, 256): (32, 256, 256), (256, 128): (64, 128, 256),
          (128, 1024): (64, 512, 256), (64, 128): (64, 128, 1024), (64, 64): (64, 64, 1024)}


def case_id(c):
    pro = {PRO_RAW: "raw", PRO_BNRELU: "bnrelu"}[c.pro]
    epi = {EPI_FWD: "fwd", EPI_DGRAD: "dgrad", EPI_RAW: "rawout", EPI_BNRELU: "bnreluout"}[c.epi]
    return f"{c.cls}-K{c.K}xN{c.Ncols}-{pro}-{epi}-{c.variant}-N{c.N}-cps{c.cps}"


def flags_of(case):
    """What the variant sets: bias, scene_bias, a_mask, pool, es with the pool, stats, C."""
    v, fwd = case.variant, case.epi == EPI_FWD
    return dict(bias=v in ("bias", "both", "mask", "pool", "pool_es", "mask_pool", "nostats", "nullC"),
                scene_bias=v in ("scene_bias", "both"), mask=v in ("mask", "mask_pool"),
                pool=fwd and v in ("pool", "pool_es", "mask_pool", "nullC"), pool_es=v == "pool_es",
                stats=(fwd and v != "nostats") or (case.epi == EPI_BNRELU and v != "nostats"
                                                   and case.cls in ("big", "stream")),
                C=v != "nullC")


def kernel_of(case):
    """The kernel instantiation pcs_gemm dispatches the case to, as a kernel trace prints it."""
    f = flags_of(case)
    tf = lambda b: "true" if b else "false"   # noqa: E731
    mask = tf(f["mask"] and case.pro == PRO_BNRELU)
    if case.cls == "big":
        return f"gemm_big_kernel<{case.pro}, {case.epi}, {mask}, false>"
    if case.cls == "stream":
        return f"fwd_stream_kernel<{case.K}, {case.Ncols}, {case.epi}, {mask}, {tf(f['scene_bias'])}, false, false>"
    T = "float" if case.cls == "f32" else "unsigned short"
    return (f"gemm_nt_kernel<{T}, 128, {128 if case.Ncols % 128 == 0 else 64}, {case.pro}, {case.epi}, {tf(f['pool'])}, "
            f"{mask}, false>")


def tile_of(case):
    return 128 if case.cls in ("f32", "bf16g") else 256


def geometry(case):
    """(chunks_per_scene, rows_per_chunk) of pcs_gemm_geometry for the case."""
    tile = tile_of(case)
    if case.cls in ("f32", "bf16g"):
        target, ncb = 2048, max(case.Ncols // 128, 1)
    elif case.cls == "stream":
        _, nb, target = STREAM[(case.K, case.Ncols)]
        ncb = case.Ncols // nb
    else:
        target, ncb = 256, case.Ncols // 256
    tps = -(-case.N // tile)
    cps = case.cps if case.cps > 0 else -(-target // (B * ncb))
    cps = max(min(cps, tps), 1)
    tpc = -(-tps // cps)
    return -(-tps // tpc), tpc * tile


# ---------------------------------------------------------------------------------------
# the forward epilogues
# ---------------------------------------------------------------------------------------
def fwd_ref(op, W, bias, scene_bias, es, et, epi, dtype, epi_relu=True, folded=False):
    """C of PCS_EPI_FWD / PCS_EPI_BNRELU / PCS_EPI_RAW on the staged operand op (x_operand's dict):
    the unrounded value and the bound e_C on |stored - C| (module docstring).  W [Ncols, K], bias
    [Ncols], scene_bias [B, Ncols] (it wins over bias), es / et [Ncols] (EPI_BNRELU only).
    folded=True bounds EPI_BNRELU as the streaming kernel evaluates it, the bias folded into the
    shift; every other kernel adds the bias to the accumulator first.  epi_relu=False drops the
    epilogue's ReLU (a perturbed reference of the sensitivity tests)."""
    W = f64(W)
    x, xe = op["v"], op["err"]
    acc = x @ W.T
    e = sum_bound(W.shape[1], np.abs(x) @ np.abs(W).T) * SLACK + xe @ np.abs(W).T
    v = acc
    if epi != EPI_RAW:
        b = f64(scene_bias)[:, None, :] if scene_bias is not None else f64(bias)
        e_y = e
        if b is not None:
            v = acc + b
            e_y = e + U * np.abs(v) * SLACK
        if epi == EPI_BNRELU:
            es, et = f64(es), f64(et)
            z = v * es + et
            e_z = np.abs(es) * e_y + U * np.abs(z) * SLACK
            if folded and b is not None:       # the bias folded into the shift
                e_z = np.abs(es) * e + U * (np.abs(b * es) + np.abs(et + b * es) + np.abs(z)) * SLACK
            v, e = (np.maximum(z, 0.0) if epi_relu else z), e_z
        else:
            e = e_y
    if dtype != "f32":
        e = e + BF16_U * (np.abs(v) + e)
    return dict(C=v, e_C=e, x=x, flagged=float(op["flag"].mean()))


def stored(v, dtype):
    """v as the storage dtype holds it (fp64 array)."""
    return R._stored(v, dtype)


def stats_ref(C, cps, rpc, epi, row=None, boundary=0):
    """Per-chunk statistics [B * cps, Ncols] of stored values C [B, N, Ncols] with their bounds:
    (mean, M2) for EPI_FWD, (sum, 0) for EPI_BNRELU.  Perturbed references of the sensitivity
    tests: row = (n, w) counts row n of every scene w times (0 drops it, 2 doubles it), boundary
    moves the first chunk boundary by that many rows."""
    C = f64(C)
    Bn, N, Nc = C.shape
    if row is not None:
        n, w = row
        C = np.delete(C, n, axis=1) if w == 0 else np.insert(C, n, C[:, n], axis=1)
        N = C.shape[1]
        assert (cps - 1) * rpc < N <= cps * rpc, "the perturbed row count keeps the chunking"
    if boundary:
        assert cps > 1
        parts = [stats_ref(C[:, :rpc + boundary], 1, rpc + boundary, epi),
                 stats_ref(C[:, rpc + boundary:], cps - 1, rpc, epi)]
        out = {}
        for k in parts[0]:
            out[k] = np.concatenate([p[k].reshape(Bn, -1, Nc) for p in parts], axis=1).reshape(Bn * cps, Nc)
        return out
    if epi == EPI_FWD:
        w = welford_partials(C, cps, rpc, rounded=False)
        return dict(mean=w[..., 0], e_mean=np.full(w[..., 0].shape, 1e-5 * np.abs(C).max()),
                    M2=w[..., 1], e_M2=1e-4 * w[..., 1])
    zero = np.zeros_like(C)
    s = sum_partials(C, zero, cps, rpc, rounded=False)[..., 0]
    sa = sum_partials(np.abs(C), zero, cps, rpc, rounded=False)[..., 0]
    n = np.repeat(np.array([hi - lo for lo, hi in chunk_bounds(N, cps, rpc)], np.float64)[None], Bn, 0).reshape(-1, 1)
    return dict(mean=s, e_mean=sum_bound(n, sa), M2=np.zeros_like(s), e_M2=np.zeros_like(s))


def pool_ref(C, cps, rpc, last=False):
    """The (max, argmax, min, argmin) records of stored values C: small_refs.pool_partials.
    last=True names the last occurrence of the extremum (a perturbed reference)."""
    rec = pool_partials(C, cps, rpc)
    if last:
        y = np.asarray(C, np.float32)
        Bn, N, Nc = y.shape
        idx = rec.view(np.int32).reshape(Bn, cps, Nc, 4)
        base = (np.arange(Bn, dtype=np.int64) * N)[:, None]
        for j, (lo, hi) in enumerate(chunk_bounds(N, cps, rpc)):
            idx[:, j, :, 1] = base + hi - 1 - y[:, lo:hi][:, ::-1].argmax(1)
            idx[:, j, :, 3] = base + hi - 1 - y[:, lo:hi][:, ::-1].argmin(1)
    return rec


# ---------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------
def _generic_cases(cls):
    ks = 16 if cls == "f32" else 32
    P, Rw, F = PRO_BNRELU, PRO_RAW, EPI_FWD
    out = [FCase(cls, 128, 64, P, F, v, 133, 0) for v in FWD_VARIANTS]                 # every variant, 64-column tile
    out += [FCase(cls, 64, 128, Rw, F, v, 133, 0) for v in FWD_VARIANTS if "mask" not in v]   # 128-column tile
    for sh, vp, vr in (((ks, 64), "mask_pool", "pool_es"), ((64, 64), "both", "bias"), ((64, 128), "mask_pool", None),
                       ((128, 64), None, "both"), ((128, 256), "mask", "scene_bias"), ((1024, 64), "mask_pool", "both")):
        if vp:
            out.append(FCase(cls, *sh, P, F, vp, 133, 0))
        if vr:
            out.append(FCase(cls, *sh, Rw, F, vr, 133, 0))
    out += [FCase(cls, 64, 128, P, F, v, 133, 0) for v in ("bias", "pool")]            # 128-column tile, no dropout bits
    for sh, vp, vr in (((ks, 64), "bias", "plain"), ((64, 128), "mask", "bias"), ((1024, 64), "mask", "bias")):
        out += [FCase(cls, *sh, P, EPI_BNRELU, vp, 133, 0), FCase(cls, *sh, Rw, EPI_BNRELU, vr, 133, 0)]
    out.append(FCase(cls, 64, 128, P, EPI_BNRELU, "plain", 133, 0))
    out += [FCase(cls, ks, 64, P, EPI_RAW, "mask", 133, 0), FCase(cls, 64, 64, P, EPI_RAW, "plain", 133, 0),
            FCase(cls, 64, 128, P, EPI_RAW, "plain", 133, 0), FCase(cls, 128, 256, P, EPI_RAW, "mask", 133, 0)]
    for pro in (P, Rw):
        out += [FCase(cls, 64, 128, pro, EPI_DGRAD, v, 133, 0) for v in DGRAD_VARIANTS]
        out += [FCase(cls, 128, 64, pro, EPI_DGRAD, v, 133, 0) for v in ("plain", "cmask_addend")]
        out.append(FCase(cls, ks, 64, pro, EPI_DGRAD, "bias", 133, 0))
    out += [FCase(cls, 128, 64, P, F, "mask_pool", n, 0) for n in (1, 127, 128, 129, 2 * 128 + 5)]
    out.append(FCase(cls, 128, 64, P, F, "mask_pool", 2 * 128 + 5, 2))
    return out


def _big_cases():
    # bf16, default flags, wide class (K % 64 == 0, 128 <= K <= 1024, Ncols % 256 == 0), on
    # gemm_big_kernel because every kernel asked before it turns the call away:
    #   pcs_fwd_stream_applicable: (128, 256), (256, 256), (128, 512) are no FsShape pairs (and PRO_RAW
    #                              is not its prologue);
    #   pcs_gemm_wres_applicable:  needs PCS_FLAG_C_FP8;
    #   pcs_gemm_glds_applicable:  PRO_RAW only, and its EPI_FWD only with C == NULL: PRO_BNRELU, or
    #                              PRO_RAW with C set (or EPI_BNRELU), is not taken.
    P, Rw, F = PRO_BNRELU, PRO_RAW, EPI_FWD
    out = [FCase("big", 128, 256, P, F, v, 257, 0) for v in FWD_VARIANTS]
    out += [FCase("big", 256, 256, P, F, "mask_pool", 257, 0), FCase("big", 256, 256, P, F, "scene_bias", 257, 0),
            FCase("big", 128, 512, P, F, "both", 257, 0), FCase("big", 128, 512, P, F, "pool_es", 257, 0)]
    out += [FCase("big", 256, 256, Rw, F, v, 257, 0) for v in ("plain", "bias", "pool", "both")]
    out += [FCase("big", 128, 256, P, EPI_BNRELU, v, 257, 0) for v in ("plain", "mask", "nostats")]
    out += [FCase("big", 256, 256, Rw, EPI_BNRELU, "bias", 257, 0)]
    out += [FCase("big", 128, 256, P, F, "mask_pool", n, 0) for n in (255, 256, 3 * 256 + 7)]
    out.append(FCase("big", 128, 256, P, F, "mask_pool", 3 * 256 + 7, 2))
    return out


def _stream_cases():
    # bf16, default flags, PRO_BNRELU: the six FsShape pairs with the operands each accepts
    P, F = PRO_BNRELU, EPI_FWD
    out = [FCase("stream", 64, 512, P, F, v, 133, 0) for v in ("plain", "bias", "scene_bias", "both", "nostats")]
    out += [FCase("stream", 512, 256, P, F, v, 133, 0) for v in ("plain", "bias", "mask")]
    out += [FCase("stream", 256, 128, P, F, v, 133, 0) for v in ("plain", "mask")]
    out += [FCase("stream", 64, 128, P, F, "bias", 133, 0), FCase("stream", 64, 64, P, F, "plain", 133, 0),
            FCase("stream", 64, 64, P, F, "bias", 133, 0)]
    out += [FCase("stream", 128, 1024, P, EPI_BNRELU, v, 133, 0) for v in ("plain", "bias", "nostats")]
    for (K, Nc, v) in ((512, 256, "mask"), (64, 512, "scene_bias")):
        ms = STREAM[(K, Nc)][0]
        out += [FCase("stream", K, Nc, P, F, v, n, 0) for n in (1, ms - 1, ms + 1)]
        out.append(FCase("stream", K, Nc, P, F, v, 256 + 2 * ms + 5, 2))
    out.append(FCase("stream", 128, 1024, P, EPI_BNRELU, "plain", 3 * 256 + 7, 0))      # 3 x 775 x 1024
    return out


def _seam_cases():
    # bf16, default flags, wide class (256-row-multiple chunks) at (256, 256); pcs_gemm_big_applicable
    # takes EPI_RAW and EPI_DGRAD only with PRO_BWD, pcs_gemm_glds_applicable its EPI_DGRAD only with
    # Yp == A and no es: gemm_nt_kernel<bf16_t> walks the chunks in 128-row tiles
    P = PRO_BNRELU
    out = [FCase("seam", 256, 256, P, EPI_RAW, v, 257, 0) for v in ("plain", "mask")]
    out += [FCase("seam", 256, 256, P, EPI_DGRAD, v, 257, 0) for v in DGRAD_VARIANTS]
    out.append(FCase("seam", 256, 256, PRO_RAW, EPI_DGRAD, "plain", 257, 0))
    out += [FCase("seam", 256, 256, P, EPI_RAW, "mask", n, 0) for n in (255, 256, 3 * 256 + 7)]
    out.append(FCase("seam", 256, 256, P, EPI_RAW, "mask", 3 * 256 + 7, 2))
    out.append(FCase("seam", 256, 256, P, EPI_DGRAD, "cmask_addend", 3 * 256 + 7, 2))
    return out


FWD_CASES = _generic_cases("f32") + _generic_cases("bf16g") + _big_cases() + _stream_cases() + _seam_cases()
assert len(set(FWD_CASES)) == len(FWD_CASES)


# ---------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------
def fwd_data(case, kind):
    """Operands of one case; what the variant does not set is None.

    exact: integers, s = 1, keep_scale = 2, eight +-1 entries per row of W (one row all zero), so
    |x| <= 12, every partial sum of |x| |W| <= 96, |y| <= 112, |y es + et| <= 232 and (EPI_DGRAD)
    the stored dz <= 256: every staged, summed and stored value is exact in bf16 and fp32.  Outputs
    tie often.
    value: Gaussian data; A s + t is exactly 0 (A = t = 0) in some places and at least ZGAP away
    from 0 everywhere else; one row of W is 0, so that output column is constant (= the bias) and,
    for EPI_BNRELU, its y es + et is exactly 0 while every other y es + et is at least ZGAP from 0
    (et is moved into a free interval, _gapped_shift); with a bias, one 8-column block in 16 is offset by 16
    (standard deviations of y, about)."""
    r = np.random.default_rng(R._seed(case, kind))
    dt = dtype_of(case)
    N, K, Nc = case.N, case.K, case.Ncols
    f = flags_of(case)
    exact = kind == "exact"
    f32 = lambda a: f64(np.asarray(a, np.float32))   # noqa: E731
    d = dict.fromkeys(("s", "t", "keep", "bias", "scene_bias", "es", "et", "addend", "Yp", "mean", "rstd", "ckeep"))
    d.update(keep_scale=1.0, c_keep_scale=1.0)
    # ---- operand
    if case.pro == PRO_RAW:
        d["A"] = 1.0 * r.integers(-12, 13, (B, N, K)) if exact else stored(r.standard_normal((B, N, K)), dt)
    elif exact:
        d.update(A=1.0 * r.integers(-4, 5, (B, N, K)), s=np.ones(K), t=1.0 * r.integers(-2, 3, K))
    else:
        s = f32(r.uniform(0.5, 1.5, K) * np.where(r.random(K) < 0.25, -1.0, 1.0))
        t = f32(0.3 * r.standard_normal(K))
        t[::16] = 0.0
        A = stored(r.standard_normal((B, N, K)), dt)
        z = A * s + t
        A = np.where(np.abs(z) < ZGAP, stored((np.where(z >= 0, 0.05, -0.05) - t) / s, dt), A)
        A[:, :, ::16] = np.where(r.random((B, N, len(t[::16]))) < 0.05, 0.0, A[:, :, ::16])
        A[:, 0, ::16] = 0.0
        d.update(A=A, s=s, t=t)
    if f["mask"]:
        d.update(keep=r.random((B, N, K)) < (0.5 if exact else 0.7), keep_scale=2.0 if exact else float(np.float32(1 / 0.7)))
    # ---- W and the epilogue operands
    zc = Nc - 3                                       # the all-zero row of W
    if case.epi == EPI_DGRAD:
        gv = "plain" if case.variant == "bias" else case.variant
        g = R.gemm_data(R.GCase(case.cls, K, Nc, EPI_DGRAD, gv, N, case.cps), kind)
        d.update(W=g["W"], addend=g["addend"], Yp=g["Yp"], es=g["es"], et=g["et"], mean=g["mean"], rstd=g["rstd"],
                 ckeep=g["keep"], c_keep_scale=g["keep_scale"])
        if case.variant == "bias":
            d["bias"] = 1.0 * r.integers(-16, 17, Nc) if exact else f32(0.1 * r.standard_normal(Nc))
        return d
    if exact:
        W = np.zeros((Nc, K))
        for n in range(Nc):
            W[n, r.choice(K, 8, replace=False)] = r.choice([-1.0, 1.0], 8)
        bias, sb = 1.0 * r.integers(-16, 17, Nc), 1.0 * r.integers(-16, 17, (B, Nc))
        es, et = r.choice([1.0, -1.0, 2.0], Nc), 1.0 * r.integers(-8, 9, Nc)
    else:
        W = stored(r.standard_normal((Nc, K)) / np.sqrt(K), dt)
        off = np.where((np.arange(Nc) // 8) % 16 == 1, 16.0, 0.0)
        bias, sb = f32(0.1 * r.standard_normal(Nc) + off), f32(0.3 * r.standard_normal((B, Nc)) + off)
        es = f32(r.uniform(0.5, 1.5, Nc) * np.where(r.random(Nc) < 0.25, -1.0, 1.0))
        et = f32(0.5 * r.standard_normal(Nc))
    W[zc] = 0.0
    d["W"] = W
    if f["bias"]:
        d["bias"] = bias
    if f["scene_bias"]:
        d["scene_bias"] = sb
    if case.epi == EPI_BNRELU or f["pool_es"]:
        if case.epi == EPI_BNRELU:
            if not exact:
                y = fwd_ref(fwd_operand(case, d), W, d["bias"], None, None, None, EPI_FWD, "f32")["C"]
                et = f32(_gapped_shift(y.reshape(-1, Nc) * es, et))
            es[zc] = -1.0 if es[zc] < 0 else 1.0     # y es + et = 0 exactly in the constant column
            et[zc] = -(bias[zc] if f["bias"] else 0.0) * es[zc]
        d.update(es=es, et=et)
    return d


def _gapped_shift(ye, et, gap=1.5 * ZGAP):
    """et moved, per column and as little as possible, to where no ye + et lies within gap of 0."""
    et = et.copy()
    for c in range(ye.shape[1]):
        u = np.sort(-ye[:, c])
        if np.abs(u - et[c]).min() >= gap:
            continue
        lo = np.concatenate([[-np.inf], u + gap])          # the free intervals between the -ye
        hi = np.concatenate([u - gap, [np.inf]])
        ok = hi >= lo
        cand = np.clip(et[c], lo[ok], hi[ok])
        et[c] = cand[np.argmin(np.abs(cand - et[c]))]
    return et


def fwd_operand(case, d, pro_relu=True, pre_round=False):
    """The staged operand.  pro_relu=False drops the prologue's ReLU, pre_round=True rounds x to
    bf16 before the keep scale (perturbed references of the sensitivity tests)."""
    dt = dtype_of(case)
    if case.pro == PRO_RAW or (pro_relu and not pre_round):
        return R.x_operand(d["A"], d["s"], d["t"], d["keep"], d["keep_scale"], case.pro, dt,
                           folded=case.cls == "stream")
    x = d["A"] * d["s"] + d["t"]
    x = np.maximum(x, 0.0) if pro_relu else x
    if pre_round:
        x = bf16_round(x)
    if d["keep"] is not None:
        x = x * d["keep"] * d["keep_scale"]
    return R._stage(x, 2.0 * U * np.abs(x), dt)


def fwd_reference(case, d, pro_relu=True, pre_round=False, epi_relu=True, **kw):
    op = fwd_operand(case, d, pro_relu, pre_round)
    dt = dtype_of(case)
    if case.epi == EPI_DGRAD:
        out = R.dgrad_from(op, d["W"], d["addend"], d["Yp"], d["es"], d["et"], d["ckeep"], d["c_keep_scale"],
                           d["mean"], d["rstd"], dt, bias=d["bias"], **kw)
        out["x"] = op["v"]
        return out
    return fwd_ref(op, d["W"], d["bias"], d["scene_bias"], d["es"], d["et"], case.epi, dt, epi_relu=epi_relu,
                   folded=case.cls == "stream")
