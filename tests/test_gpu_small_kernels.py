"""The glue kernels of csrc/small.hip, each on its own through the C ABI against the fp64
references of tests/small_refs.py (proved against torch in tests/test_small_refs.py): BatchNorm
finalize (forward, backward, eval), max-pool finalize and backward, the per-scene GEMV, the
partial reductions, weight casts and the Adam step.  All inputs are synthetic, so every regime
of these kernels is reached directly: more than 256 chunks per scene, more than 8 scenes in
the pool backward, every kernel switch of the reductions, ragged sizes.

Bounds (none tuned on GPU output): selections, casts and integer sums are exact; the finalize
kernels work in fp64 and round once (2^-23 relative, or 2^-23 of the sum of the absolute terms
of a difference); fp32 sums get terms * 2^-24 * sum|terms|, propagated linearly."""
import ctypes as ct
import itertools

import numpy as np
import pytest
import torch

import small_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F32 = np.float32
MOM, EPS = float(F32(0.1)), float(F32(1e-5))     # the fp32 values the kernels receive


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def nans(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def rng(*key):
    return np.random.default_rng(list(key))


# (B, N, cps, rpc): one chunk; a ragged last chunk of 104 rows; 301 chunks per scene (the
# 256-thread chunk loop wraps, ragged last chunk of 5 rows); the Gram-statistics form
BN_CASES = [(1, 37, 1, 37), (3, 1000, 8, 128), (2, 300 * 7 + 5, 301, 7), (2, 4096, 1, 4096)]


def _activation(r, B, N, C):
    off = r.uniform(0.5, 3.0, C) * r.choice([-1.0, 1.0], C)      # means well away from 0
    return r.standard_normal((B, N, C)) * r.uniform(0.5, 2.0, C) + off


@pytest.mark.parametrize("C", [64, 24])
@pytest.mark.parametrize("B,N,cps,rpc", BN_CASES)
def test_bn_fwd_finalize(B, N, cps, rpc, C):
    import pcs_amd._lib as L
    r = rng(1, N, C)
    st = R.welford_partials(_activation(r, B, N, C), cps, rpc)
    gamma, beta, moff = (r.standard_normal(C).astype(F32) for _ in range(3))
    rm0, rv0 = r.standard_normal(C).astype(F32), r.uniform(0.5, 1.5, C).astype(F32)
    d_st, d_g, d_b, d_moff = dev(st), dev(gamma), dev(beta), dev(moff)
    for use_moff, update, use_ss in itertools.product([False, True], repeat=3):
        rm, rv = dev(rm0), dev(rv0)
        mean, rstd, scale, shift = (nans(C) for _ in range(4))
        ss = nans(B, C)
        L.call("pcs_bn_fwd_finalize", L.ptr(d_st), B, N, C, cps, rpc, L.ptr(d_g), L.ptr(d_b),
               L.ptr(d_moff) if use_moff else None, L.ptr(rm), L.ptr(rv), 0.1, 1e-5, int(update), L.ptr(mean),
               L.ptr(rstd), L.ptr(scale), L.ptr(shift), L.ptr(ss) if use_ss else None, L.stream_ptr())
        torch.cuda.synchronize()
        ref = R.bn_fwd_from_partials(st, B, N, cps, rpc, gamma, beta, moff if use_moff else None, rm0, rv0, MOM, EPS)
        tag = f"moff={use_moff} update={update} scene_sum={use_ss}"
        for name, got in (("mean", mean), ("rstd", rstd), ("scale", scale)):
            R.assert_within(host(got), ref[name], R.round_bound(ref[name]), f"{name} {tag}")
        R.assert_within(host(shift), ref["shift"], R.ULP * ref["shift_terms"], f"shift {tag}")
        if use_ss:
            R.assert_within(host(ss), ref["scene_sum"], R.round_bound(ref["scene_sum"]), f"scene_sum {tag}")
        else:
            assert torch.isnan(ss).all()
        if update:
            R.assert_within(host(rm), ref["rmean"], R.ULP * ref["rmean_terms"], f"running_mean {tag}")
            R.assert_within(host(rv), ref["rvar"], R.round_bound(ref["rvar"]), f"running_var {tag}")
        else:
            assert np.array_equal(host(rm).view(np.int32), rm0.view(np.int32)), tag
            assert np.array_equal(host(rv).view(np.int32), rv0.view(np.int32)), tag


@pytest.mark.parametrize("C", [64, 24])
@pytest.mark.parametrize("B,N,cps,rpc", BN_CASES)
def test_bn_bwd_finalize(B, N, cps, rpc, C):
    import pcs_amd._lib as L
    r = rng(2, N, C)
    y = _activation(r, B, N, C)
    mean = y.reshape(-1, C).mean(0).astype(F32)
    rstd = (1.0 / np.sqrt(y.reshape(-1, C).var(0) + EPS)).astype(F32)
    gamma = r.standard_normal(C).astype(F32)
    dz = r.standard_normal((B, N, C)) * (r.random((B, N, C)) < 0.6)            # a ReLU-masked gradient
    st = R.sum_partials(dz, (y - mean.astype(np.float64)) * rstd.astype(np.float64), cps, rpc)
    ssum = y.sum(1).astype(F32)
    d_st, d_m, d_r, d_g, d_ss = dev(st), dev(mean), dev(rstd), dev(gamma), dev(ssum)
    for use_ss, extras in itertools.product([False, True], repeat=2):
        alpha, beta_c, gamma_c, dgamma, dbeta, dbias = (nans(C) for _ in range(6))
        s1 = nans(B, C)
        opt = [L.ptr(dgamma), L.ptr(dbeta)] if extras else [None, None]
        L.call("pcs_bn_bwd_finalize", L.ptr(d_st), B, N, C, cps, L.ptr(d_m), L.ptr(d_r), L.ptr(d_g),
               L.ptr(d_ss) if use_ss else None, L.ptr(alpha), L.ptr(beta_c), L.ptr(gamma_c), opt[0], opt[1],
               L.ptr(dbias), L.ptr(s1) if extras else None, L.stream_ptr())
        torch.cuda.synchronize()
        ref = R.bn_bwd_from_partials(st, B, N, cps, mean, rstd, gamma, ssum if use_ss else None)
        tag = f"scene_sum={use_ss} extras={extras}"
        R.assert_within(host(alpha), ref["alpha"], R.round_bound(ref["alpha"]), f"alpha {tag}")
        R.assert_within(host(gamma_c), ref["gamma_c"], R.round_bound(ref["gamma_c"]), f"gamma_c {tag}")
        R.assert_within(host(beta_c), ref["beta_c"], R.ULP * ref["beta_c_terms"], f"beta_c {tag}")
        if use_ss:
            R.assert_within(host(dbias), ref["dbias"], R.ULP * ref["dbias_terms"], f"dbias {tag}")
        else:
            assert (dbias == 0).all(), tag
        if extras:
            R.assert_within(host(dgamma), ref["dgamma"], R.round_bound(ref["dgamma"]), f"dgamma {tag}")
            R.assert_within(host(dbeta), ref["dbeta"], R.round_bound(ref["dbeta"]), f"dbeta {tag}")
            R.assert_within(host(s1), ref["scene_s1"], R.round_bound(ref["scene_s1"]), f"scene_s1 {tag}")
        else:
            assert torch.isnan(dgamma).all() and torch.isnan(dbeta).all() and torch.isnan(s1).all()


@pytest.mark.parametrize("use_moff", [False, True])
@pytest.mark.parametrize("C", [1, 64, 300])
def test_bn_eval_coefs(C, use_moff):
    import pcs_amd._lib as L
    r = rng(3, C)
    gamma, beta, rm, moff = (r.standard_normal(C).astype(F32) for _ in range(4))
    rv = r.uniform(0.01, 2.0, C).astype(F32)
    scale, shift = nans(C + 3), nans(C + 3)
    d = [dev(a) for a in (gamma, beta, rm, rv, moff)]
    L.call("pcs_bn_eval_coefs", L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.ptr(d[3]), L.ptr(d[4]) if use_moff else None,
           1e-5, C, L.ptr(scale), L.ptr(shift), L.stream_ptr())
    torch.cuda.synchronize()
    ref = R.bn_eval_ref(gamma, beta, rm, rv, moff if use_moff else None, EPS)
    R.assert_within(host(scale)[:C], ref["scale"], R.round_bound(ref["scale"]), "scale")
    R.assert_within(host(shift)[:C], ref["shift"], R.ULP * ref["shift_terms"], "shift")
    assert torch.isnan(scale[C:]).all() and torch.isnan(shift[C:]).all()       # nothing past C


# ---------------------------------------------------------------------------------------
# global max-pool
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [12, 300])
def test_pool_finalize(C):
    import pcs_amd._lib as L
    B, N, cps, rpc = 3, 40, 4, 10
    r = rng(4, C)
    y = r.integers(-3, 4, (B, N, C)).astype(F32)          # small integers: ties within and across chunks
    y[:, :, 0] = 0.0
    y[:, 5, 0] = y[:, 25, 0] = 7.0                        # the max in chunks 0 and 2: row 5 must win
    y[:, 7, 1] = y[:, 36, 1] = -7.0                       # the min likewise (column 1 gets s < 0)
    pool = R.pool_partials(y, cps, rpc)
    rec = pool.reshape(B, cps, C, 4)
    for c in (2, 3):                                      # no candidate in any chunk: all sentinels
        rec[:, :, c, 0], rec[:, :, c, 2] = -np.inf, np.inf
        rec.view(np.int32)[:, :, c, 1] = rec.view(np.int32)[:, :, c, 3] = R.POOL_NONE
    s = r.standard_normal(C).astype(F32)
    s[0], s[1], s[2], s[3] = 0.5, -0.5, 1.5, -1.5
    s[4::4] = 0.0                                         # scale == 0: the scene's first row
    s[5::4] = -np.abs(s[5::4])
    assert (s > 0).any() and (s < 0).any() and (s == 0).any()
    t = r.standard_normal(C).astype(F32)
    g, ysel = nans(B, C), nans(B, C)
    am = torch.full((B, C), -5, dtype=torch.int32, device=DEV)
    d_pool, d_s, d_t = dev(pool), dev(s), dev(t)
    L.call("pcs_pool_finalize", L.ptr(d_pool), B, N, C, cps, L.ptr(d_s), L.ptr(d_t), L.ptr(g), L.ptr(am),
           L.ptr(ysel), L.stream_ptr())
    torch.cuda.synchronize()
    ref = R.pool_finalize_ref(pool, B, N, cps, s, t)
    got_am = host(am).astype(np.int64)
    assert np.array_equal(got_am, ref["am"])
    base = (np.arange(B) * N)[:, None]
    assert ((got_am >= base) & (got_am < base + N)).all()
    assert (got_am[:, s == 0] == base).all() and (got_am[:, 2:4] == base).all()
    assert (got_am[:, 0] == base[:, 0] + 5).all() and (got_am[:, 1] == base[:, 0] + 7).all()
    assert np.array_equal(host(ysel).view(np.int32), ref["ysel"].view(np.int32))
    fin = np.isfinite(ref["z"])
    assert fin[:, 4:].all() and not fin[:, 2:4].any()
    # g = relu(fmaf(y, s, t)): one rounding of the exact y*s + t
    R.assert_within(host(g)[fin], ref["g"][fin], R.U * np.abs(ref["z"][fin]) + 2.0 ** -149, "g")
    assert (host(g)[~fin] == 0).all()                     # relu(-inf)


def _pool_bwd_inputs(r, B, N, Cs, Cg, col_off, ldw):
    f = lambda *s: r.standard_normal(s).astype(F32)       # noqa: E731
    d = dict(s1_alpha=f(Cs), s1_beta=f(Cs) * F32(0.1), s1_gamma=f(Cs) * F32(0.1), s1_scene_s1=f(B, Cs) * F32(3),
             s1_scene_sum=f(B, Cs) * F32(5), W_s1=f(Cs, ldw) * F32(0.1), g=np.maximum(f(B, Cg), 0),
             ysel=f(B, Cg), g_mean=f(Cg) * F32(0.3), g_rstd=r.uniform(0.5, 2.0, Cg).astype(F32), g_gamma=f(Cg),
             g_scene_sum=f(B, Cg) * F32(N))
    return d


def _pool_bwd_call(L, d, B, N, Cs, Cg, col_off, ldw):
    t = {k: dev(v) for k, v in d.items()}
    out = dict(dW_s1_global=torch.full((Cs, ldw), -777.0, device=DEV), csum=nans(B, Cs), alpha=nans(Cg),
               beta_c=nans(Cg), gamma_c=nans(Cg), dgamma=nans(Cg), dbeta=nans(Cg), dbias=nans(Cg), sp=nans(B, Cg))
    a = L.PoolBwdArgs(num_scenes=B, scene_rows=N, Cs=Cs, Cg=Cg, col_off=col_off, ldw=ldw)
    for k, v in {**t, **out}.items():
        setattr(a, k, v.data_ptr())
    return a, t, out


@pytest.mark.parametrize("B,Cs,Cg", [(1, 512, 1024), (8, 512, 1024), (9, 512, 1024), (17, 40, 100), (64, 64, 64)])
def test_pool_bwd(B, Cs, Cg):
    """B = 9 and 17 take a second and third pass of 8 scenes over the reused LDS staging, 64 is
    the LDS limit; (40, 100) and (64, 64) leave the model's 512 / 1024 channels (a ragged
    last block of 64 columns, uneven 16-way splits of the Cs reduction)."""
    import pcs_amd._lib as L
    N, col_off = 37, 64
    ldw = col_off + Cg + 3
    d = _pool_bwd_inputs(rng(5, B, Cs, Cg), B, N, Cs, Cg, col_off, ldw)
    a, keep, out = _pool_bwd_call(L, d, B, N, Cs, Cg, col_off, ldw)
    L.call("pcs_pool_bwd", ct.byref(a), L.stream_ptr())
    torch.cuda.synchronize()
    ref, err = R.pool_bwd_ref(N, d["s1_alpha"], d["s1_beta"], d["s1_gamma"], d["s1_scene_s1"], d["s1_scene_sum"],
                              d["W_s1"], col_off, d["g"], d["ysel"], d["g_mean"], d["g_rstd"], d["g_gamma"],
                              d["g_scene_sum"])
    dW = host(out["dW_s1_global"])
    assert (dW[:, :col_off] == -777.0).all() and (dW[:, col_off + Cg:] == -777.0).all()
    R.assert_within(dW[:, col_off:col_off + Cg], ref["dW"], err["dW"], "dW")
    for k in ("csum", "sp", "alpha", "beta_c", "gamma_c", "dgamma", "dbeta", "dbias"):
        worst = R.assert_within(host(out[k]), ref[k], err[k], k)
        print(f"pool_bwd B={B} {k}: worst error / bound = {worst:.3f}")
    assert (host(out["sp"])[d["g"] == 0] == 0).all()


def test_pool_bwd_refuses_65_scenes():
    import pcs_amd._lib as L
    B, N, Cs, Cg, col_off = 65, 37, 64, 64, 64
    ldw = col_off + Cg + 3
    d = _pool_bwd_inputs(rng(6), B, N, Cs, Cg, col_off, ldw)
    a, keep, out = _pool_bwd_call(L, d, B, N, Cs, Cg, col_off, ldw)
    with pytest.raises(L.PcsError):
        L.call("pcs_pool_bwd", ct.byref(a), L.stream_ptr())
    torch.cuda.synchronize()
    assert (out["dW_s1_global"] == -777.0).all()
    for k, v in out.items():
        if k != "dW_s1_global":
            assert torch.isnan(v).all(), k


@pytest.mark.parametrize("use_bias,use_offset", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("B,Kg,Nout", [(1, 1024, 512), (3, 100, 5), (4, 1, 65)])
def test_scene_gemv(B, Kg, Nout, use_bias, use_offset):
    import pcs_amd._lib as L
    r = rng(7, B, Kg, Nout)
    col_off = 3
    ldw = col_off + Kg + 5
    g = np.maximum(r.standard_normal((B, Kg)), 0).astype(F32)
    W = r.standard_normal((Nout, ldw)).astype(F32)
    bias = r.standard_normal(Nout).astype(F32)
    out, off = nans(B, Nout), nans(Nout)
    d_g, d_W, d_b = dev(g), dev(W), dev(bias)
    L.call("pcs_scene_gemv", L.ptr(d_g), B, Kg, L.ptr(d_W), ldw, col_off, L.ptr(d_b) if use_bias else None, Nout,
           L.ptr(out), L.ptr(off) if use_offset else None, L.stream_ptr())
    torch.cuda.synchronize()
    v, e = R.scene_gemv_ref(g, W, col_off, bias if use_bias else None)
    if not use_offset:
        R.assert_within(host(out), v, e, "out")
        assert torch.isnan(off).all()
        return
    # offset = the fp64 mean over the scenes of the fp32 v, rounded once; out = v - offset in
    # fp32, one more rounding (2^-24 |out|); out + offset is then the uncentred v
    o, m = host(out).astype(np.float64), host(off).astype(np.float64)
    R.assert_within(m, v.mean(0), e.mean(0) + R.round_bound(v.mean(0)), "offset")
    R.assert_within(o + m, v, e + R.U * np.abs(o), "out + offset")


# ---------------------------------------------------------------------------------------
# partial reductions: integer-valued partials, |sum| < 2^24, a power-of-two scale: every
# summation order is exact, so the result equals the fp64 sum bit for bit
# ---------------------------------------------------------------------------------------
def _int_partials(r, *shape):
    return r.integers(-8, 9, shape).astype(F32)


@pytest.mark.parametrize("length,row_len,ldo", [(4096, 4096, 4096), (192, 3, 3), (192, 3, 8), (387, 387, 387),
                                                (516, 516, 516)])
@pytest.mark.parametrize("nslabs", [1, 7, 8, 63, 64, 65, 1000])
def test_reduce_partials(nslabs, length, row_len, ldo):
    import pcs_amd._lib as L
    p = _int_partials(rng(8, nslabs, length, ldo), nslabs, length)
    rows = length // row_len
    out = torch.full((rows, ldo), -777.0, device=DEV)
    d_p = dev(p)
    L.call("pcs_reduce_partials", L.ptr(d_p), nslabs, length, 0.25, L.ptr(out), ldo, row_len, L.stream_ptr())
    torch.cuda.synchronize()
    ref = (p.astype(np.float64).sum(0) * 0.25).reshape(rows, row_len)
    assert np.abs(ref).max() * 4 < 2 ** 24
    got = host(out)
    assert np.array_equal(got[:, :row_len].astype(np.float64), ref)
    assert (got[:, row_len:] == -777.0).all()                      # the padding of an output row


@pytest.mark.parametrize("length", [2048, 4160])
@pytest.mark.parametrize("ngroups", [1, 3])
@pytest.mark.parametrize("nslabs", [5, 9, 70])
def test_reduce_partials_grouped(nslabs, ngroups, length):
    import pcs_amd._lib as L
    p = _int_partials(rng(9, nslabs, ngroups, length), ngroups, nslabs, length)
    out = torch.full((ngroups + 1, length), -777.0, device=DEV)
    d_p = dev(p)
    L.call("pcs_reduce_partials_grouped", L.ptr(d_p), ngroups, nslabs, length, 2.0, L.ptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    got = host(out)
    assert np.array_equal(got[:ngroups].astype(np.float64), p.astype(np.float64).sum(1) * 2.0)
    assert (got[ngroups] == -777.0).all()


# ---------------------------------------------------------------------------------------
# weight casts
# ---------------------------------------------------------------------------------------
def _special_f32():
    bits = np.array([0x3F808000,    # tie, even neighbour below: rounds down to 0x3F80
                     0x3F818000,    # tie, odd neighbour below: rounds up to 0x3F82
                     0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF,
                     0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
                     0x00000001, 0x80000001, 0x007FFFFF, 0x00008000, 0x00018000,   # fp32 subnormals (bf16 ties too)
                     0x7F7FFFFF, 0xFF7FFFFF,                                      # largest finite: rounds to inf
                     0x7FC00000, 0x7F800001, 0xFFC12345], np.uint32)                # NaNs
    return bits.view(F32)


def _same_bits(got, ref, what):
    """bit equality, NaNs compared with isnan (their payload is not part of the contract)"""
    g, e = got.float(), ref.float()
    assert torch.equal(torch.isnan(g), torch.isnan(e)), what
    ok = ~torch.isnan(e)
    gi = got.view(torch.int16 if got.dtype == torch.bfloat16 else torch.int32)
    ei = ref.view(torch.int16 if ref.dtype == torch.bfloat16 else torch.int32)
    assert torch.equal(gi[ok], ei[ok]), what


@pytest.mark.parametrize("which", ["Wc", "WcT", "both"])
@pytest.mark.parametrize("rows,cols,ldw", [(64, 3, 3), (512, 64, 1088), (5, 7, 7)])
def test_cast_and_round_weight(rows, cols, ldw, which):
    import pcs_amd._lib as L
    r = rng(10, rows, cols)
    W = np.full((rows, ldw), 12345.0, F32)
    W[:, :cols] = r.standard_normal((rows, cols)).astype(F32)
    sp = _special_f32()
    flat = [(i // cols, i % cols) for i in r.permutation(rows * cols)[:len(sp)]]
    for (i, j), v in zip(flat, sp):
        W[i, j] = v
    Wt = torch.from_numpy(W)
    d_W = Wt.to(DEV)
    for dt, tdt in ((L.BF16, torch.bfloat16), (L.F32, torch.float32)):
        want = Wt[:, :cols].to(tdt)
        Wc = torch.full((rows, cols), 9.0, dtype=tdt, device=DEV)
        WcT = torch.full((cols, rows), 9.0, dtype=tdt, device=DEV)
        L.call("pcs_cast_weight", L.ptr(d_W), rows, cols, ldw, dt, L.ptr(Wc) if which != "WcT" else None,
               L.ptr(WcT) if which != "Wc" else None, L.stream_ptr())
        torch.cuda.synchronize()
        if which != "WcT":
            _same_bits(Wc.cpu(), want, f"Wc {tdt}")
        else:
            assert (Wc == 9.0).all()
        if which != "Wc":
            _same_bits(WcT.cpu(), want.T.contiguous(), f"WcT {tdt}")
        else:
            assert (WcT == 9.0).all()
        # pcs_round_weight: the same rounding, widened back to fp32, over the whole buffer
        out = nans(rows * ldw + 2)
        L.call("pcs_round_weight", L.ptr(d_W), rows * ldw, dt, L.ptr(out), L.stream_ptr())
        torch.cuda.synchronize()
        _same_bits(out[:rows * ldw].cpu(), Wt.reshape(-1).to(tdt).float(), f"round_weight {tdt}")
        assert torch.isnan(out[rows * ldw:]).all()
        assert L.call("pcs_round_weight", L.ptr(d_W), 0, dt, L.ptr(out), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out[rows * ldw:]).all()


# ---------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------
HP = dict(lr=float(F32(1e-3)), b1=float(F32(0.9)), b2=float(F32(0.999)), eps=float(F32(1e-8)))


def _adam_check(tag, before, after, step, wd, scale):
    """``before`` / ``after``: (p, g, m, v) fp32 arrays around one pcs_adam call.  The reference
    starts from the same fp32 state.  Bounds, with u = 2^-24 and n_g the roundings the effective
    gradient gi = g*scale + wd*p carries (one for the scale product, one for adding wd*p):

    * exp_avg = b1*m + (1 - b1)*gi, both terms of one sign here: the products round once each
      and the sum once, so (n_g + 2) u <= 4 u relative;
    * exp_avg_sq = b2*v + (1 - b2)*gi*gi, terms >= 0: gi*gi doubles gi's error (2 n_g u), the
      two products round once each and the sum once: (2 n_g + 3) u relative.  That is 3 u for a
      plain gradient; 4 u, which ignores gi's own roundings, is exceeded on the GPU by up to
      1.21x as soon as a scale or a weight decay is set (211 of 100003 elements at step 1);
    * param: 2^-23 |p| + 16 u |lr/bc1 * m/denom| (the terms above, sqrt, two divisions, eps,
      the rounded bias corrections and the last product: 2 n_g + 11.5 roundings)."""
    p0, g0, m0, v0 = before
    p1, g1, m1, v1 = after
    n_g = int(scale is not None) + int(wd != 0)
    pr, mr, vr, ge, upd = R.adam_ref(p0, g0, m0, v0, step, HP["lr"], HP["b1"], HP["b2"], HP["eps"], wd, scale)
    if scale is None:
        assert np.array_equal(g1.view(np.int32), g0.view(np.int32)), f"{tag}: grad touched"
    else:   # the scaled gradient, written back: one fp32 product
        assert np.array_equal(g1.view(np.int32), (g0 * F32(scale)).astype(F32).view(np.int32)), f"{tag}: grad write-back"
    wm = R.assert_within(m1, mr, 4 * R.U * np.abs(mr), f"{tag} exp_avg")
    wv = R.assert_within(v1, vr, (2 * n_g + 3) * R.U * np.abs(vr), f"{tag} exp_avg_sq")
    wp = R.assert_within(p1, pr, R.ULP * np.abs(p0) + 16 * R.U * np.abs(upd), f"{tag} param")
    print(f"adam {tag}: worst error / bound: exp_avg {wm:.3f} exp_avg_sq {wv:.3f} param {wp:.3f}")


def _adam_call(L, t, n, step, wd, d_scale):
    L.call("pcs_adam", L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]), n, L.ptr(d_scale), 1e-3, 0.9, 0.999, 1e-8,
           wd, step, L.stream_ptr())
    torch.cuda.synchronize()


@pytest.mark.parametrize("scale", [None, 0.37])
@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("n", [1, 255, 257, 100003])
def test_adam(n, wd, scale):
    """Gradients keep their sign from step to step and stay away from 0, so exp_avg is a sum of
    same-sign terms and its relative bound is well posed (no cancellation); exp_avg_sq is a sum
    of squares anyway."""
    import pcs_amd._lib as L
    r = rng(11, n)
    wdf = float(F32(wd))
    sc = None if scale is None else float(F32(scale))
    d_scale = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=DEV)
    sign = r.choice([-1.0, 1.0], n)
    grad = lambda: (sign * (0.1 + np.abs(r.standard_normal(n)))).astype(F32)      # noqa: E731
    pad = 3                                                # the kernel must stop at n
    t = [torch.full((n + pad,), 5.0, device=DEV) for _ in range(4)]
    t[0][:n] = dev(r.standard_normal(n).astype(F32))
    t[2][:n], t[3][:n] = 0.0, 0.0
    for step in (1, 2, 3):
        t[1][:n] = dev(grad())
        before = [host(x)[:n].copy() for x in t]
        _adam_call(L, t, n, step, wd, d_scale)
        _adam_check(f"n={n} step={step}", before, [host(x)[:n] for x in t], step, wdf, sc)
    for x in t:
        assert (x[n:] == 5.0).all()
    # a fresh state at a large step number: both bias corrections are 1 to fp32
    t[0][:n] = dev(r.standard_normal(n).astype(F32))
    t[1][:n] = dev(grad())
    t[2][:n], t[3][:n] = 0.0, 0.0
    before = [host(x)[:n].copy() for x in t]
    _adam_call(L, t, n, 100000, wd, d_scale)
    _adam_check(f"n={n} step=100000", before, [host(x)[:n] for x in t], 100000, wdf, sc)
    with pytest.raises(L.PcsError):
        _adam_call(L, t, n, 0, wd, d_scale)


def test_fused_adam_on_model():
    """FusedAdam over the flat buffers of a PointNetSegmentation(3, input_dim=3): three steps
    with random gradients written into the flat gradient buffer, every parameter against
    adam_ref from the state before the step."""
    from pcs_amd.model import PointNetSegmentation
    from pcs_amd.optim import FusedAdam, flat_buffers, param_slices
    torch.manual_seed(0)
    model = PointNetSegmentation(3, input_dim=3).to(DEV)
    opt = FusedAdam(model)                                 # lr 1e-3, betas (0.9, 0.999), eps 1e-8, wd 1e-4
    pflat, gflat = flat_buffers(model)
    n = pflat.numel()
    assert n == sum(p.numel() for p in model.parameters())
    g = torch.Generator().manual_seed(12)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    wd = float(F32(1e-4))
    for step in (1, 2, 3):
        gflat[:n] = (sign * (0.1 + torch.randn(n, generator=g).abs())).to(DEV)
        before = [host(x)[:n].copy() for x in (pflat, gflat, opt.exp_avg, opt.exp_avg_sq)]
        opt.step()
        torch.cuda.synchronize()
        after = [host(x)[:n] for x in (pflat, gflat, opt.exp_avg, opt.exp_avg_sq)]
        covered = 0
        for (name, p), (_, off, k) in zip(model.named_parameters(), param_slices(model)):
            sl = slice(off, off + k)
            assert np.array_equal(host(p).reshape(-1), after[0][sl]), name   # the parameter is its slice
            _adam_check(f"{name} step={step}", [b[sl] for b in before], [a[sl] for a in after], step, wd, None)
            covered += k
        assert covered == n
