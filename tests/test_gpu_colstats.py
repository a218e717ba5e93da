"""The streaming passes of csrc/colstats.hip through the C ABI against fp64: pcs_colstats
(per-chunk BN partials and max-pool records of a stored activation) and pcs_bnrelu_bwd (the
EPI_DGRAD epilogue as an in-place pass).

Pool records are selections: value and first row bit-exact against torch.max / torch.min over
the chunk, ties, a -inf column and a NaN included.  Welford partials take the bounds
test_gpu_glds.py applies to fp32 partials of this format (1e-5 * max|y| on chunk means, 1e-4
relative on chunk M2).  The S1 / S2 sums of pcs_bnrelu_bwd are fp32 sums: (rows + roundings of
a term) * 2^-24 * sum|terms|.  Its ReLU gate is made exact by construction: no element has
|Yp*s + t| < 2^-18 * (|Yp*s| + |t|), so the fp32 sign agrees with fp64 and nothing is excluded
from any comparison."""
import ctypes as ct

import numpy as np
import pytest
import torch

import small_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F32 = np.float32

CD = [(1024, "bf16"), (64, "bf16"), (8, "bf16"), (1024, "fp32"), (4, "fp32")]
BN = [(2, 1000), (1, 5)]     # (1, 5): fewer rows than threads per column, the empty-thread merge


def _dt(L, name):
    return (L.BF16, torch.bfloat16) if name == "bf16" else (L.F32, torch.float32)


def _geometry(L, B, N, C):
    cps = ct.c_int32(0)
    rpc = L.load().pcs_colstats_geometry(B, N, C, ct.byref(cps))
    assert rpc > 0 and (cps.value - 1) * rpc < N <= cps.value * rpc
    return cps.value, rpc


def _eq_nan(got, ref, what):
    """bitwise equal values; a NaN matches a NaN"""
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), what
    ok = ~torch.isnan(ref)
    assert torch.equal(got[ok].view(torch.int32), ref[ok].view(torch.int32)), what


@pytest.mark.parametrize("mode", ["stats", "pool", "both"])
@pytest.mark.parametrize("B,N", BN)
@pytest.mark.parametrize("C,dtype", CD)
def test_colstats(C, dtype, B, N, mode):
    import pcs_amd._lib as L
    dt, tdt = _dt(L, dtype)
    g = torch.Generator().manual_seed(C + N)
    Y = (torch.randn(B, N, C, generator=g) * 2.0 + 0.7).to(tdt)
    Y[:, :, 0] = 2.5                           # constant: every row ties
    Y[:, :, 1] = float("-inf")
    Y[0, 3, 2] = float("nan")
    cps, rpc = _geometry(L, B, N, C)
    nch = B * cps
    st = torch.full((nch + 1, C, 2), 123.0, device=DEV)
    pool = torch.full((nch + 1, C, 4), 123.0, device=DEV)
    d_Y = Y.to(DEV)
    L.call("pcs_colstats", L.ptr(d_Y), B, N, C, dt, cps, rpc, L.ptr(st) if mode != "pool" else None,
           L.ptr(pool) if mode != "stats" else None, L.stream_ptr())
    torch.cuda.synchronize()
    assert (st[nch:] == 123.0).all() and (pool[nch:] == 123.0).all()
    Yf = Y.float()                             # the stored values, widened exactly
    st, pool = st[:nch].cpu().view(B, cps, C, 2), pool[:nch].cpu().view(B, cps, C, 4)
    if mode == "stats":
        assert (pool == 123.0).all()
    if mode == "pool":
        assert (st == 123.0).all()
    finite = torch.ones(C, dtype=torch.bool)
    finite[1] = False
    scl = float(Yf[:, :, finite][~torch.isnan(Yf[:, :, finite])].abs().max())
    for j, (lo, hi) in enumerate(R.chunk_bounds(N, cps, rpc)):
        blk = Yf[:, lo:hi]
        base = (torch.arange(B) * N + lo)[:, None]
        if mode != "stats":
            mx, mn = blk.max(1), blk.min(1)
            tag = f"chunk {j}"
            _eq_nan(pool[:, j, :, 0], mx.values, f"max {tag}")
            _eq_nan(pool[:, j, :, 2], mn.values, f"min {tag}")
            rows = pool[:, j].contiguous().view(torch.int32)
            assert torch.equal(rows[..., 1].long(), mx.indices + base), f"argmax {tag}"
            assert torch.equal(rows[..., 3].long(), mn.indices + base), f"argmin {tag}"
            assert (rows[:, 0, 1] == base[:, 0]).all() and (rows[:, 1, 3] == base[:, 0]).all()   # ties, -inf: first row
        if mode != "pool":
            bd = blk.double()
            nanc = torch.isnan(bd).any(1)                         # [B, C]: a NaN in this chunk's column
            nanc[:, 1] = True                                     # -inf: the variance is undefined
            mean = bd.mean(1)
            m2 = ((bd - mean[:, None]) ** 2).sum(1)
            good = (~nanc).numpy()
            R.assert_within(st[:, j, :, 0].numpy()[good], mean.numpy()[good], 1e-5 * scl, f"chunk {j} mean")
            R.assert_within(st[:, j, :, 1].numpy()[good], m2.numpy()[good], 1e-4 * m2.numpy()[good], f"chunk {j} M2")
            assert torch.isnan(st[:, j, :, 1][nanc]).all(), f"chunk {j}: M2 of a non-finite column"


def test_colstats_rejects_bad_width():
    import pcs_amd._lib as L
    Y = torch.zeros(2 * 16, 24, dtype=torch.bfloat16, device=DEV)
    st = torch.full((2, 24, 2), 123.0, device=DEV)
    with pytest.raises(L.PcsError):        # 24 / 8 = 3 chunks per row does not divide 256
        L.call("pcs_colstats", L.ptr(Y), 2, 16, 24, L.BF16, 1, 16, L.ptr(st), None, L.stream_ptr())
    with pytest.raises(L.PcsError):
        L.call("pcs_bnrelu_bwd", L.ptr(Y), L.ptr(Y), None, None, 1.0, L.ptr(st), L.ptr(st), L.ptr(st), L.ptr(st),
               2, 16, 24, L.BF16, 1, 16, L.ptr(st), L.stream_ptr())
    torch.cuda.synchronize()
    assert (st == 123.0).all()


def _gated_inputs(g, B, N, C, tdt):
    """Yp (storage dtype), s, t with every |Yp*s + t| >= 2^-18 * (|Yp*s| + |t|): offenders are
    resampled on the CPU until none remain."""
    s = torch.randn(C, generator=g)
    s = torch.where(s.abs() < 0.05, torch.full_like(s, 0.5), s)
    t = torch.randn(C, generator=g) * 0.5
    Yp = torch.randn(B, N, C, generator=g).to(tdt)
    for _ in range(20):
        z1 = Yp.double() * s.double()
        bad = (z1 + t.double()).abs() < 2.0 ** -18 * (z1.abs() + t.double().abs())
        if not bad.any():
            break
        Yp[bad] = torch.randn(int(bad.sum()), generator=g).to(tdt)
    z1 = Yp.double() * s.double()
    assert not ((z1 + t.double()).abs() < 2.0 ** -18 * (z1.abs() + t.double().abs())).any()
    return Yp, s, t


# keep bits are bytes of 8 channels: no mask for C = 4
CDM = [(c, d, m) for c, d in CD for m in (False, True) if not (m and c % 8)]


@pytest.mark.parametrize("use_addend", [False, True])
@pytest.mark.parametrize("B,N", BN)
@pytest.mark.parametrize("C,dtype,use_mask", CDM)
def test_bnrelu_bwd(C, dtype, use_mask, B, N, use_addend):
    import pcs_amd._lib as L
    dt, tdt = _dt(L, dtype)
    g = torch.Generator().manual_seed(7 * C + N)
    M = B * N
    Yp, s, t = _gated_inputs(g, B, N, C, tdt)
    D = torch.randn(B, N, C, generator=g).to(tdt)
    ad = torch.randn(B, N, C, generator=g).to(tdt)
    mean, rstd = torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5
    ks = float(F32(1.0 / 0.7))
    cps, rpc = _geometry(L, B, N, C)
    nch = B * cps
    d_D, d_Yp, d_ad = D.to(DEV), Yp.to(DEV), ad.to(DEV)
    d_s, d_t, d_m, d_r = (x.to(DEV) for x in (s, t, mean, rstd))
    st = torch.full((nch + 1, C, 2), 123.0, device=DEV)
    keep = torch.ones(B, N, C, dtype=torch.float64)
    bits = None
    if use_mask:
        bits = torch.empty(M, C // 8, dtype=torch.uint8, device=DEV)
        L.call("pcs_dropout_bits", 99, 0, M, C, 0.3, L.ptr(bits), L.stream_ptr())
        torch.cuda.synchronize()
        kb = np.unpackbits(bits.cpu().numpy(), axis=1, bitorder="little")
        assert 0.5 < kb.mean() < 0.9 or M * C < 200
        keep = torch.from_numpy(kb.astype(np.float64)).view(B, N, C) * ks
    L.call("pcs_bnrelu_bwd", L.ptr(d_D), L.ptr(d_Yp), L.ptr(d_ad) if use_addend else None, L.ptr(bits), ks,
           L.ptr(d_s), L.ptr(d_t), L.ptr(d_m), L.ptr(d_r), B, N, C, dt, cps, rpc, L.ptr(st), L.stream_ptr())
    torch.cuda.synchronize()
    assert (st[nch:] == 123.0).all()
    gate = (Yp.double() * s.double() + t.double()) > 0
    assert gate.any() and not gate.all()
    v = D.double() + (ad.double() if use_addend else 0.0)          # one fp32 rounding
    dz = torch.where(gate, v * keep, torch.zeros_like(v))          # a second one (keep_scale)
    got = d_D.cpu().double()
    assert (got[~gate] == 0).all()
    # rounding to the storage dtype: bf16 keeps 8 significant bits, half an ulp is 2^-8 relative
    store = 2.0 ** -8 if tdt == torch.bfloat16 else 0.0
    R.assert_within(got.numpy(), dz.numpy(), (2 * R.U + store * (1 + 2 * R.U)) * dz.abs().numpy(), "dz")
    xhat = (Yp.double() - mean.double()) * rstd.double()           # two fp32 roundings
    st = st[:nch].cpu().double().view(B, cps, C, 2)
    for j, (lo, hi) in enumerate(R.chunk_bounds(N, cps, rpc)):
        a, x = dz[:, lo:hi], xhat[:, lo:hi]
        n = hi - lo
        R.assert_within(st[:, j, :, 0].numpy(), a.sum(1).numpy(), R.sum_bound(n + 2, a.abs().sum(1).numpy()), f"S1 chunk {j}")
        R.assert_within(st[:, j, :, 1].numpy(), (a * x).sum(1).numpy(),
                        R.sum_bound(n + 4, (a * x).abs().sum(1).numpy()), f"S2 chunk {j}")
