"""conv1 (csrc/small.hip: pcs_conv1_fwd, pcs_conv1_wgrad) through the C ABI for every
input_dim 1..8 and both storage dtypes, against fp64: forced and automatic chunk / split
counts, one-row and ragged scenes, a padded dW.

Forward operands lie on a binary grid (x in 1/64, W and b in 1/512, |y| < 2^7), so every partial
sum is exact in fp32 whatever the order of the fmaf chain: the stored fp32 y must be the fp64
y, and the stored bf16 y its round-to-nearest-even; the one-ulp slack allowed for the fmaf order
is never needed.  The statistics are those of the stored values, with the bounds
test_gpu_glds.py applies to fp32 Welford partials: 1e-5 * max|y| on the chunk means, 1e-4
relative on the chunk variance (M2).  The weight gradient is an fp32 sum over the M rows of
dy = alpha*dz + beta + gamma*y (two roundings) times x: (M + 2) * 2^-24 * sum|terms|."""
import ctypes as ct

import numpy as np
import pytest
import torch

import small_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F32 = np.float32

SHAPES = [(2, 300, 0), (2, 300, 3), (1, 1, 0), (3, 128 * 4 + 1, 2)]     # (B, N, chunks_per_scene)


def _dt(L, name):
    return (L.BF16, torch.bfloat16) if name == "bf16" else (L.F32, torch.float32)


def _geometry(L, B, N, K, cps):
    a = L.GemmArgs(num_scenes=B, scene_rows=N, K=K, Ncols=64, dtype=L.F32, chunks_per_scene=cps,
                   flags=L.FLAG_GENERIC)
    rpc = L.load().pcs_gemm_geometry(ct.byref(a))       # conv1 follows the generic 128-row geometry
    assert rpc > 0
    return a.chunks_per_scene, rpc


def _ulp(x, tdt):
    """spacing of the storage dtype at |x| (fp32: 24 significant bits, bf16: 8)"""
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -126)))
    return 2.0 ** (e - (7 if tdt == torch.bfloat16 else 23))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("K", range(1, 9))
def test_conv1_forward(K, dtype):
    import pcs_amd._lib as L
    dt, tdt = _dt(L, dtype)
    for case, (B, N, cps_in) in enumerate(SHAPES):
        r = np.random.default_rng([20, K, case])
        M = B * N
        x = (r.integers(-256, 257, (M, K)) / 64.0).astype(F32)
        W = (r.integers(-1024, 1025, (64, K)) / 512.0).astype(F32)
        b = (r.integers(-1024, 1025, 64) / 512.0).astype(F32) if case != 1 else None
        cps, rpc = _geometry(L, B, N, K, cps_in)
        if cps_in:
            assert cps == min(cps_in, (N + 127) // 128)
        d_x, d_W = torch.from_numpy(x).to(DEV), torch.from_numpy(W).to(DEV)
        d_b = torch.from_numpy(b).to(DEV) if b is not None else None
        C = torch.full((M + 1, 64), float("nan"), dtype=tdt, device=DEV)
        st = torch.full((B * cps + 1, 64, 2), float("nan"), device=DEV)
        a = L.GemmArgs(num_scenes=B, scene_rows=N, K=K, Ncols=64, dtype=dt, chunks_per_scene=cps,
                       A=L.ptr(d_x), W=L.ptr(d_W), C=L.ptr(C), bias=L.ptr(d_b), stats=L.ptr(st))
        L.call("pcs_conv1_fwd", ct.byref(a), L.stream_ptr())
        torch.cuda.synchronize()
        tag = f"K={K} {dtype} B={B} N={N} cps={cps}"
        ref = x.astype(np.float64) @ W.astype(np.float64).T + (b.astype(np.float64) if b is not None else 0.0)
        want = torch.from_numpy(ref).to(tdt).double().numpy()         # rounded to the storage dtype
        got = C[:M].double().cpu().numpy()
        worst = R.assert_within(got, want, _ulp(want, tdt), f"y {tag}")
        print(f"conv1 fwd {tag}: worst |y - rounded fp64| / ulp = {worst:.3f}")
        assert torch.isnan(C[M:].float()).all() and torch.isnan(st[B * cps:]).all()
        # statistics of the stored (rounded) values, per chunk
        sref = R.welford_partials(got.reshape(B, N, 64), cps, rpc, rounded=False)
        sgot = st[:B * cps].double().cpu().numpy()
        R.assert_within(sgot[..., 0], sref[..., 0], 1e-5 * np.abs(got).max(), f"chunk mean {tag}")
        R.assert_within(sgot[..., 1], sref[..., 1], 1e-4 * sref[..., 1], f"chunk M2 {tag}")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("K", range(1, 9))
def test_conv1_wgrad(K, dtype):
    import pcs_amd._lib as L
    dt, tdt = _dt(L, dtype)
    for case, (B, N, _) in enumerate(SHAPES):
        g = torch.Generator().manual_seed(1000 * K + case)
        M = B * N
        x = torch.randn(M, K, generator=g)
        dz = (torch.randn(M, 64, generator=g) * (torch.rand(M, 64, generator=g) < 0.6)).to(tdt)
        y = (torch.randn(M, 64, generator=g) * 2.0 + 0.5).to(tdt)
        al, be, ga = (torch.randn(64, generator=g) * sc for sc in (1.0, 0.05, 0.05))
        d = [t.to(DEV) for t in (x, dz, y, al, be, ga)]
        terms = (al.double() * dz.double()).abs() + be.double().abs() + (ga.double() * y.double()).abs()
        dy = al.double() * dz.double() + be.double() + ga.double() * y.double()
        ref = (dy.T @ x.double()).numpy()
        bound = R.sum_bound(M + 2, (terms.T @ x.double().abs()).numpy())
        for sps in (0, 1, 3):
            for ldw in (0, 8):
                ld = ldw or K
                dW = torch.full((64, ld), -777.0, device=DEV)
                ws = torch.full((B * 8 * 64 * K,), float("nan"), device=DEV)
                a = L.WgradArgs(num_scenes=B, scene_rows=N, Cout=64, Cin=K, dtype=dt, splits_per_scene=sps,
                                dy_mode=L.PRO_BWD, x_mode=L.PRO_RAW, dZ=L.ptr(d[1]), Y=L.ptr(d[2]),
                                alpha=L.ptr(d[3]), beta=L.ptr(d[4]), gamma=L.ptr(d[5]), X=L.ptr(d[0]),
                                x_keep_scale=1.0, partial=L.ptr(ws), dW=L.ptr(dW), ldw=ldw)
                L.call("pcs_conv1_wgrad", ct.byref(a), L.stream_ptr())
                torch.cuda.synchronize()
                tag = f"K={K} {dtype} B={B} N={N} splits={sps} ldw={ldw}"
                got = dW.cpu().numpy()
                R.assert_within(got[:, :K], ref, bound, f"dW {tag}")
                assert (got[:, K:] == -777.0).all(), f"padding {tag}"
