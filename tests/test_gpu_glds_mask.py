"""The LDS-DMA global_feat kernels (csrc/gemm_glds.hip) where a tolerance test cannot see a
mistake:

* the input gradient's ReLU mask, which the kernel turns into bits K-tile by K-tile from the
  staged operand, must be exact: the operands are chosen so that no kept element can be zero
  (v = A H^T + 1 with |A H^T| <= 0.5), hence (out == 0) == (A <= 0) element for element, for a
  sign pattern with planted all-zero / all-positive rows and columns at every boundary of the
  kernel's row and column decomposition and with -0, +0 and the smallest subnormal planted;
  bf16 and fp8 operands;
* the DMA source offsets: one-row scenes, a partial-only tile and full-then-partial tiles, forward
  (max-pool, signed W) and input gradient, against fp64 and the register-staged kernel
  (FLAG_NO_GLDS).
"""
import ctypes as ct
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

K = 1024                    # = Ncols: four 256-column blocks, mask K-tiles kq0 = 0, 4, 8, 12 (fp8: 0, 2, 4, 6)
B, N = 2, 256 * 3 + 1       # four row tiles per scene, the last with one valid row


def _args(L, B, N, K, Nc, epi, flags, cps):
    a = L.GemmArgs(num_scenes=B, scene_rows=N, K=K, Ncols=Nc, dtype=L.BF16, prologue=L.PRO_RAW, epilogue=epi,
                   chunks_per_scene=cps, flags=flags)
    rpc = L.load().pcs_gemm_geometry(ct.byref(a))
    assert rpc > 0
    return a, rpc


def _sign_pattern(g):
    """[B*N, K] bool, True = positive: a seeded random half, then planted columns, then planted
    rows (rows win at the crossings, so an all-positive row is positive in every column)."""
    pos = torch.rand(B * N, K, generator=g) < 0.5
    # columns: at every 8-column boundary of every 256-column block the column before and the
    # column after are planted, one all-zero and one all-positive; which is which alternates with
    # the boundary's kind (8 / 32 / 64) so that both orders occur at chunk, word and K-tile edges
    for c in range(8, K + 1, 8):
        before_pos = (c % 32 == 0) and (c % 64 != 0)
        pos[:, c - 1] = before_pos
        if c < K:
            pos[:, c] = not before_pos
    pos[:, 0] = True
    # rows: the half-tile boundaries 63|64, 127|128 and 255|256 of every tile, one all-positive
    # and one all-zero row each, the order alternating with tile and scene
    for b in range(B):
        for t in range((N + 255) // 256):
            flip = (t + b) & 1
            for r, p in ((63, 1), (64, 0), (127, 0), (128, 1), (255, 1), (256, 0)):
                if t * 256 + r < N:
                    pos[b * N + t * 256 + r] = bool(p ^ flip)
    return pos


# planted bit patterns at (row, column): every tile of scene 0, the one-row tile of both scenes,
# columns in every 256-column block and in different 16-byte chunks of a K-tile
_PLANTS = [(5, 3), (70, 300), (130, 517), (200, 1023), (256 + 17, 64), (256 + 64, 255), (512 + 127, 776),
           (512 + 250, 9), (768, 100), (768, 1000), (N + 768, 511), (N + 768, 520), (N + 300, 33)]


def _plant(bits, neg0, sub, pos0):
    """Cycle -0, smallest subnormal, +0 through the planted positions (only the subnormal is kept)."""
    for i, (r, c) in enumerate(_PLANTS):
        bits[r, c] = (neg0, sub, pos0)[i % 3]


def _check_plants(keep):
    for i, (r, c) in enumerate(_PLANTS):
        assert bool(keep[r, c]) == (i % 3 == 1), (r, c)


@functools.lru_cache(maxsize=None)
def _case_bf16():
    g = torch.Generator().manual_seed(20240607)
    pos = _sign_pattern(g)
    val = (torch.rand(B * N, K, generator=g) * 4.0).clamp(min=2.0 ** -6)       # (0, 4]
    A = torch.where(pos, val, torch.zeros(())).to(torch.bfloat16)
    _plant(A.view(torch.int16), -0x8000, 0x0001, 0x0000)
    H = ((torch.rand(K, K, generator=g) * 2 - 1) * 2.0 ** -13).to(torch.bfloat16)
    c = torch.ones(K)
    A, H, c = A.to(DEV), H.to(DEV), c.to(DEV)
    Ad = A.double()
    keep = A.view(torch.int16) > 0                         # bf16 x > 0: sign clear, magnitude nonzero
    assert torch.equal(keep, Ad > 0)
    _check_plants(keep)
    v = Ad @ H.double().T + c.double()
    assert float((v - 1).abs().max()) <= 0.5               # no kept element can round to zero
    return A, H, c, keep, torch.where(keep, v, torch.zeros_like(v))


@functools.lru_cache(maxsize=None)
def _case_fp8():
    import pcs_amd._lib as L
    g = torch.Generator().manual_seed(20240608)
    pos = _sign_pattern(g)
    val = (torch.rand(B * N, K, generator=g) * 4.0).clamp(min=2.0 ** -6)
    A = torch.where(pos, val, torch.zeros(())).to(torch.float8_e4m3fn).view(torch.uint8)
    _plant(A, 0x80, 0x01, 0x00)
    Hf = (torch.rand(K, K, generator=g) * 2 - 1) * 2.0 ** -13
    Hf = ((Hf + Hf.T) / 2).to(DEV)
    Hq = torch.empty(K, K, dtype=torch.uint8, device=DEV)
    hs = torch.empty(K, dtype=torch.uint8, device=DEV)
    Hd = torch.empty(K, K, device=DEV)
    L.call("pcs_quant_fp8_rows", L.ptr(Hf), K, K, K, L.ptr(Hq), L.ptr(hs), L.ptr(Hd), L.stream_ptr())
    torch.cuda.synchronize()
    c = torch.ones(K, device=DEV)
    Ad = A.view(torch.float8_e4m3fn).to(torch.float64).to(DEV)
    A = A.to(DEV)
    keep = (A & 0x80 == 0) & (A & 0x7f != 0)               # e4m3 x > 0 (no NaN bytes here)
    assert torch.equal(keep, Ad > 0)
    _check_plants(keep)
    v = Ad @ Hd.double().T + c.double()                    # out[m, n] = sum_k A[m, k] Hq[n, k] 2^e[n]
    assert float((v - 1).abs().max()) < 1.0
    return A, Hq, hs, c, keep, torch.where(keep, v, torch.zeros_like(v))


def _check_dgrad(out, st, keep, dz):
    got0 = out == 0
    bad = got0 == keep                                     # masked where kept, or kept where masked
    nbad = int(bad.sum())
    if nbad:
        r, c = (int(x) for x in bad.nonzero()[0])
        pytest.fail(f"{nbad} mask bits wrong, first at row {r} (tile row {r % N % 256}) column {c}: "
                    f"out {float(out[r, c])}, keep {bool(keep[r, c])}")
    err = float((out.double() - dz).abs().max())
    assert err < 1e-2 * dz.abs().max().item(), err
    s1 = st[..., 0].double().sum(0)
    err = float((s1 - dz.sum(0)).abs().max())
    assert err < 1e-3 * dz.abs().sum(0).max().item(), err


@pytest.mark.parametrize("cps", [1, 2])
def test_dgrad_mask_exact_bf16(cps):
    """cps = 1: four tiles per chunk, so both bitmap parities are reused; cps = 2: two."""
    import pcs_amd._lib as L
    A, H, c, keep, dz = _case_bf16()
    a, rpc = _args(L, B, N, K, K, L.EPI_DGRAD, 0, cps)
    assert a.chunks_per_scene == cps and rpc == 1024 // cps
    st = torch.full((B * cps, K, 2), float("nan"), device=DEV)
    out = torch.full((B * N, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    a.A, a.W, a.C, a.Yp, a.bias = A.data_ptr(), H.data_ptr(), out.data_ptr(), A.data_ptr(), c.data_ptr()
    a.stats = st.data_ptr()
    L.call("pcs_gemm", ct.byref(a), L.stream_ptr())
    torch.cuda.synchronize()
    _check_dgrad(out, st, keep, dz)


@pytest.mark.parametrize("cps", [1, 2])
def test_dgrad_mask_exact_fp8(cps):
    import pcs_amd._lib as L
    A, Hq, hs, c, keep, dz = _case_fp8()
    a, rpc = _args(L, B, N, K, K, L.EPI_DGRAD, L.FLAG_AW_FP8, cps)
    assert a.chunks_per_scene == cps and rpc == 1024 // cps
    st = torch.full((B * cps, K, 2), float("nan"), device=DEV)
    out = torch.full((B * N, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    a.A, a.W, a.C, a.Yp, a.bias, a.w_scale = (A.data_ptr(), Hq.data_ptr(), out.data_ptr(), A.data_ptr(),
                                              c.data_ptr(), hs.data_ptr())
    a.stats = st.data_ptr()
    L.call("pcs_gemm", ct.byref(a), L.stream_ptr())
    torch.cuda.synchronize()
    _check_dgrad(out, st, keep, dz)


# ---- DMA source offsets: scene sizes around the tile, forward and input gradient ---------------
KO = 512
BO = 3


@functools.lru_cache(maxsize=None)
def _case_offsets(No):
    g = torch.Generator().manual_seed(900 + No)
    A = torch.relu(torch.randn(BO * No, KO, generator=g)).to(torch.bfloat16).to(DEV)
    W = (torch.randn(KO, KO, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    gamma = torch.randn(KO, generator=g).to(DEV)
    c = (torch.randn(KO, generator=g) * 0.1).to(DEV)
    return A, W, gamma, c, A.double() @ W.double().T


def _pool_extrema(L, pool, Bn, Nn, Nc, cps, gamma):
    gp = torch.empty(Bn, Nc, device=DEV)
    am = torch.empty(Bn, Nc, dtype=torch.int32, device=DEV)
    ysel = torch.empty(Bn, Nc, device=DEV)
    zero = torch.zeros(Nc, device=DEV)
    L.call("pcs_pool_finalize", L.ptr(pool), Bn, Nn, Nc, cps, L.ptr(gamma), L.ptr(zero), L.ptr(gp), L.ptr(am),
           L.ptr(ysel), L.stream_ptr())
    return ysel, am


@pytest.mark.parametrize("cps", [0, 2])
@pytest.mark.parametrize("No", [1, 255, 257, 256 * 2 + 128])
def test_offsets_forward_pool_signed_w(No, cps):
    """The max-pool of the LDS-DMA forward with sign-folded W: the extremum and a row holding it
    against fp64 (1e-5 of max |y|, as test_gpu_glds.py), rows bit for bit and values to 1e-6
    against the unsigned LDS-DMA call (as test_forward_pool_signed_w), and the extremum against
    the register-staged kernel at that kernel's tolerance (4e-3: bf16-rounded candidates)."""
    import pcs_amd._lib as L
    A, W, gamma, _, y = _case_offsets(No)
    Ws = torch.empty_like(W)
    L.call("pcs_sign_rows", L.ptr(W), L.BF16, KO, KO, L.ptr(gamma), L.ptr(Ws), L.stream_ptr())
    res = []
    for w, fl in ((Ws, L.FLAG_POOL_SIGNED_W), (W, 0), (W, L.FLAG_NO_GLDS)):
        a, _ = _args(L, BO, No, KO, KO, L.EPI_FWD, fl, cps)
        pool = torch.full((BO * a.chunks_per_scene, KO, 4), float("nan"), device=DEV)
        a.A, a.W, a.C, a.pool, a.es = A.data_ptr(), w.data_ptr(), None, pool.data_ptr(), gamma.data_ptr()
        L.call("pcs_gemm", ct.byref(a), L.stream_ptr())
        res.append(_pool_extrema(L, pool, BO, No, KO, a.chunks_per_scene, gamma))
    torch.cuda.synchronize()
    (vs, rs), (vu, ru), (vn, _) = res
    yb = y.view(BO, No, KO)
    sgn = torch.where(gamma > 0, 1.0, -1.0).double()
    ext = (yb * sgn).max(1).values * sgn
    scl = y.abs().max().item()
    assert float((vs.double() - ext).abs().max()) < 1e-5 * scl
    rows = rs.long() - (torch.arange(BO, device=DEV) * No)[:, None]
    assert ((rows >= 0) & (rows < No)).all()
    at = yb.gather(1, rows[:, None, :]).squeeze(1)
    assert float((at - ext).abs().max()) < 1e-5 * scl
    assert torch.equal(rs, ru)
    assert float(((vs - vu).abs() / vu.abs().clamp(min=1e-30)).max()) <= 1e-6
    assert float((vn.double() - ext).abs().max()) < 4e-3 * scl


@pytest.mark.parametrize("cps", [0, 2])
@pytest.mark.parametrize("No", [1, 255, 257, 256 * 2 + 128])
def test_offsets_dgrad(No, cps):
    """The LDS-DMA input gradient and the same call with FLAG_NO_GLDS against fp64 at the tolerances
    of test_folded_dgrad_sparse_mask_s1; both mask out exactly the elements where A <= 0.  S1 of
    the FLAG_NO_GLDS call sums values its kernel has rounded to bf16 (half an ulp, 2^-9 relative,
    each), which the 1e-3 of the largest column sum only covers for scenes of many rows: its
    bound adds 2^-9 of the column's sum of |dz|."""
    import pcs_amd._lib as L
    A, W, _, c, y = _case_offsets(No)
    dz = torch.where(A > 0, y + c.double(), torch.zeros_like(y))
    s1_tol = 1e-3 * dz.abs().sum(0).max().item()
    for fl in (0, L.FLAG_NO_GLDS):
        a, _ = _args(L, BO, No, KO, KO, L.EPI_DGRAD, fl, cps)
        st = torch.full((BO * a.chunks_per_scene, KO, 2), float("nan"), device=DEV)
        out = torch.full((BO * No, KO), float("nan"), dtype=torch.bfloat16, device=DEV)
        a.A, a.W, a.C, a.Yp, a.bias = A.data_ptr(), W.data_ptr(), out.data_ptr(), A.data_ptr(), c.data_ptr()
        a.stats = st.data_ptr()
        L.call("pcs_gemm", ct.byref(a), L.stream_ptr())
        torch.cuda.synchronize()
        assert bool((out[A <= 0] == 0).all()) and bool(torch.isfinite(out.float()).all()), fl
        err = float((out.double() - dz).abs().max())
        assert err < 1e-2 * dz.abs().max().item(), (fl, err)
        s1 = st[..., 0].double().sum(0)
        bound = s1_tol + (2.0 ** -9 * dz.abs().sum(0) if fl else 0.0)
        assert bool(((s1 - dz.sum(0)).abs() < bound).all()), (fl, float((s1 - dz.sum(0)).abs().max()))
