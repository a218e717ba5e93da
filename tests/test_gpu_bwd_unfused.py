"""The unfused backward GEMMs on their own through the C ABI, against the fp64 restatements of
tests/bwd_refs.py (proved against torch autograd in tests/test_bwd_refs.py):

  pcs_wgrad, dy_mode PCS_PRO_BWD / PCS_PRO_RAW     pcs_gemm, PCS_PRO_BWD with EPI_DGRAD / EPI_RAW
    f32    wgrad_kernel<float, 64|128, 64|128>       f32    gemm_nt_kernel<float, 128, 64|128>
    bf16g  wgrad_kernel<bf16_t, ...> (FLAG_GENERIC)  bf16g  gemm_nt_kernel<bf16_t, ...> (FLAG_GENERIC)
    big    wgrad_big_kernel<PRO_BWD, MASK>           big    gemm_big_kernel<PRO_BWD, DGRAD|RAW, ...>
           ((BWD, RAW) there: wgrad_kernel<bf16_t>)  seam   a wide-class call (256-row-multiple chunks)
                                                            that lands on gemm_nt_kernel<bf16_t>

The cases (bwd_refs.WGRAD_CASES / GEMM_CASES; B = 3 scenes throughout) take every tile class through
every mode pair at one ragged N, and every N edge of the row step (16 rows fp32, 64 bf16), of the
row tile (128, or 256 in the wide class), of the library's own splits and of caller-set splits /
chunks once per kernel class.  Every case runs twice:

  exact  small integers and powers of two (bwd_refs.wgrad_data / gemm_data): dy, x, every partial
         sum and the stored dz are exact in bf16 and fp32, so the fp64 reference is what any
         correct kernel produces, and dW, dz / raw and the per-scene S1 / S2 must equal it bit for
         bit.  Yp es + et is 0 in many places; the gradient there must be exactly 0;
  value  Gaussian data against the derived element-wise bounds of bwd_refs (none tuned on GPU
         output).  The worst err / bound per kernel and output is printed when the module finishes
         (pytest -s).  Two of those come close to 1 by construction: a bf16 dz / raw is one
         rounding to bf16, whose term of the bound (2^-8 |dz|) is exactly that rounding's worst
         case, met by some element of a few thousand; and where the kernel's fp32 value of a
         flagged operand element falls on the other side of the midpoint, dW is off by exactly
         the allowance (one bf16 ulp times the other operand), which is up to 0.94 of the bound
         at the few hundred rows of these cases (the bf16 dW maxima are exactly that share).

Every output is prefilled with NaN (dW with a sentinel, which the columns beyond Cin of a padded
row must keep) and followed by a guard region that must stay untouched; C has exactly M rows and
stats exactly the [B * chunks_per_scene, Ncols, 2] entries pcs_gemm_geometry reports, all of which
must come back finite."""
import ctypes as ct

import numpy as np
import pytest
import torch

import bwd_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GUARD = 512                 # elements after every output
SENTINEL = 1234.0           # the guard is compared in its own dtype (bf16 stores 1232)
KINDS = ["exact", "value"]
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst err / bound per kernel and output (value data):")
    for (k, name), (v, where) in sorted(RATIOS.items()):
        print(f"  {k:42s} {name:4s} {v:.3f}  {where}")


def note(kernel, name, ratio, where):
    RATIOS[(kernel, name)] = max(RATIOS.get((kernel, name), (0.0, "")), (ratio, where))


def tdtype(case):
    return torch.float32 if R.dtype_of(case) == "f32" else torch.bfloat16


def dev(a, dtype=torch.float32):
    """A host array (rows flattened to [M, C]) on the device in dtype; None stays None."""
    if a is None:
        return None
    a = np.asarray(a)
    if a.ndim == 3:
        a = a.reshape(-1, a.shape[-1])
    if a.dtype == np.uint8:
        return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype).to(DEV)


class Out:
    """n elements of fill and a guard region of GUARD sentinels after them."""

    def __init__(self, n, dtype=torch.float32, fill=float("nan")):
        self.n = n
        self.t = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
        self.t[n:] = SENTINEL
        self.guard = self.t[n:].clone()

    def ptr(self):
        return self.t.data_ptr()

    def get(self, *shape):
        return self.t[:self.n].double().cpu().numpy().reshape(shape)

    def intact(self):
        return bool(torch.equal(self.t[self.n:], self.guard))


def check(case_id, kind, kernel, name, got, ref, bound):
    if kind == "exact":
        assert np.array_equal(got, ref), (name, int((got != ref).sum()), np.argwhere(got != ref)[:4].tolist())
    else:
        note(kernel, name, R.assert_within(got, ref, bound, name), case_id)


# ---------------------------------------------------------------------------------------
# pcs_wgrad
# ---------------------------------------------------------------------------------------
def wgrad_kernel_of(case):
    if case.cls == "big" and case.x_mode == R.PRO_BNRELU:
        return "wgrad_big_kernel"
    return "wgrad_kernel<float>" if case.cls == "f32" else "wgrad_kernel<bf16_t>"


def wgrad_args(case, L):
    return L.WgradArgs(num_scenes=R.B, scene_rows=case.N, Cout=case.Cout, Cin=case.Cin,
                       dtype=L.F32 if case.cls == "f32" else L.BF16, splits_per_scene=case.sps,
                       dy_mode=case.dy_mode, x_mode=case.x_mode, x_keep_scale=1.0,
                       ldw=case.Cin + case.ldw_pad if case.ldw_pad else 0,
                       flags=L.FLAG_GENERIC if case.cls == "bf16g" else 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=R.wcase_id)
def test_wgrad(case, kind):
    import pcs_amd._lib as L
    d = R.wgrad_data(case, kind)
    ref = R.wgrad_reference(case, d)
    dt = tdtype(case)
    bwd, bn = case.dy_mode == R.PRO_BWD, case.x_mode == R.PRO_BNRELU
    T = dict(dZ=dev(d["dZ"], dt), Y=dev(d["Y"], dt) if bwd else None, X=dev(d["X"], dt),
             alpha=dev(d["alpha"]) if bwd else None, beta=dev(d["beta"]) if bwd else None,
             gamma=dev(d["gamma"]) if bwd else None, s=dev(d["s"]) if bn else None, t=dev(d["t"]) if bn else None,
             mask=dev(R.pack_bits(d["keep"])) if case.mask else None)
    a = wgrad_args(case, L)
    a.x_keep_scale = d["keep_scale"]
    a.dZ, a.Y, a.X, a.alpha, a.beta, a.gamma, a.s, a.t, a.x_mask = (
        L.ptr(T[k]) for k in ("dZ", "Y", "X", "alpha", "beta", "gamma", "s", "t", "mask"))
    nbytes = L.load().pcs_wgrad_workspace(ct.byref(a))
    assert nbytes == R.B * a.splits_per_scene * case.Cout * case.Cin * 4 and a.splits_per_scene >= 1
    assert not case.sps or a.splits_per_scene == case.sps
    ws = Out(nbytes // 4)
    ld = case.Cin + case.ldw_pad
    dW = Out(case.Cout * ld, fill=SENTINEL)
    a.partial, a.dW = ws.ptr(), dW.ptr()
    L.call("pcs_wgrad", ct.byref(a), L.stream_ptr())
    torch.cuda.synchronize()
    got = dW.get(case.Cout, ld)
    assert dW.intact() and ws.intact()
    assert (got[:, case.Cin:] == SENTINEL).all(), "columns beyond Cin of a padded row were written"
    check(R.wcase_id(case), kind, wgrad_kernel_of(case), "dW", got[:, :case.Cin], ref["dW"], ref["bound"])


def test_wgrad_own_geometry_splits_the_scenes():
    """splits_per_scene = 0: at least one case of every kernel class runs more than one slice per
    scene (pcs_wgrad_workspace fills the value pcs_wgrad then uses)."""
    import pcs_amd._lib as L
    most = {}
    for case in R.WGRAD_CASES:
        if case.sps == 0:
            a = wgrad_args(case, L)
            assert L.load().pcs_wgrad_workspace(ct.byref(a)) > 0
            k = wgrad_kernel_of(case)
            most[k] = max(most.get(k, 0), a.splits_per_scene)
    assert set(most) == {"wgrad_kernel<float>", "wgrad_kernel<bf16_t>", "wgrad_big_kernel"}
    assert all(v > 1 for v in most.values()), most


def test_wgrad_raw_raw_is_refused():
    import pcs_amd._lib as L
    case = R.WCase("f32", 64, 64, R.PRO_RAW, R.PRO_RAW, False, 21, 0, 0)
    dZ, X = torch.zeros(R.B * 21, 64, device=DEV), torch.zeros(R.B * 21, 64, device=DEV)
    a = wgrad_args(case, L)
    a.dZ, a.X = dZ.data_ptr(), X.data_ptr()
    nbytes = L.load().pcs_wgrad_workspace(ct.byref(a))
    ws, dW = Out(nbytes // 4), Out(64 * 64)
    a.partial, a.dW = ws.ptr(), dW.ptr()
    assert L.load().pcs_wgrad(ct.byref(a), L.stream_ptr()) == -1000      # PCS_EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(dW.t[:dW.n]).all() and dW.intact() and ws.intact()


# ---------------------------------------------------------------------------------------
# pcs_gemm, PCS_PRO_BWD
# ---------------------------------------------------------------------------------------
def gemm_kernel_of(case):
    return {"f32": "gemm_nt_kernel<float>", "bf16g": "gemm_nt_kernel<bf16_t>", "big": "gemm_big_kernel",
            "seam": "gemm_nt_kernel<bf16_t>, wide-class chunks"}[case.cls]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.GEMM_CASES, ids=R.gcase_id)
def test_gemm_pro_bwd(case, kind):
    import pcs_amd._lib as L
    d = R.gemm_data(case, kind)
    ref = R.gemm_reference(case, d)
    dt = tdtype(case)
    dgrad = case.epi == R.EPI_DGRAD
    M, Nc = R.B * case.N, case.Ncols
    T = dict(A=dev(d["dZ"], dt), A2=dev(d["Y"], dt), pa=dev(d["alpha"]), pb=dev(d["beta"]), pc=dev(d["gamma"]),
             W=dev(d["W"], dt), addend=dev(d["addend"], dt), Yp=dev(d["Yp"], dt), es=dev(d["es"]), et=dev(d["et"]),
             emean=dev(d["mean"]), erstd=dev(d["rstd"]),
             c_mask=dev(R.pack_bits(d["keep"])) if d["keep"] is not None else None)
    g = L.GemmArgs(num_scenes=R.B, scene_rows=case.N, K=case.K, Ncols=Nc, dtype=L.F32 if case.cls == "f32" else L.BF16,
                   prologue=L.PRO_BWD, epilogue=case.epi, chunks_per_scene=case.cps, c_keep_scale=d["keep_scale"],
                   flags=L.FLAG_GENERIC if case.cls == "bf16g" else 0)
    for k, t in T.items():
        setattr(g, k, L.ptr(t))
    rpc = L.load().pcs_gemm_geometry(ct.byref(g))
    cps = g.chunks_per_scene
    tile = 256 if case.cls in ("big", "seam") else 128
    assert rpc > 0 and rpc % tile == 0 and (cps - 1) * rpc < case.N <= cps * rpc      # no empty chunk
    assert not case.cps or cps == case.cps
    C = Out(M * Nc, dt)                                                                # exactly M rows
    stats = Out(R.B * cps * Nc * 2) if dgrad and case.variant != "nostats" else None
    g.C, g.stats = C.ptr(), stats.ptr() if stats else None
    L.call("pcs_gemm", ct.byref(g), L.stream_ptr())
    torch.cuda.synchronize()
    got = C.get(R.B, case.N, Nc)
    assert C.intact() and (stats is None or stats.intact())
    kern = gemm_kernel_of(case)
    if not dgrad:
        check(R.gcase_id(case), kind, kern, "raw", got, ref["raw"], ref["e_raw"])
        return
    assert ref["zeros"] > 0 and ref["zmin"] >= (1.0 if kind == "exact" else R.ZGAP)
    assert not got[~ref["gate"]].any(), "a gradient where Yp es + et <= 0"
    check(R.gcase_id(case), kind, kern, "dz", got, ref["dz"], ref["e_dz"])
    if stats is None:
        return
    st = stats.get(R.B, cps, Nc, 2)
    assert np.isfinite(st).all()
    S = st.sum(1)                                            # chunk partials summed per scene, in fp64
    check(R.gcase_id(case), kind, kern, "S1", S[..., 0], ref["S1"], ref["e_S1"])
    if d["rstd"] is None:
        assert not st[..., 1].any(), "S2 without erstd"
    else:
        check(R.gcase_id(case), kind, kern, "S2", S[..., 1], ref["S2"], ref["e_S2"])
