"""The forward pcs_gemm paths on their own through the C ABI (PCS_PRO_RAW / PCS_PRO_BNRELU operands,
PCS_EPI_FWD / PCS_EPI_BNRELU / PCS_EPI_RAW and the folded PCS_EPI_DGRAD), against the fp64
restatement of tests/fwd_refs.py (proved against torch in tests/test_fwd_refs.py).  Kernels by
class, with the template arguments as a kernel trace prints them (PRO 0 = RAW, 1 = BNRELU; EPI 0 =
FWD, 1 = DGRAD, 2 = RAW, 3 = BNRELU; bf16_t prints as unsigned short).  fwd_refs.kernel_of names
the instantiation of every case, and tests/test_fwd_refs.py holds those names against the list
recorded from a kernel trace of this module, profiles/fwd_gemm_kernels.txt:

  f32     gemm_nt_kernel<float, 128, BN, PRO, EPI, POOL, MASK, false>, for BN = 64 and BN = 128 each:
            EPI 0: PRO 1 with POOL and MASK each on and off, PRO 0 with POOL on and off;
            EPI 3: PRO 1 with MASK on and off, PRO 0;  EPI 2: PRO 1 with MASK on and off;
            EPI 1: PRO 1 and PRO 0 (no MASK, no sparse rows): 13 per tile
  bf16g   gemm_nt_kernel<unsigned short, 128, BN, ...>: the same 26 (PCS_FLAG_GENERIC)
  big     gemm_big_kernel<PRO, EPI, MASK, false>: <1, 0, false|true>, <0, 0, false>,
            <1, 3, false|true>, <0, 3, false>
  stream  fwd_stream_kernel<K, NCOLS, EPI, MASK, SBIAS, false, false>: <64, 512, 0, false, false|true>,
            <512, 256, 0, false|true, false>, <256, 128, 0, false|true, false>, <64, 128, 0, false, false>,
            <64, 64, 0, false, false>, <128, 1024, 3, false, false>
  seam    gemm_nt_kernel<unsigned short, 128, 128, 1, 2, false, false|true, false> and
            <unsigned short, 128, 128, 1|0, 1, false, false, false> on the 256-row-multiple chunks
            of the wide class

(wres_bnrelu_kernel needs PCS_FLAG_C_FP8 and gemm_glds_kernel is the LDS-DMA kernel: both belong to
other test modules.)  fwd_refs.FWD_CASES (B = 3 scenes throughout) takes every class through its
operand variants at one ragged N and through every N edge of its row tile and row step once; the
comments there say which *_applicable predicate keeps the other kernels away.  Every case runs twice:

  exact  small integers (fwd_refs.fwd_data): every staged operand, partial sum and stored value is
         exact in bf16 and fp32, so the stored C, the EPI_DGRAD dz / S1 / S2 and the EPI_BNRELU
         column sums must equal the fp64 reference bit for bit.  The integer outputs tie often:
         the max-pool rows must be the first occurrence across threads, tiles and chunks;
  value  Gaussian data against the derived element-wise bounds of fwd_refs (none tuned on GPU
         output).  The worst err / bound per class and output is printed when the module finishes
         (pytest -s; recorded in profiles/fwd_gemm_ratios.txt).  A bf16 C comes close to 1 by
         construction: its bound is dominated by 2^-8 |C|, the worst case of the one rounding to
         bf16, met by some element of many thousand.

Statistics and pool records are checked against the kernel's own stored C for both kinds of data:
chunk means within 1e-5 max|C|, chunk M2 within 1e-4 M2 (0 for the constant column), column sums
within sum_bound, pool records exactly; with es only the pair sign(es) selects is required.  The
`nullC` cases run a second time with C = NULL: statistics and pool must not change by a bit.

Every output is prefilled with NaN and followed by a guard region that must stay untouched; C has
exactly M rows, stats and pool exactly the [B * chunks_per_scene, Ncols, 2 | 4] entries
pcs_gemm_geometry reports, all of which must come back written."""
import ctypes as ct

import numpy as np
import pytest
import torch

import fwd_refs as R
from test_gpu_bwd_unfused import Out, dev, tdtype

pytestmark = pytest.mark.gpu
KINDS = ["exact", "value"]
RATIOS = {}
KERNEL = {"f32": "gemm_nt_kernel<float>", "bf16g": "gemm_nt_kernel<bf16_t>", "big": "gemm_big_kernel",
          "stream": "fwd_stream_kernel", "seam": "gemm_nt_kernel<bf16_t>, wide-class chunks"}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst err / bound per kernel class and output (value data):")
    for (k, name), (v, where) in sorted(RATIOS.items()):
        print(f"  {k:42s} {name:5s} {v:.3f}  {where}")


def check(case, kind, name, got, ref, bound, exact=True):
    if kind == "exact" and exact:
        assert np.array_equal(got, ref), (name, int((got != ref).sum()), np.argwhere(got != ref)[:4].tolist())
    else:
        ratio = R.assert_within(got, ref, bound, name)
        if kind == "value":
            key = (KERNEL[case.cls], name)
            RATIOS[key] = max(RATIOS.get(key, (0.0, "")), (ratio, R.case_id(case)))


def launch(case, d, L, T, with_C):
    """One pcs_gemm call into fresh NaN-prefilled outputs; returns (C, stats, pool, cps, rpc)."""
    f = R.flags_of(case)
    M, Nc = R.B * case.N, case.Ncols
    g = L.GemmArgs(num_scenes=R.B, scene_rows=case.N, K=case.K, Ncols=Nc, dtype=L.F32 if case.cls == "f32" else L.BF16,
                   prologue=case.pro, epilogue=case.epi, chunks_per_scene=case.cps, a_keep_scale=d["keep_scale"],
                   c_keep_scale=d["c_keep_scale"], flags=L.FLAG_GENERIC if case.cls == "bf16g" else 0)
    for k, t in T.items():
        setattr(g, k, L.ptr(t))
    rpc = L.load().pcs_gemm_geometry(ct.byref(g))
    cps = g.chunks_per_scene
    assert (cps, rpc) == R.geometry(case)
    assert rpc % R.tile_of(case) == 0 and (cps - 1) * rpc < case.N <= cps * rpc      # no empty chunk
    C = Out(M * Nc, tdtype(case)) if with_C else None                                  # exactly M rows
    dstats = case.epi == R.EPI_DGRAD and case.variant != "nostats"
    stats = Out(R.B * cps * Nc * 2) if f["stats"] or dstats else None
    pool = Out(R.B * cps * Nc * 4) if f["pool"] else None
    g.C, g.stats, g.pool = (o.ptr() if o else None for o in (C, stats, pool))
    L.call("pcs_gemm", ct.byref(g), L.stream_ptr())
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:           # a faulted device runs nothing more in this session
        pytest.exit(f"GPU error in {R.case_id(case)}: {e}", returncode=3)
    assert all(o is None or o.intact() for o in (C, stats, pool))
    return C, stats, pool, cps, rpc


def pool_records(pool, nrec, Nc):
    rec = pool.t[:pool.n].cpu().numpy().reshape(nrec, Nc, 4)
    return rec, rec.view(np.int32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.FWD_CASES, ids=R.case_id)
def test_fwd_gemm(case, kind):
    import pcs_amd._lib as L
    d = R.fwd_data(case, kind)
    ref = R.fwd_reference(case, d)
    dt = tdtype(case)
    Nc = case.Ncols
    T = dict(A=dev(d["A"], dt), pa=dev(d["s"]), pb=dev(d["t"]), W=dev(d["W"], dt), bias=dev(d["bias"]),
             scene_bias=dev(d["scene_bias"]), es=dev(d["es"]), et=dev(d["et"]), addend=dev(d["addend"], dt),
             Yp=dev(d["Yp"], dt), emean=dev(d["mean"]), erstd=dev(d["rstd"]),
             a_mask=dev(R.pack_bits(d["keep"])) if d["keep"] is not None else None,
             c_mask=dev(R.pack_bits(d["ckeep"])) if d["ckeep"] is not None else None)
    C, stats, pool, cps, rpc = launch(case, d, L, T, True)
    got = C.get(R.B, case.N, Nc)
    assert np.isfinite(got).all()
    if case.epi == R.EPI_DGRAD:
        assert ref["zeros"] > 0 and ref["zmin"] >= (1.0 if kind == "exact" else R.ZGAP)
        assert not got[~ref["gate"]].any(), "a gradient where Yp es + et <= 0"
        check(case, kind, "dz", got, ref["dz"], ref["e_dz"])
        st = stats.get(R.B, cps, Nc, 2)
        assert np.isfinite(st).all()
        S = st.sum(1)                                            # chunk partials summed per scene, in fp64
        check(case, kind, "S1", S[..., 0], ref["S1"], ref["e_S1"])
        if d["rstd"] is None:
            assert not st[..., 1].any(), "S2 without erstd"
        else:
            check(case, kind, "S2", S[..., 1], ref["S2"], ref["e_S2"])
        return
    # the EPI_BNRELU output gets a line of its own in the table: its bound goes through the affine step
    check(case, kind, "a" if case.epi == R.EPI_BNRELU else "C", got, ref["C"], ref["e_C"])
    if stats is not None:                                        # of the kernel's own stored C
        st = stats.get(R.B * cps, Nc, 2)
        assert np.isfinite(st).all()
        sref = R.stats_ref(got, cps, rpc, case.epi)
        colsum = case.epi == R.EPI_BNRELU
        check(case, kind, "sum" if colsum else "mean", st[..., 0], sref["mean"], sref["e_mean"], exact=colsum)
        check(case, kind, "M2", st[..., 1], sref["M2"], sref["e_M2"], exact=colsum)
    if pool is not None:
        rec, idx = pool_records(pool, R.B * cps, Nc)
        want = R.pool_ref(got, cps, rpc)
        widx = want.view(np.int32)
        # without es both pairs are compared (a NaN left from the prefill fails the comparison); with
        # es the header lets a kernel drop the pair sign(es) does not select, so only the other is read
        need_max = np.ones(Nc, bool) if d["es"] is None else d["es"] >= 0
        need_min = np.ones(Nc, bool) if d["es"] is None else d["es"] < 0
        for sel, v, i in ((need_max, 0, 1), (need_min, 2, 3)):
            assert sel.any() or d["es"] is not None
            assert np.array_equal(rec[:, sel, v], want[:, sel, v]), "pool value"
            bad = np.argwhere(idx[:, sel, i] != widx[:, sel, i])
            assert not len(bad), ("pool row is not the first occurrence", len(bad), bad[:4].tolist())
    if case.variant == "nullC":                                  # the same call without C: the same records
        _, stats2, pool2, _, _ = launch(case, d, L, T, False)
        assert torch.equal(stats2.t.view(torch.int32), stats.t.view(torch.int32)), "statistics change with C == NULL"
        assert torch.equal(pool2.t.view(torch.int32), pool.t.view(torch.int32)), "pool records change with C == NULL"


def test_every_class_has_a_null_c_case_and_a_multi_chunk_case():
    null = {c.cls for c in R.FWD_CASES if c.variant == "nullC"}
    assert null == {"f32", "bf16g", "big"}          # the streaming kernel needs C, the seam modes store only
    multi = {c.cls for c in R.FWD_CASES if R.geometry(c)[0] > 1}
    assert multi == set(KERNEL)
