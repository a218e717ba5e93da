// The entry points that choose among kernel families: pcs_gemm, pcs_wgrad, pcs_gram and
// pcs_dgrad_wgrad_bn with their geometry / workspace queries.  Host code only (HIP for
// hipStream_t).  Each follows one sequence: validate the operands, compute the route once
// (route.h), check the flags against it, apply its geometry, switch on its kernel to the family's
// launcher.
#include "common.h"

using namespace route;

// ---------------------------------------------------------------------------------------
// pcs_gemm
// ---------------------------------------------------------------------------------------
extern "C" int64_t pcs_gemm_geometry(pcs_gemm_args *a) {
  if (!a || a->num_scenes <= 0 || a->scene_rows <= 0 || a->Ncols <= 0)
    return pcs_set_einval("pcs_gemm_geometry", "empty geometry");
  const GemmRoute r = gemm_class(*a);
  a->chunks_per_scene = r.chunks_per_scene;
  return r.rows_per_chunk;
}

extern "C" int pcs_gemm(const pcs_gemm_args *ap, pcs_stream_t stream) {
  if (!ap) return pcs_set_einval("pcs_gemm", "null args");
  pcs_gemm_args a = *ap;
  if (a.prologue != PCS_PRO_RAW && a.prologue != PCS_PRO_BNRELU && a.prologue != PCS_PRO_BWD &&
      a.prologue != PCS_PRO_CAT)
    return pcs_set_einval("pcs_gemm", "unknown prologue (PCS_PRO_RAW, PCS_PRO_BNRELU, PCS_PRO_BWD or PCS_PRO_CAT)");
  if (a.K <= 0 || a.Ncols <= 0) return pcs_set_einval("pcs_gemm", "K/Ncols must be positive");
  if (a.Ncols % 64 != 0) return pcs_set_einval("pcs_gemm", "Ncols must be a multiple of 64");
  const int kstep = a.dtype == PCS_BF16 ? 32 : 16;
  if (a.K % kstep != 0) return pcs_set_einval("pcs_gemm", "K must be a multiple of the k-step");
  if (!a.A || !a.W) return pcs_set_einval("pcs_gemm", "A and W are required");
  if (a.prologue == PCS_PRO_BWD && (!a.A2 || !a.pa || !a.pb || !a.pc))
    return pcs_set_einval("pcs_gemm", "PRO_BWD needs A2 (=Y_l), alpha, beta, gamma");
  if (a.prologue == PCS_PRO_BNRELU && (!a.pa || !a.pb))
    return pcs_set_einval("pcs_gemm", "PRO_BNRELU needs s and t");
  if (a.epilogue < PCS_EPI_FWD || a.epilogue > PCS_EPI_BNRELU) return pcs_set_einval("pcs_gemm", "bad epilogue");
  if (a.epilogue == PCS_EPI_DGRAD && (!a.Yp || !a.C || !a.es != !a.et || (a.erstd && !a.emean)))
    return pcs_set_einval("pcs_gemm", "EPI_DGRAD needs Yp and C (es/et both or neither, emean with erstd)");
  if (a.epilogue == PCS_EPI_BNRELU && (!a.es || !a.et || !a.C || a.pool))
    return pcs_set_einval("pcs_gemm", "EPI_BNRELU needs es, et and C (no pool)");

  // Pure, and safe on what is not validated yet: the checks below stay in the order they always
  // had, and those that depend on the kernel read it from the route.
  const GemmRoute r = gemm_route(a);
  const GemmKernel k = r.kernel;
  // the bf16 256-wide BN+ReLU store: EPI_BNRELU on fwd_stream (conv5), gemm_wres or gemm_big
  const bool wide_bnrelu = a.epilogue == PCS_EPI_BNRELU && (k == GEMM_FWD_STREAM || k == GEMM_WRES || k == GEMM_BIG);

  // EPI_BNRELU statistics = per-chunk column sums of the stored output: kernel in {fwd_stream, gemm_wres, gemm_big}
  if (a.epilogue == PCS_EPI_BNRELU && a.stats && !wide_bnrelu)
    return pcs_set_einval("pcs_gemm", "EPI_BNRELU column sums need the bf16 256-wide kernel (Ncols % 256 == 0)");
  if (a.pool && a.epilogue != PCS_EPI_FWD) return pcs_set_einval("pcs_gemm", "pool needs EPI_FWD");
  if (a.pool_w && (a.epilogue != PCS_EPI_DGRAD || a.prologue != PCS_PRO_RAW || !a.pool_idx || !a.pool_coef ||
                   a.pool_c <= 0 || a.pool_c > 1024 || a.pool_ldw < a.Ncols))
    return pcs_set_einval("pcs_gemm", "pool_w (sparse rows) needs EPI_DGRAD, PRO_RAW, pool_idx, pool_coef, "
                                      "0 < pool_c <= 1024, pool_ldw >= Ncols");
  if (a.scene_rows * a.num_scenes >= (int64_t)1 << 31)
    return pcs_set_einval("pcs_gemm", "M must be < 2^31 rows");
  if (a.prologue == PCS_PRO_CAT) {
    if (!a.A2 || !a.W2 || !a.pa || !a.pb || a.K1 <= 0 || a.K1 >= a.K || a.K1 % kstep || a.K - a.K1 > KMAX ||
        a.epilogue != PCS_EPI_DGRAD || a.a_mask)
      return pcs_set_einval("pcs_gemm", "PRO_CAT needs A2, W2, pa, pb, 0 < K1 < K (a k-step multiple), "
                                        "K - K1 <= 1024, EPI_DGRAD, no a_mask");
  } else if (a.K > KMAX) {
    return pcs_set_einval("pcs_gemm", "K must be <= 1024");
  }
  // PCS_FLAG_AW_FP8: kernel in {gemm_glds}
  if ((a.flags & PCS_FLAG_AW_FP8) && k != GEMM_GLDS)
    return pcs_set_einval("pcs_gemm", "fp8 operands (PCS_FLAG_AW_FP8) need the LDS-DMA kernel: bf16 C, RAW prologue, "
                                      "K % 256 == 0, Ncols % 256 == 0, w_scale, FWD (no C) or folded DGRAD");
  // PCS_FLAG_C_FP8: kernel in {fwd_stream, gemm_wres, gemm_big} on EPI_BNRELU
  if ((a.flags & PCS_FLAG_C_FP8) &&
      !((a.prologue == PCS_PRO_BNRELU || a.prologue == PCS_PRO_RAW) && !a.a_mask && wide_bnrelu))
    return pcs_set_einval("pcs_gemm", "fp8 output (PCS_FLAG_C_FP8) needs PRO_BNRELU (no dropout) or PRO_RAW + EPI_BNRELU "
                                      "on the bf16 256-wide kernel");
  // PCS_FLAG_POOL_SIGNED_W: kernel in {gemm_glds}
  if ((a.flags & PCS_FLAG_POOL_SIGNED_W) &&
      !(a.epilogue == PCS_EPI_FWD && a.pool && a.es && !a.stats && k == GEMM_GLDS))
    return pcs_set_einval("pcs_gemm", "PCS_FLAG_POOL_SIGNED_W needs EPI_FWD with pool and es, no statistics, on the "
                                      "LDS-DMA kernel");
  if (a.a_mask && a.prologue != PCS_PRO_BNRELU)
    return pcs_set_einval("pcs_gemm", "a_mask applies to the BNRELU prologue only");
  if (r.error) return pcs_set_einval("pcs_gemm_geometry", r.error);
  // gram: kernel in {fwd_stream}
  if (a.gram && !(a.K == 64 && a.Ncols == 64 && a.epilogue == PCS_EPI_FWD && !a.a_mask && !a.scene_bias &&
                  k == GEMM_FWD_STREAM))
    return pcs_set_einval("pcs_gemm", "gram (the operand's Gram) needs bf16 PRO_BNRELU + EPI_FWD, K = Ncols = 64, "
                                      "no dropout bits, on the streaming kernel");

  a.chunks_per_scene = r.chunks_per_scene;
  const int64_t rpc = r.rows_per_chunk;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int tps_big = (int)((a.scene_rows + BIG_BM - 1) / BIG_BM);
  switch (k) {
    case GEMM_FWD_STREAM: return pcs_fwd_stream_launch(a, rpc, s);
    case GEMM_WRES: return pcs_gemm_wres_launch(a, rpc, s);
    case GEMM_GLDS: return pcs_gemm_glds_launch(a, tps_big, (int)(rpc / BIG_BM), s);
    case GEMM_BIG: return pcs_gemm_big_launch(a, tps_big, (int)(rpc / BIG_BM), s);
    case GEMM_C5_DGRAD: return pcs_c5_dgrad_launch(a, rpc, s);
    case GEMM_NT: break;
  }
  if (a.dtype != PCS_BF16 && a.dtype != PCS_F32) return pcs_set_einval("pcs_gemm", "bad dtype");
  return pcs_gemm_nt_launch(a, (int)((a.scene_rows + NT_BM - 1) / NT_BM), (int)(rpc / NT_BM), s);
}

// ---------------------------------------------------------------------------------------
// pcs_wgrad, pcs_gram
// ---------------------------------------------------------------------------------------
// a caller built against ABI 2 may still fill the three fields ABI 3 removed (pcs.h)
static bool reserved_set(const pcs_wgrad_args &a) { return a.reserved0 || a.reserved1 || a.reserved2; }

extern "C" int64_t pcs_wgrad_workspace(pcs_wgrad_args *a) {
  if (!a || a->num_scenes <= 0 || a->scene_rows <= 0 || a->Cout <= 0 || a->Cin <= 0)
    return pcs_set_einval("pcs_wgrad_workspace", "bad geometry");
  if (reserved_set(*a)) return pcs_set_einval("pcs_wgrad_workspace", "reserved0..2 must be NULL (removed in ABI 3)");
  a->splits_per_scene = wgrad_class_splits(*a);
  const int64_t nslabs = (int64_t)a->num_scenes * a->splits_per_scene;
  return nslabs * a->Cout * a->Cin * 4;
}

extern "C" int pcs_wgrad(const pcs_wgrad_args *ap, pcs_stream_t stream) {
  if (!ap) return pcs_set_einval("pcs_wgrad", "null args");
  pcs_wgrad_args a = *ap;
  if (reserved_set(a)) return pcs_set_einval("pcs_wgrad", "reserved0..2 must be NULL (removed in ABI 3)");
  if (a.dy_mode != PCS_PRO_RAW && a.dy_mode != PCS_PRO_BNRELU && a.dy_mode != PCS_PRO_BWD)
    return pcs_set_einval("pcs_wgrad", "unknown dy_mode (PCS_PRO_RAW, PCS_PRO_BNRELU or PCS_PRO_BWD)");
  if (a.Cout % 64 || a.Cin % 64) return pcs_set_einval("pcs_wgrad", "Cout/Cin must be multiples of 64");
  if (!a.X || !a.partial || !a.dW) return pcs_set_einval("pcs_wgrad", "missing operand");
  if (a.dy_mode == PCS_PRO_RAW ? !a.dZ : (!a.Y || !a.beta || !a.gamma))
    return pcs_set_einval("pcs_wgrad", "dy operands missing (RAW: dZ; otherwise: Y, beta, gamma)");
  if (a.dy_mode == PCS_PRO_BWD && (!a.dZ || !a.alpha)) return pcs_set_einval("pcs_wgrad", "PRO_BWD needs dZ, alpha");
  if (a.x_mode == PCS_PRO_BNRELU && (!a.s || !a.t)) return pcs_set_einval("pcs_wgrad", "x BNRELU needs s, t");
  if (pcs_wgrad_workspace(&a) < 0) return PCS_EINVAL;   // checks the geometry, fills the class's splits
  const WgradRoute r = wgrad_route(a);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int rc = 0;
  switch (r.kernel) {
    case WGRAD_C5: rc = pcs_wgrad_c5_launch(a, r.rows_per_split, s); break;
    case WGRAD_BIG: rc = pcs_wgrad_big_launch(a, s); break;
    case WGRAD_TN:
      if (a.dtype != PCS_BF16 && a.dtype != PCS_F32) return pcs_set_einval("pcs_wgrad", "bad dtype");
      rc = pcs_wgrad_tn_launch(a, r.rows_per_split, s);
      break;
  }
  if (rc) return rc;
  const int64_t nslabs = a.num_scenes * a.splits_per_scene;
  return pcs_reduce_partials(a.partial, nslabs, (int64_t)a.Cout * a.Cin, 1.0f, a.dW,
                             a.ldw ? a.ldw : a.Cin, a.Cin, stream);
}

// Gram of the BN+ReLU activations (global_feat weight gradient, see gram.hip)
extern "C" int64_t pcs_gram_workspace(int64_t num_scenes, int64_t scene_rows, int32_t C, int32_t dtype,
                                      int32_t *splits_per_scene) {
  if (num_scenes <= 0 || scene_rows <= 0 || C <= 0 || C % 64 || !splits_per_scene)
    return pcs_set_einval("pcs_gram_workspace", "bad geometry");
  const pcs_wgrad_args a = gram_args(nullptr, nullptr, nullptr, num_scenes, scene_rows, C, dtype, 0);
  *splits_per_scene = gram_route(a).splits_per_scene;
  return num_scenes * *splits_per_scene * ((int64_t)C * C + C) * 4;
}

extern "C" int pcs_gram(const void *Y, const float *s, const float *t, int64_t num_scenes, int64_t scene_rows,
                        int32_t C, int32_t dtype, int32_t splits_per_scene, float *workspace, float *G,
                        float *colsum, pcs_stream_t stream) {
  if (!Y || !s != !t || !workspace || !G || !colsum || splits_per_scene <= 0)
    return pcs_set_einval("pcs_gram", "missing operand or splits (s and t both set, or both NULL)");
  if (C % 64) return pcs_set_einval("pcs_gram", "C must be a multiple of 64");
  pcs_wgrad_args a = gram_args(Y, s, t, num_scenes, scene_rows, C, dtype, splits_per_scene);
  a.partial = workspace;
  const GramRoute r = gram_route(a);
  if (!s && r.kernel != GRAM_BIG)   // s = t = NULL: Y is already the activation
    return pcs_set_einval("pcs_gram", "s = t = NULL needs the 256x256 kernel (bf16, C % 256 == 0)");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int rc = 0;
  switch (r.kernel) {
    case GRAM_128: rc = pcs_gram128_launch(a, st); break;
    case GRAM_BIG: rc = pcs_wgrad_big_launch(a, st); break;
    case GRAM_TN:
      if (dtype != PCS_BF16 && dtype != PCS_F32) return pcs_set_einval("pcs_gram", "bad dtype");
      rc = pcs_wgrad_tn_launch(a, r.rows_per_split, st);
      break;
  }
  if (rc) return rc;
  const int nsplit = (int)(num_scenes * splits_per_scene);
  const int64_t n = (int64_t)C * C;
  if ((rc = pcs_reduce_partials(workspace, nsplit, n, 1.f, G, C, C, stream))) return rc;
  if ((rc = pcs_reduce_partials(workspace + nsplit * n, nsplit, C, 1.f, colsum, C, C, stream))) return rc;
  return pcs_gram_mirror_launch(G, C, st);
}

// ---------------------------------------------------------------------------------------
// pcs_dgrad_wgrad_bn
// ---------------------------------------------------------------------------------------
static int bn_checked_route(const pcs_gemm_args *a, BnRoute *r) {
  if (!a || a->num_scenes <= 0 || a->scene_rows <= 0) return pcs_set_einval("pcs_dgrad_wgrad_bn_workspace", "bad geometry");
  *r = bn_route(*a);
  return r->error ? pcs_set_einval("pcs_dgrad_wgrad_bn_workspace", r->error) : 0;
}

extern "C" int64_t pcs_dgrad_wgrad_bn_workspace(pcs_gemm_args *a) {
  BnRoute r;
  if (bn_checked_route(a, &r)) return PCS_EINVAL;
  a->chunks_per_scene = r.chunks_per_scene;
  return (int64_t)a->num_scenes * a->chunks_per_scene * a->K * a->Ncols * 4;
}

extern "C" int pcs_dgrad_wgrad_bn(const pcs_gemm_args *ap, float *partial, float *dW, int64_t ldw,
                                  pcs_stream_t stream) {
  if (!ap || !partial || !dW) return pcs_set_einval("pcs_dgrad_wgrad_bn", "null argument");
  pcs_gemm_args a = *ap;
  BnRoute r;
  if (bn_checked_route(&a, &r)) return PCS_EINVAL;
  if (r.chunks_per_scene != a.chunks_per_scene)
    return pcs_set_einval("pcs_dgrad_wgrad_bn", "chunks_per_scene must come from pcs_dgrad_wgrad_bn_workspace");
  if (!a.A || !a.A2 || !a.pa || !a.pb || !a.pc || !a.W || !a.C || !a.Yp || !a.es || !a.et || !a.emean ||
      !a.erstd || !a.stats)
    return pcs_set_einval("pcs_dgrad_wgrad_bn", "missing operand (A, A2, pa, pb, pc, W, C, Yp, es, et, emean, "
                                                "erstd, stats)");
  if (a.scene_rows * a.num_scenes >= (int64_t)1 << 31) return pcs_set_einval("pcs_dgrad_wgrad_bn", "M must be < 2^31");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = r.kernel == BN_SEG4 ? pcs_seg4_launch(a, partial, r.rows_per_chunk, s)
                                     : pcs_dgrad_wgrad_bn_launch(a, partial, r.rows_per_chunk, s);
  if (rc) return rc;
  const int nslab = (int)(a.num_scenes * a.chunks_per_scene);
  return pcs_reduce_partials(partial, nslab, (int64_t)a.K * a.Ncols, 1.0f, dW, ldw ? ldw : a.Ncols, a.Ncols, stream);
}
