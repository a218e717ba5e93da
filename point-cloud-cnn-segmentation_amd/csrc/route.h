// Which kernel family a call reaches and over which chunk / split geometry: the host-side
// routing of pcs_gemm, pcs_wgrad, pcs_gram, pcs_dgrad_wgrad_bn (dispatch.hip) and pcs_head's
// class.  Plain C++17 (no HIP): every function here is a pure function of the argument struct,
// so tests/test_routes.py walks it with the system compiler.  A kernel file that owns one of the
// constants below static_asserts its own value against it.
#pragma once
#include <cstdint>

#include "../../include/pcs.h"

// ---------------------------------------------------------------------------------------
// One split formula: about `target` workgroups over scenes x column blocks, never fewer than
// min_steps steps of `step` rows per split, at least one split; rows per split rounded up to
// the row step; `count` = the splits that are not empty.  fixed > 0 is a caller's split count in
// place of the target (clamped the same way).
// ---------------------------------------------------------------------------------------
namespace route {

struct Split { int64_t splits, rows, count; };

inline int64_t rows_per_split(int64_t rows, int64_t splits, int64_t step) {
  return ((rows + splits - 1) / splits + step - 1) / step * step;
}

inline Split split_rows(int64_t target, int64_t scenes, int64_t ncb, int64_t rows, int64_t step, int64_t min_steps,
                        int64_t fixed = 0) {
  int64_t sps = fixed > 0 ? fixed : (target + scenes * ncb - 1) / (scenes * ncb);
  const int64_t max_sps = (rows + min_steps * step - 1) / (min_steps * step);
  if (sps > max_sps) sps = max_sps;
  if (sps < 1) sps = 1;
  const int64_t rps = rows_per_split(rows, sps, step);
  return {sps, rps, (rows + rps - 1) / rps};
}

}  // namespace route

// Scene-aligned chunk geometry: fills a->chunks_per_scene (auto when <= 0, aiming at
// ~target workgroups over ncb column blocks) and returns rows per chunk.
inline int64_t pcs_fill_geometry(pcs_gemm_args *a, int64_t tile, int64_t target, int64_t ncb) {
  const route::Split sp = route::split_rows(target, a->num_scenes, ncb, a->scene_rows, tile, 1, a->chunks_per_scene);
  a->chunks_per_scene = (int32_t)sp.count;   // no empty chunks
  return sp.rows;
}

namespace route {

// ---------------------------------------------------------------------------------------
// pcs_gemm
// ---------------------------------------------------------------------------------------
constexpr int KMAX = 1024;                        // prologue coefficient arrays staged in LDS (gemm_nt, gemm_big)
constexpr int NT_BM = 128;                        // gemm_nt: row tile (column block 128 or 64)
constexpr int BIG_BM = 256, BIG_BN = 256, BIG_BK = 64;   // gemm_big and gemm_glds: tile, k-step
constexpr int WRES_K = 128, WRES_BN = 256;        // gemm_wres: conv5's input width, column block
constexpr int C5_K1 = 1024, C5_K2 = 128, C5_NC = 128;    // fused_c5: conv5's folded input gradient
#ifndef FS_SMALL_TARGET
#define FS_SMALL_TARGET 1024
#endif
// fwd_stream: bf16, PRO_BNRELU; EPI_FWD on (K, Ncols) = (64, 512) seg_conv1, (512, 256) seg_conv2,
// (256, 128) seg_conv3, (64, 128) conv4, (64, 64) conv2 / conv3; EPI_BNRELU with a bf16 store on
// (128, 1024) conv5.  nb: output columns per workgroup; target: workgroups in the grid (256 = one
// per CU; the small 64-wide layers, whose workgroups fit several to a CU, take more)
struct FsShape { int K, Ncols, epilogue, nb, target; };
inline constexpr FsShape kFsShapes[] = {
    {64, 512, PCS_EPI_FWD, 512, 256},          {512, 256, PCS_EPI_FWD, 256, 256},
    {256, 128, PCS_EPI_FWD, 128, 256},         {64, 128, PCS_EPI_FWD, 128, FS_SMALL_TARGET},
    {64, 64, PCS_EPI_FWD, 64, FS_SMALL_TARGET}, {128, 1024, PCS_EPI_BNRELU, 512, 256}};
constexpr const FsShape *fs_shape(int K, int Ncols, int epilogue) {
  for (const FsShape &f : kFsShapes)
    if (f.K == K && f.Ncols == Ncols && f.epilogue == epilogue) return &f;
  return nullptr;
}

enum GemmKernel { GEMM_FWD_STREAM, GEMM_WRES, GEMM_GLDS, GEMM_BIG, GEMM_C5_DGRAD, GEMM_NT };
enum GemmClass { CLASS_STREAM, CLASS_WIDE, CLASS_C5, CLASS_NT };

// The class gives the chunk geometry (row tile, workgroup target, column blocks); the kernel is
// the family that runs.  Kernel GEMM_NT with a class whose tile is 256 is the seam: a call of
// the wide or streaming class whose operands no 256-row kernel takes runs on the generic kernel,
// which walks the same 256-row-multiple chunks in 128-row tiles.
struct GemmRoute {
  GemmClass cls;
  bool wide;                 // wide_class(): also true for a streaming-class shape the 256x256 kernels take
  GemmKernel kernel;
  int tile, target, ncb;     // geometry of the class: pcs_fill_geometry(a, tile, target, ncb)
  int32_t chunks_per_scene;  // as filled (the caller's, clamped, or auto)
  int64_t rows_per_chunk;    // 0 with error set
  const char *error;         // "empty geometry" or nullptr
};

// streaming forward: the class's table entry (nullptr = not this class; shapes only)
inline const FsShape *fwd_stream_shape(const pcs_gemm_args &a) {
  if (a.dtype != PCS_BF16 || (a.flags & (PCS_FLAG_GENERIC | PCS_FLAG_AW_FP8)) || a.prologue != PCS_PRO_BNRELU)
    return nullptr;
  return fs_shape(a.K, a.Ncols, a.epilogue);
}

// The row-chunk geometry depends only on shapes, dtype and flags, never on which optional
// operands are set: callers size their partial buffers from pcs_gemm_geometry() before the
// pointers exist.  Shapes the 256x256 kernels can take use 256-row-multiple chunks.
inline bool wide_class(const pcs_gemm_args &a) {
  if (a.prologue == PCS_PRO_CAT) return false;   // generic kernel only
  // seg_conv3's input gradient (K 128 -> 256 columns, DGRAD epilogue): the 128-row kernel
  // measured faster at cfg2 (3.13 vs 3.38 ms, tools/bench_bwd_shapes.py)
  if (a.K == 128 && a.Ncols == 256 && a.epilogue == PCS_EPI_DGRAD) return false;
  return a.dtype == PCS_BF16 && !(a.flags & PCS_FLAG_GENERIC) && a.K % 64 == 0 && a.Ncols % 256 == 0 &&
         a.K >= 128 && a.K <= 1024;
}

// conv5's folded input gradient: bf16, PCS_PRO_CAT with K1 = 1024, K - K1 = 128, 128 output
// columns, EPI_DGRAD without dropout bits, addend or sparse pool rows.
inline bool c5_dgrad_class(const pcs_gemm_args &a) {
  return a.dtype == PCS_BF16 && !(a.flags & PCS_FLAG_GENERIC) && a.prologue == PCS_PRO_CAT &&
         a.epilogue == PCS_EPI_DGRAD && a.K1 == C5_K1 && a.K == C5_K1 + C5_K2 && a.Ncols == C5_NC;
}

// Shapes, dtype, prologue / epilogue and flags only (what pcs_gemm_geometry needs); the kernel is
// left at GEMM_NT.  Needs Ncols > 0; num_scenes or scene_rows <= 0 sets error.
inline GemmRoute gemm_class(const pcs_gemm_args &a) {
  GemmRoute r = {CLASS_NT, wide_class(a), GEMM_NT, NT_BM, 2048, a.Ncols >= 128 ? a.Ncols / 128 : 1,   // ~8 WGs per CU
                 a.chunks_per_scene, 0, nullptr};
  if (const FsShape *f = fwd_stream_shape(a)) {   // streaming forward
    r.cls = CLASS_STREAM; r.tile = 256; r.target = f->target; r.ncb = a.Ncols / f->nb;
  } else if (r.wide) {                            // one 512-thread WG per CU
    r.cls = CLASS_WIDE; r.tile = BIG_BM; r.target = 256; r.ncb = a.Ncols / 256;
  } else if (c5_dgrad_class(a)) {                 // one 512-thread WG per CU
    r.cls = CLASS_C5; r.tile = NT_BM; r.target = 256; r.ncb = 1;
  }
  if (a.num_scenes <= 0 || a.scene_rows <= 0) {
    r.error = "empty geometry";
    return r;
  }
  pcs_gemm_args g = a;
  r.rows_per_chunk = pcs_fill_geometry(&g, r.tile, r.target, r.ncb);
  r.chunks_per_scene = g.chunks_per_scene;
  return r;
}

// The operand-dependent predicates of each family, in the order pcs_gemm applies them.  `a`
// carries the chunks_per_scene of its class's geometry.
inline bool fwd_stream_takes(const pcs_gemm_args &a) {
  if (!a.C || !a.pa || !a.pb || a.pool) return false;
  if ((a.flags & PCS_FLAG_C_FP8) && a.epilogue != PCS_EPI_BNRELU) return false;
  if (a.scene_rows * a.num_scenes >= ((int64_t)1 << 31)) return false;
  // 32-bit store ranges / row offsets: a chunk of the widest rows must stay below 2 GB
  const int64_t rpc = a.chunks_per_scene > 0 ? (a.scene_rows + a.chunks_per_scene - 1) / a.chunks_per_scene
                                             : a.scene_rows;
  if (rpc * (int64_t)(a.K > a.Ncols ? a.K : a.Ncols) * 2 >= ((int64_t)1 << 31)) return false;
  if (a.epilogue == PCS_EPI_BNRELU) return a.es && a.et && !a.a_mask && !a.scene_bias;
  // dropout bits only where the layer has them (seg_conv2 / seg_conv3 inputs)
  if (a.a_mask && !((a.K == 512 && a.Ncols == 256) || (a.K == 256 && a.Ncols == 128))) return false;
  if (a.scene_bias && !(a.K == 64 && a.Ncols == 512)) return false;
  return true;
}

// gemm_wres: W-resident LDS-DMA stream for conv5's BN+ReLU pass with an fp8 store (K = 128).
// Measured at cfg2 (tools/bench_conv5.py): fp8 store 4.0 ms here vs 4.9 ms on the
// register-staged kernel; bf16 store 5.4 vs 5.0 ms, so bf16 stays there (the pass is bound by
// the epilogue's vector work and the store issue, not by the MFMAs or the loads).
inline bool gemm_wres_takes(const pcs_gemm_args &a) {
  if (a.dtype != PCS_BF16 || (a.flags & (PCS_FLAG_GENERIC | PCS_FLAG_NO_GLDS | PCS_FLAG_AW_FP8))) return false;
  if (!(a.flags & PCS_FLAG_C_FP8)) return false;
  return a.prologue == PCS_PRO_BNRELU && a.epilogue == PCS_EPI_BNRELU && a.K == WRES_K && a.Ncols % WRES_BN == 0 &&
         !a.a_mask && a.C && a.es && a.et && !a.pool && !a.scene_bias && a.scene_rows * a.num_scenes < ((int64_t)1 << 31);
}

// gemm_glds: LDS-DMA 256x256 kernel for the RAW-operand global_feat GEMMs
inline bool gemm_glds_takes(const pcs_gemm_args &a) {
  if (a.dtype != PCS_BF16 || (a.flags & (PCS_FLAG_GENERIC | PCS_FLAG_NO_GLDS))) return false;
  const bool fp8 = a.flags & PCS_FLAG_AW_FP8;
  if (fp8 && !a.w_scale) return false;
  if (a.prologue != PCS_PRO_RAW || a.K % (fp8 ? 256 : 2 * BIG_BK) != 0 || a.Ncols % BIG_BN != 0) return false;
  // forward: statistics / max-pool only (nothing stored); the pool keeps one extremum per
  // column, chosen by sign(es), so a pool needs es
  if (a.epilogue == PCS_EPI_FWD)
    return a.C == nullptr && a.scene_bias == nullptr && (!a.pool || a.es) &&
           (!(a.flags & PCS_FLAG_POOL_SIGNED_W) || (a.pool && !a.stats));
  if (a.epilogue == PCS_EPI_DGRAD)   // mask read from the operand itself, no S2, no addend
    return a.Yp == a.A && a.K == a.Ncols && !a.es && !a.et && !a.erstd && !a.addend && !a.c_mask &&
           !a.pool_w;
  return false;
}

// gemm_big: wide-layer bf16 kernel
inline bool gemm_big_takes(const pcs_gemm_args &a) {
  if (a.dtype != PCS_BF16 || a.K % BIG_BK != 0 || a.Ncols % BIG_BN != 0 || a.K < 128 || a.K > KMAX) return false;
  if (a.flags & PCS_FLAG_GENERIC) return false;
  if (a.a_mask && a.prologue != PCS_PRO_BNRELU) return false;
  if (a.epilogue == PCS_EPI_FWD || a.epilogue == PCS_EPI_BNRELU)
    return a.prologue == PCS_PRO_BNRELU || a.prologue == PCS_PRO_RAW;
  if (a.epilogue == PCS_EPI_DGRAD && (!a.es || !a.erstd || a.bias || a.pool_w)) return false;
  if (a.epilogue == PCS_EPI_DGRAD) return a.prologue == PCS_PRO_BWD && !(a.c_mask && a.addend);
  if (a.epilogue == PCS_EPI_RAW) return a.prologue == PCS_PRO_BWD;
  return false;
}

// fused_c5: conv5's folded input gradient as one LDS-DMA stream
inline bool c5_dgrad_takes(const pcs_gemm_args &a) {
  return !a.c_mask && !a.addend && !a.pool_w && a.A2 && a.W2 && a.pa && a.pb && a.C && a.Yp == a.A2 &&
         (!a.erstd || a.emean);
}

// Class, geometry and kernel of one pcs_gemm call.  With an empty geometry (error set) the
// kernel is still the one the operands select, as the flag checks that come first need it.
inline GemmRoute gemm_route(const pcs_gemm_args &a) {
  GemmRoute r = gemm_class(a);
  pcs_gemm_args g = a;
  g.chunks_per_scene = r.chunks_per_scene;
  if (r.cls == CLASS_STREAM && fwd_stream_takes(g)) r.kernel = GEMM_FWD_STREAM;
  else if (r.wide && gemm_wres_takes(g)) r.kernel = GEMM_WRES;
  else if (r.wide && gemm_glds_takes(g)) r.kernel = GEMM_GLDS;
  else if (r.wide && gemm_big_takes(g)) r.kernel = GEMM_BIG;
  else if (r.cls == CLASS_C5 && c5_dgrad_takes(g)) r.kernel = GEMM_C5_DGRAD;
  return r;
}

// ---------------------------------------------------------------------------------------
// pcs_wgrad and pcs_gram
// ---------------------------------------------------------------------------------------
constexpr int TN_MS_BF16 = 64, TN_MS_F32 = 16;    // gemm_tn: rows (reduction) per step
constexpr int BIGTN_TM = 256, BIGTN_TN = 256, BIGTN_MS = 64;   // gemm_big_tn
constexpr int WC5_CIN = 128, WC5_NB = 256, WC5_MS = 32;        // wgrad_c5: a4 channels, dz5 columns per WG, row step
constexpr int GRAM128_MS = 64;                    // wgrad_c5's Gram kernel: rows per step
// workgroups in the grid: two 512-thread workgroups per CU
constexpr int WC5_TARGET = 512, GRAM128_TARGET = 512, TN_TARGET = 1024;

enum WgradKernel { WGRAD_C5, WGRAD_BIG, WGRAD_TN };
enum GramKernel { GRAM_128, GRAM_BIG, GRAM_TN };
template <typename Kernel> struct TnRoute {
  Kernel kernel;
  int32_t splits_per_scene;   // the caller's when > 0, else the class's
  int64_t rows_per_split;     // in the generic kernel's row steps (wgrad_c5 takes the same value)
};
typedef TnRoute<WgradKernel> WgradRoute;
typedef TnRoute<GramKernel> GramRoute;

inline int tn_row_step(int32_t dtype) { return dtype == PCS_BF16 ? TN_MS_BF16 : TN_MS_F32; }

// the Gram of relu(bn(Y)) at C = 128 in one pass over Y (wgrad_c5.hip; pcs_gram)
inline bool gram128_class(const pcs_wgrad_args &a) {   // shapes / modes only (the split geometry)
  return a.dtype == PCS_BF16 && !(a.flags & PCS_FLAG_GENERIC) && a.dy_mode == PCS_PRO_BNRELU &&
         a.x_mode == PCS_PRO_BNRELU && a.Cin == WC5_CIN && a.Cout == WC5_CIN &&
         a.num_scenes * a.scene_rows < ((int64_t)1 << 31);
}
inline bool gram128_takes(const pcs_wgrad_args &a) { return a.Y && a.Y == a.X && a.s && a.t && !a.x_mask; }

// conv5's R = dz5^T relu(bn4(y4)) as an LDS-DMA stream (wgrad_c5.hip): bf16, dy_mode RAW
// (dZ = dz5), x_mode BNRELU without dropout bits, Cin 128, Cout a multiple of 256
inline bool wgrad_c5_class(const pcs_wgrad_args &a) {   // shapes / modes only (the split geometry)
  return a.dtype == PCS_BF16 && !(a.flags & PCS_FLAG_GENERIC) && a.dy_mode == PCS_PRO_RAW &&
         a.x_mode == PCS_PRO_BNRELU && a.Cin == WC5_CIN && a.Cout % WC5_NB == 0 &&
         a.num_scenes * a.scene_rows < ((int64_t)1 << 31);
}
inline bool wgrad_c5_takes(const pcs_wgrad_args &a) { return !a.x_mask && a.dZ && a.X && a.s && a.t; }

// wide-layer bf16 weight-gradient kernel (gemm_big_tn.hip)
inline bool wgrad_big_takes(const pcs_wgrad_args &a) {
  if (a.dy_mode == PCS_PRO_BNRELU && (a.Cout != a.Cin || a.x_mask)) return false;   // Gram: square
  return !(a.flags & PCS_FLAG_GENERIC) && a.dtype == PCS_BF16 && a.Cout % BIGTN_TM == 0 && a.Cin % BIGTN_TN == 0 &&
         a.x_mode == PCS_PRO_BNRELU &&
         (a.dy_mode == PCS_PRO_BWD || a.dy_mode == PCS_PRO_BNRELU);
}
inline int wgrad_big_tiles(const pcs_wgrad_args &a) {
  const int ntm = a.Cout / BIGTN_TM, ntn = a.Cin / BIGTN_TN;
  return a.dy_mode == PCS_PRO_BNRELU ? ntm * (ntm + 1) / 2 : ntm * ntn;
}
inline int wgrad_big_splits(const pcs_wgrad_args &a) {
  // one 512-thread workgroup per CU: pick the row splits per scene that minimise
  // (waves of 256 workgroups) / splits, i.e. the time of the slowest CU, with the fp32
  // partial slabs kept below 256 MB
  const int64_t per_split = a.num_scenes * wgrad_big_tiles(a);
  const int64_t slab = (int64_t)a.Cout * a.Cin * 4;
  int64_t max_sps = (a.scene_rows + 8 * BIGTN_MS - 1) / (8 * BIGTN_MS);
  const int64_t mem_sps = ((int64_t)256 << 20) / slab / a.num_scenes;
  if (max_sps > mem_sps) max_sps = mem_sps;
  if (max_sps < 1) max_sps = 1;
  int64_t best = 1;
  double best_cost = 1e30;
  for (int64_t sps = 1; sps <= max_sps; ++sps) {
    const double waves = (double)((per_split * sps + 255) / 256);
    const double cost = waves / (double)sps * (1.0 + 1e-3 * sps);   // tie-break: fewer slabs
    if (cost < best_cost) { best_cost = cost; best = sps; }
  }
  return (int)best;
}

// The splits of a call's class, where the caller gave none (the workspace query: shapes and
// modes; wgrad_big_takes also reads x_mask).  Needs a checked geometry (all counts > 0).
inline int32_t wgrad_class_splits(const pcs_wgrad_args &a) {
  if (a.splits_per_scene > 0) return a.splits_per_scene;
  if (wgrad_c5_class(a))
    return (int32_t)split_rows(WC5_TARGET, a.num_scenes, a.Cout / WC5_NB, a.scene_rows, WC5_MS, 4).splits;
  if (wgrad_big_takes(a)) return wgrad_big_splits(a);
  const int tm = a.Cout % 128 == 0 ? 128 : 64, tn = a.Cin % 128 == 0 ? 128 : 64;
  const int64_t ntiles = a.Cin >= 64 ? (int64_t)(a.Cout / tm) * (a.Cin / tn) : 1;
  return (int32_t)split_rows(TN_TARGET, a.num_scenes, ntiles, a.scene_rows, tn_row_step(a.dtype), 4).splits;
}

// Splits and kernel of one pcs_wgrad call.  A call of the conv5 class whose operands that kernel
// does not take runs on the generic kernel over the class's splits.
inline WgradRoute wgrad_route(const pcs_wgrad_args &a) {
  WgradRoute r = {WGRAD_TN, wgrad_class_splits(a), 0};
  r.rows_per_split = rows_per_split(a.scene_rows, r.splits_per_scene, tn_row_step(a.dtype));
  if (wgrad_c5_class(a) && wgrad_c5_takes(a)) r.kernel = WGRAD_C5;
  else if (wgrad_big_takes(a)) r.kernel = WGRAD_BIG;
  return r;
}

// pcs_gram's arguments as the pcs_wgrad_args its kernels take: dy_mode = x_mode = PRO_BNRELU, Y = X
inline pcs_wgrad_args gram_args(const void *Y, const float *s, const float *t, int64_t num_scenes,
                                int64_t scene_rows, int32_t C, int32_t dtype, int32_t sps) {
  pcs_wgrad_args a = {};
  a.num_scenes = num_scenes; a.scene_rows = scene_rows; a.Cout = C; a.Cin = C; a.dtype = dtype;
  a.splits_per_scene = sps; a.dy_mode = PCS_PRO_BNRELU; a.x_mode = PCS_PRO_BNRELU;
  a.Y = Y; a.X = Y; a.s = s; a.t = t; a.x_keep_scale = 1.f;
  return a;
}

// Splits and kernel of one pcs_gram call (pcs_wgrad itself never takes the Gram-128 kernel).
inline GramRoute gram_route(const pcs_wgrad_args &a) {
  const bool c128 = gram128_class(a);
  GramRoute r = {GRAM_TN, a.splits_per_scene, 0};
  if (r.splits_per_scene <= 0)
    r.splits_per_scene = c128 ? (int32_t)split_rows(GRAM128_TARGET, a.num_scenes, 1, a.scene_rows, GRAM128_MS, 4).splits
                              : wgrad_class_splits(a);
  r.rows_per_split = rows_per_split(a.scene_rows, r.splits_per_scene, tn_row_step(a.dtype));
  if (c128 && gram128_takes(a)) r.kernel = GRAM_128;
  else if (wgrad_big_takes(a)) r.kernel = GRAM_BIG;
  return r;
}

// ---------------------------------------------------------------------------------------
// pcs_dgrad_wgrad_bn
// ---------------------------------------------------------------------------------------
constexpr int SEG4_CB = 256, SEG4_MS = 16;   // fused_seg4: CIN columns per workgroup, rows per step
// fused_bwd's dgrad_wgrad_bn_kernel, (Cout, Cin) pairs served: (column block, rows per step).  The
// column-block split also instantiates seg_conv3 (128 x 256, CB 128, 64-row steps) and seg_conv2
// (256 x 512, CB 128, 32-row steps: 64 spill VGPRs); both are correct (tests/test_gpu_fused_bwd.py
// history) but measured no faster at cfg2 than the pcs_gemm + pcs_wgrad pair they replace (seg_conv3
// 4.96 vs 4.73 ms, seg_conv2 12.8 vs 12.6 ms: 2 TB/s, latency-bound at one workgroup per
// CU with the dy slab staged once per column block), so they stay on the pair.
// (seg_conv2 and seg_conv3 go to the LDS-DMA stream of fused_seg4.hip instead)
struct BnShape { int cout, cin, cb, ms; };
inline constexpr BnShape kBnShapes[] = {{64, 64, 64, 64}, {128, 64, 64, 64}};
constexpr const BnShape *bn_shape(int K, int Ncols) {
  for (const BnShape &b : kBnShapes)
    if (b.cout == K && b.cin == Ncols) return &b;
  return nullptr;
}

enum BnKernel { BN_SEG4, BN_64, BN_128 };
struct BnRoute {
  BnKernel kernel;
  int32_t chunks_per_scene;
  int64_t rows_per_chunk;
  const char *error;
};

// Needs num_scenes and scene_rows > 0.
inline BnRoute bn_route(const pcs_gemm_args &a) {
  // fused_seg4, shapes served: (Cout, Cin) = K x Ncols in {256 x 512 (seg_conv2), 128 x 256
  // (seg_conv3)}, bf16, PRO_BWD / EPI_DGRAD, no addend: one wave per SIMD, one WG per CU
  if (a.dtype == PCS_BF16 && !(a.flags & PCS_FLAG_GENERIC) && !a.addend &&
      ((a.K == 256 && a.Ncols == 512) || (a.K == 128 && a.Ncols == 256))) {
    const Split sp = split_rows(256, a.num_scenes, a.Ncols / SEG4_CB, a.scene_rows, SEG4_MS, 8);
    // the buffer-store range and the per-lane row offsets are 32-bit: a slice's rows (Ncols
    // bf16) below 2 GB
    if (sp.rows * (int64_t)a.Ncols * 2 < ((int64_t)1 << 31)) return {BN_SEG4, (int32_t)sp.count, sp.rows, nullptr};
  }
  const BnShape *sh = bn_shape(a.K, a.Ncols);
  if (a.dtype != PCS_BF16 || !sh || (a.flags & PCS_FLAG_GENERIC))
    return {BN_64, 0, 0, "bf16 with (Cout, Cin) = K x Ncols in {64x64, 128x64} only"};
  // 64 x 64 (conv2, conv3: <= 128 VGPRs) fits two 512-thread workgroups per CU: twice the
  // workgroups, 0.91 -> 0.85 ms at cfg2; 128 x 64 (conv4, 158-164 VGPRs) stays at one
  const Split sp = split_rows(sh->cout == 64 ? 512 : 256, a.num_scenes, sh->cin / sh->cb, a.scene_rows, sh->ms, 4);
  return {sh->cout == 64 ? BN_64 : BN_128, (int32_t)sp.count, sp.rows, nullptr};
}

// ---------------------------------------------------------------------------------------
// pcs_head (small.hip): the streamed CE head's class (head_stream.hip)
// ---------------------------------------------------------------------------------------
constexpr int HS_CIN = 128, HS_MS = 64;   // head_stream: input channels, rows per step
#ifndef HS_TARGET
#define HS_TARGET 1024
#endif
// bf16, CE mode, C <= 4, no logits out (the fused train step); shapes / modes only
inline bool head_stream_class(const pcs_head_args &a) {
  return a.dtype == PCS_BF16 && a.mode == PCS_HEAD_CE && a.num_classes >= 1 && a.num_classes <= 4 &&
         !a.logits && a.Cin == HS_CIN && a.num_scenes * a.scene_rows < ((int64_t)1 << 31);
}

}  // namespace route
