// Walks csrc/route.h over the cases of tests/golden/routes.json (tests/test_routes.py): one case
// per input line, one line of route per case.  Plain C++17, no HIP, no device; the pointers are
// dummy non-null values that nothing dereferences.
//   g dtype pro epi flags K Ncols K1 rows scenes cps pool_c pool_ldw mask   -> class kernel cps rows_per_chunk error
//   w dtype dy_mode x_mode flags Cout Cin rows scenes splits mask          -> kernel splits workspace_bytes
//   r dtype C rows scenes mask (Y, s, t)                                   -> kernel splits workspace_bytes
//   b dtype flags K Ncols rows scenes mask                                 -> kernel cps workspace_bytes error
// mask (hex): bit i = the i-th pointer field of the struct, in declaration order, is set; the bits
// after the last field make Yp equal A, Yp equal A2 (pcs_gemm_args) or Y equal X (pcs_wgrad_args).
#include <cinttypes>
#include <cstdio>

#include "route.h"

// the enumerators of route.h, in order
static const char *const GEMM_CLASS[] = {"stream", "wide", "c5", "nt"};
static const char *const GEMM_KERNEL[] = {"fwd_stream", "gemm_wres", "gemm_glds", "gemm_big", "c5_dgrad", "gemm_nt"};
static const char *const WGRAD_KERNEL[] = {"wgrad_c5", "wgrad_big", "wgrad_tn"};
static const char *const GRAM_KERNEL[] = {"gram128", "wgrad_big", "wgrad_tn"};
static const char *const BN_KERNEL[] = {"seg4", "bn64", "bn128"};
static_assert(route::CLASS_NT == 3 && route::GEMM_NT == 5 && route::WGRAD_TN == 2 && route::GRAM_TN == 2 &&
              route::BN_128 == 2, "route.h's enumerators");

template <typename T> static void set(T *&p, unsigned long long mask, int bit) {
  p = (mask >> bit) & 1 ? reinterpret_cast<T *>((uintptr_t)0x1000 * (bit + 1)) : nullptr;
}

static void gemm_pointers(pcs_gemm_args &a, unsigned long long m) {
  int i = 0;
  set(a.A, m, i++); set(a.A2, m, i++); set(a.pa, m, i++); set(a.pb, m, i++); set(a.pc, m, i++);
  set(a.a_mask, m, i++); set(a.pool_idx, m, i++); set(a.pool_coef, m, i++); set(a.W, m, i++); set(a.C, m, i++);
  set(a.bias, m, i++); set(a.scene_bias, m, i++); set(a.addend, m, i++); set(a.c_mask, m, i++); set(a.Yp, m, i++);
  set(a.es, m, i++); set(a.et, m, i++); set(a.emean, m, i++); set(a.erstd, m, i++); set(a.stats, m, i++);
  set(a.pool, m, i++); set(a.pool_w, m, i++); set(a.w_scale, m, i++); set(a.W2, m, i++); set(a.gram, m, i++);
  if ((m >> i++) & 1) a.Yp = a.A;
  if ((m >> i++) & 1) a.Yp = a.A2;
}

int main() {
  char kind;
  while (scanf(" %c", &kind) == 1) {
    unsigned long long m;
    if (kind == 'g') {
      pcs_gemm_args a = {};
      if (scanf("%d %d %d %d %d %d %d %" SCNd64 " %" SCNd64 " %d %d %" SCNd64 " %llx", &a.dtype, &a.prologue, &a.epilogue,
                &a.flags, &a.K, &a.Ncols, &a.K1, &a.scene_rows, &a.num_scenes, &a.chunks_per_scene, &a.pool_c,
                &a.pool_ldw, &m) != 13)
        return 1;
      gemm_pointers(a, m);
      const route::GemmRoute r = route::gemm_route(a);
      printf("%s %s %d %" PRId64 " %s\n", GEMM_CLASS[r.cls], GEMM_KERNEL[r.kernel], r.chunks_per_scene,
             r.rows_per_chunk, r.error ? r.error : "-");
    } else if (kind == 'w') {
      pcs_wgrad_args a = {};
      if (scanf("%d %d %d %d %d %d %" SCNd64 " %" SCNd64 " %d %llx", &a.dtype, &a.dy_mode, &a.x_mode, &a.flags, &a.Cout,
                &a.Cin, &a.scene_rows, &a.num_scenes, &a.splits_per_scene, &m) != 10)
        return 1;
      int i = 0;
      set(a.dZ, m, i++); set(a.Y, m, i++); set(a.alpha, m, i++); set(a.beta, m, i++); set(a.gamma, m, i++);
      set(a.reserved0, m, i++); set(a.reserved1, m, i++); set(a.X, m, i++); set(a.s, m, i++); set(a.t, m, i++);
      set(a.x_mask, m, i++); set(a.partial, m, i++); set(a.dW, m, i++); set(a.reserved2, m, i++);
      if ((m >> i++) & 1) a.Y = a.X;
      const route::WgradRoute r = route::wgrad_route(a);
      printf("%s %d %" PRId64 "\n", WGRAD_KERNEL[r.kernel], r.splits_per_scene,
             a.num_scenes * r.splits_per_scene * a.Cout * a.Cin * 4);
    } else if (kind == 'r') {
      int32_t dtype, C;
      int64_t rows, scenes;
      if (scanf("%d %d %" SCNd64 " %" SCNd64 " %llx", &dtype, &C, &rows, &scenes, &m) != 5) return 1;
      const void *Y;
      const float *s, *t;
      set(Y, m, 0); set(s, m, 1); set(t, m, 2);
      const route::GramRoute r = route::gram_route(route::gram_args(Y, s, t, scenes, rows, C, dtype, 0));
      printf("%s %d %" PRId64 "\n", GRAM_KERNEL[r.kernel], r.splits_per_scene,
             scenes * r.splits_per_scene * ((int64_t)C * C + C) * 4);
    } else if (kind == 'b') {
      pcs_gemm_args a = {};
      if (scanf("%d %d %d %d %" SCNd64 " %" SCNd64 " %llx", &a.dtype, &a.flags, &a.K, &a.Ncols, &a.scene_rows,
                &a.num_scenes, &m) != 7)
        return 1;
      gemm_pointers(a, m);
      const route::BnRoute r = route::bn_route(a);
      printf("%s %d %" PRId64 " %s\n", BN_KERNEL[r.kernel], r.chunks_per_scene,
             a.num_scenes * r.chunks_per_scene * a.K * a.Ncols * 4, r.error ? r.error : "-");
    } else {
      return 1;
    }
  }
  return 0;
}
