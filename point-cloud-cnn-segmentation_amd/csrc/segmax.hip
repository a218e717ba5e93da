// Segmented max on the occupied-voxel path (pcs_amd/segmax.py): the max over a segment of rows with
// torch.max's pick (voxel_max over a voxel's points, the 2x2x2 max-pool over a coarse voxel's
// children) and its backward.  Build-defined like the rest of the voxel vocabulary: the numpy
// statement is tests/segmax_refs.py.
//
//   segmax     Y[m][c], arg[m][c] = the value and the source row of the pick over the rows
//              s = src[j] (src NULL: s = j), j in [seg_off[m], seg_off[m + 1]) ascending, s < 0
//              skipped: a NaN beats every number, and among equal values (or among NaNs) the
//              earliest j wins (pool_max_wins of common.h, as the running step over ascending
//              positions, pool_max_step); a segment without a present row is a zero row, arg -1
//   argselect  dX[r][c] = arg[seg_of[r]][c] == r ? dY[seg_of[r]][c] : 0, seg_of[r] < 0: a zero row;
//              the transpose of the pick when a source row belongs to at most one segment
//
// Both are bandwidth-bound row kernels (no MFMA, no LDS, no atomics) over the lanes-of-E-elements
// row scheme of row_piece.h, for any C (lane_slot_wide); the walk of a segment keeps SEG_UNROLL row
// loads in flight, as pointvoxel.hip's rows_segsum_kernel does.  Values are compared in fp32 (bf16
// inputs are exact); every output row is stored exactly once, so results are bitwise reproducible.
#include <limits.h>

#include "../../include/pcs_segmax.h"
#include "row_piece.h"

namespace {

using namespace pcs_rows;

constexpr int SEG_UNROLL = 4;   // row loads a lane keeps in flight along a segment

template <int E>
PCS_DEV void store_index_piece(int32_t *__restrict__ p, const int (&v)[E]) {
#pragma unroll
  for (int i = 0; i < E / 4; ++i)
    reinterpret_cast<u32x4 *>(p)[i] = mk_u32x4((unsigned)v[4 * i], (unsigned)v[4 * i + 1], (unsigned)v[4 * i + 2],
                                               (unsigned)v[4 * i + 3]);
}

template <int E>
PCS_DEV void load_index_piece(const int32_t *__restrict__ p, bool present, int (&v)[E]) {
#pragma unroll
  for (int i = 0; i < E / 4; ++i) {
    const u32x4 q = present ? reinterpret_cast<const u32x4 *>(p)[i] : mk_u32x4(~0u, ~0u, ~0u, ~0u);
    v[4 * i] = (int)q.x; v[4 * i + 1] = (int)q.y; v[4 * i + 2] = (int)q.z; v[4 * i + 3] = (int)q.w;
  }
}

// One lane group walks one segment.  pick[e] is the source row of the running pick of channel e,
// PCS_POOL_NONE until the first present row (which always makes a pick: a segment of -inf gives -inf).
template <typename XT, typename YT>
__global__ __launch_bounds__(THREADS) void rows_segmax_kernel(const XT *__restrict__ X, const int32_t *__restrict__ src,
                                                              const int64_t *__restrict__ seg_off, int64_t M, int C,
                                                              YT *__restrict__ Y, int32_t *__restrict__ arg) {
  constexpr int E = Piece<XT, YT>::E;
  const int lpr = C / E;
  int rpb, r, c0;
  if (!lane_slot_wide(lpr, rpb, r, c0)) return;
  for (int64_t m = (int64_t)blockIdx.x * rpb + r; m < M; m += (int64_t)gridDim.x * rpb) {
    const int64_t j0 = seg_off[m], j1 = seg_off[m + 1];
    for (int c = c0; c < lpr; c += THREADS) {
      float best[E];
      int pick[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        best[e] = 0.f;
        pick[e] = PCS_POOL_NONE;
      }
      for (int64_t j = j0; j < j1; j += SEG_UNROLL) {
        int32_t id[SEG_UNROLL];
        Raw<XT, E> raw[SEG_UNROLL];
#pragma unroll
        for (int u = 0; u < SEG_UNROLL; ++u) {
          const bool in = j + u < j1;
          id[u] = in ? (src ? src[j + u] : (int32_t)(j + u)) : -1;
        }
#pragma unroll
        for (int u = 0; u < SEG_UNROLL; ++u) raw_load<XT, E>(raw[u], X + (int64_t)id[u] * C + c * E, id[u] >= 0);
#pragma unroll
        for (int u = 0; u < SEG_UNROLL; ++u) {
          if (id[u] >= 0) {
            float v[E];
            raw_unpack<XT, E>(raw[u], v);
#pragma unroll
            for (int e = 0; e < E; ++e) {
              const bool wins = pool_max_step(v[e], best[e], pick[e]);
              best[e] = wins ? v[e] : best[e];
              pick[e] = wins ? id[u] : pick[e];
            }
          }
        }
      }
#pragma unroll
      for (int e = 0; e < E; ++e) pick[e] = pick[e] == PCS_POOL_NONE ? -1 : pick[e];   // (best is still 0)
      store_piece<YT, E>(Y + m * C + c * E, best);
      if (arg) store_index_piece<E>(arg + m * C + c * E, pick);
    }
  }
}

// one lane group per source row
template <typename DT, typename XT>
__global__ __launch_bounds__(THREADS) void rows_argselect_kernel(const DT *__restrict__ dY, const int32_t *__restrict__ arg,
                                                                 const int32_t *__restrict__ seg_of, int64_t R, int C,
                                                                 XT *__restrict__ dX) {
  constexpr int E = Piece<DT, XT>::E;
  const int lpr = C / E;
  int rpb, r0, c0;
  if (!lane_slot_wide(lpr, rpb, r0, c0)) return;
  for (int64_t r = (int64_t)blockIdx.x * rpb + r0; r < R; r += (int64_t)gridDim.x * rpb) {
    const int32_t m = seg_of[r];
    for (int c = c0; c < lpr; c += THREADS) {
      Raw<DT, E> rd;
      int a[E];
      raw_load<DT, E>(rd, dY + (int64_t)m * C + c * E, m >= 0);
      load_index_piece<E>(arg + (int64_t)m * C + c * E, m >= 0, a);
      float d[E];
      raw_unpack<DT, E>(rd, d);
#pragma unroll
      for (int e = 0; e < E; ++e) d[e] = a[e] == (int)r ? d[e] : 0.f;
      store_piece<XT, E>(dX + r * C + c * E, d);
    }
  }
}

int row_blocks(int64_t M, int32_t C, int e) {
  const int lpr = C / e;
  const int64_t rpb = lpr >= THREADS ? 1 : THREADS / lpr;
  const int64_t b = (M + rpb - 1) / rpb;
  return (int)(b < 1 ? 1 : (b > (1 << 20) ? (1 << 20) : b));
}

}  // namespace

extern "C" int pcs_rows_segmax(const void *X, int32_t xdtype, const int32_t *src, const int64_t *seg_off, int64_t M,
                               int32_t C, void *Y, int32_t ydtype, int32_t *arg, pcs_stream_t stream) {
  if (M < 0) return pcs_set_einval("pcs_rows_segmax", "M >= 0 required");
  if (const char *msg = check_width(xdtype, ydtype, C)) return pcs_set_einval("pcs_rows_segmax", msg);
  if (M > 0 && (!X || !seg_off || !Y)) return pcs_set_einval("pcs_rows_segmax", "NULL pointer");
  if (M == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for_dtype_pair(xdtype, ydtype, [&](auto x, auto y) {
    using XT = decltype(x);
    using YT = decltype(y);
    hipLaunchKernelGGL((rows_segmax_kernel<XT, YT>), dim3(row_blocks(M, C, Piece<XT, YT>::E)), dim3(THREADS), 0, s,
                       static_cast<const XT *>(X), src, seg_off, M, (int)C, static_cast<YT *>(Y), arg);
  });
  PCS_CHECK_LAUNCH();
  return 0;
}

extern "C" int pcs_rows_argselect(const void *dY, int32_t dydtype, const int32_t *arg, const int32_t *seg_of, int64_t R,
                                  int32_t C, void *dX, int32_t dxdtype, pcs_stream_t stream) {
  if (R < 0 || R > INT_MAX) return pcs_set_einval("pcs_rows_argselect", "0 <= R < 2^31 required (arg holds int32 rows)");
  if (const char *msg = check_width(dydtype, dxdtype, C)) return pcs_set_einval("pcs_rows_argselect", msg);
  if (R > 0 && (!dY || !arg || !seg_of || !dX)) return pcs_set_einval("pcs_rows_argselect", "NULL pointer");
  if (R == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for_dtype_pair(dydtype, dxdtype, [&](auto d, auto x) {
    using DT = decltype(d);
    using XT = decltype(x);
    hipLaunchKernelGGL((rows_argselect_kernel<DT, XT>), dim3(row_blocks(R, C, Piece<DT, XT>::E)), dim3(THREADS), 0, s,
                       static_cast<const DT *>(dY), arg, seg_of, R, (int)C, static_cast<XT *>(dX));
  });
  PCS_CHECK_LAUNCH();
  return 0;
}
