// Point <-> voxel transfer on the occupied-voxel path: the index of a point in a level of the
// voxel pyramid (its own voxel, its eight trilinear corners and their weights) and the two row
// kernels every forward and backward of voxel_mean / devoxelize (pcs_amd/pointvoxel.py) runs.
// Build-defined like the rest of the voxel vocabulary: the numpy statement is
// tests/point_voxel_refs.py.
//
//   u_d      ((p_d - lo_d) / (hi_d - lo_d)) * G, float32, the expression of voxel_of (voxel_geom.h)
//   own      row of the voxel clamp(floor(u), 0, G - 1), or -1 when the level does not hold it
//   corners  c_d = min(max(u_d, 0), G) - 0.5, b_d = floor(c_d), f_d = c_d - b_d; corner k =
//            (ax * 2 + ay) * 2 + az is the voxel b + a (-1: outside the grid or unoccupied) with
//            raw weight prod_d (a_d ? f_d : 1 - f_d), divided by the sum over the present corners
//
// Both row kernels are bandwidth-bound gathers (no MFMA, no LDS) over the lanes-of-E-elements row
// scheme of row_piece.h, for any C (lane_slot_wide), and every lane keeps several row loads in
// flight before it accumulates in fp32.  Each output row is stored once (a zero row when nothing
// contributes), nothing is added atomically, and every sum runs in a fixed order: results are
// bitwise reproducible.
#include "../../include/pcs_dense.h"
#include "row_piece.h"
#include "voxel_geom.h"
#include "voxel_hash.h"

namespace {

using namespace pcs_rows;
using pcs_geom::Box;
using pcs_hash::hash_find;

constexpr int MAX_K = 8;
constexpr int SEG_UNROLL = 4;   // row loads a lane keeps in flight along a segment

// Where the voxels of a level are: row(key) is the row of the voxel with key scene * G^3 + (ix * G +
// iy) * G + iz, or -1 when the level does not hold it.  An occupied-voxel level looks the key up in
// its hash table; a dense grid holds every cell at the row that is its key (below 2^31, checked by
// pcs_dense_trilinear_index), so it needs no table.
struct HashLevel {
  const uint64_t *tk;
  const int32_t *tv;
  uint64_t mask;
  PCS_DEV int32_t row(uint64_t key) const { return hash_find(tk, tv, mask, key); }
};
struct DenseLevel {
  PCS_DEV int32_t row(uint64_t key) const { return (int32_t)key; }
};

// one thread per point; Level is HashLevel or DenseLevel: one set of float32 expressions for both
template <class Level>
__global__ __launch_bounds__(THREADS) void trilinear_index_kernel(
    const float *__restrict__ pts, const int64_t *__restrict__ offsets, int B, int64_t T, int G, Box bx,
    Level lv, int32_t *__restrict__ own, int32_t *__restrict__ corner, float *__restrict__ weight) {
  const uint64_t G3 = (uint64_t)G * G * G;
  for (int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x; t < T; t += (int64_t)gridDim.x * THREADS) {
    int lo = 0, hi = B;   // scene: last b with offsets[b] <= t
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (offsets[mid] <= t) lo = mid; else hi = mid;
    }
    const uint64_t base = (uint64_t)lo * G3;
    int iv[3], bv[3];
    float fv[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float q = (pts[t * 4 + d] - bx.lo[d]) / (bx.hi[d] - bx.lo[d]);
      const float u = __fmul_rn(q, (float)G);
      // clamped before the conversion (same result; an out-of-range float -> int is undefined)
      const int i = (int)floorf(fminf(fmaxf(u, -1.f), (float)G));
      iv[d] = i < 0 ? 0 : (i > G - 1 ? G - 1 : i);
      // contraction off: u * G - 0.5 as one FMA rounds once and can land on the other side of
      // an integer, which would move every corner of the point
      const float c = __fsub_rn(fminf(fmaxf(u, 0.f), (float)G), 0.5f);
      const float b = floorf(c);
      bv[d] = (int)b;
      fv[d] = __fsub_rn(c, b);
    }
    own[t] = lv.row(base + ((uint64_t)iv[0] * G + iv[1]) * G + iv[2]);
    int32_t row[MAX_K];
    float raw[MAX_K], sum = 0.f;
#pragma unroll
    for (int k = 0; k < MAX_K; ++k) {
      const int ax = (k >> 2) & 1, ay = (k >> 1) & 1, az = k & 1;
      const int jx = bv[0] + ax, jy = bv[1] + ay, jz = bv[2] + az;
      int32_t r = -1;
      if (jx >= 0 && jx < G && jy >= 0 && jy < G && jz >= 0 && jz < G)
        r = lv.row(base + ((uint64_t)jx * G + jy) * G + jz);
      const float wk = (ax ? fv[0] : 1.f - fv[0]) * (ay ? fv[1] : 1.f - fv[1]) * (az ? fv[2] : 1.f - fv[2]);
      row[k] = r;
      raw[k] = r >= 0 ? wk : 0.f;
      sum += raw[k];
    }
    const float inv = sum > 0.f ? 1.f / sum : 0.f;
#pragma unroll
    for (int k = 0; k < MAX_K; ++k) {
      corner[t * MAX_K + k] = row[k];
      weight[t * MAX_K + k] = raw[k] * inv;
    }
  }
}

// Y[m] = sum_{k < K} w[m][k] * X[idx[m][k]] (idx < 0 skipped, w NULL = 1).  KT = K at compile
// time, or 0 for any K <= 8 (eight predicated slots).
template <typename XT, typename YT, int KT>
__global__ __launch_bounds__(THREADS) void rows_interp_kernel(const XT *__restrict__ X, const int32_t *__restrict__ idx,
                                                              const float *__restrict__ w, int64_t M, int K, int C,
                                                              YT *__restrict__ Y) {
  constexpr int E = Piece<XT, YT>::E;
  constexpr int SLOTS = KT ? KT : MAX_K;
  const int lpr = C / E;
  int rpb, r, c0;
  if (!lane_slot_wide(lpr, rpb, r, c0)) return;
  const int kk = KT ? KT : K;
  for (int64_t m = (int64_t)blockIdx.x * rpb + r; m < M; m += (int64_t)gridDim.x * rpb) {
    int32_t id[SLOTS];
    float wk[SLOTS];
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
      const bool in = k < kk;
      id[k] = in ? idx[m * kk + k] : -1;
      wk[k] = (in && w) ? w[m * kk + k] : 1.f;
    }
    for (int c = c0; c < lpr; c += THREADS) {
      Raw<XT, E> raw[SLOTS];
#pragma unroll
      for (int k = 0; k < SLOTS; ++k) raw_load<XT, E>(raw[k], X + (int64_t)id[k] * C + c * E, id[k] >= 0);
      float acc[E];
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = 0.f;
#pragma unroll
      for (int k = 0; k < SLOTS; ++k)
        if (id[k] >= 0) raw_fma<XT, E>(raw[k], wk[k], acc);
      store_piece<YT, E>(Y + m * C + c * E, acc);
    }
  }
}

// Y[m] = scale[m] * sum_{j in [seg_off[m], seg_off[m + 1])} w[j] * X[src[j]], ascending j (w, scale
// NULL = 1; src < 0 skipped).  One lane group walks one segment, SEG_UNROLL rows in flight.
template <typename XT, typename YT>
__global__ __launch_bounds__(THREADS) void rows_segsum_kernel(const XT *__restrict__ X, const int32_t *__restrict__ src,
                                                              const float *__restrict__ w,
                                                              const int64_t *__restrict__ seg_off,
                                                              const float *__restrict__ scale, int64_t M, int C,
                                                              YT *__restrict__ Y) {
  constexpr int E = Piece<XT, YT>::E;
  const int lpr = C / E;
  int rpb, r, c0;
  if (!lane_slot_wide(lpr, rpb, r, c0)) return;
  for (int64_t m = (int64_t)blockIdx.x * rpb + r; m < M; m += (int64_t)gridDim.x * rpb) {
    const int64_t j0 = seg_off[m], j1 = seg_off[m + 1];
    const float sc = scale ? scale[m] : 1.f;
    for (int c = c0; c < lpr; c += THREADS) {
      float acc[E];
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = 0.f;
      for (int64_t j = j0; j < j1; j += SEG_UNROLL) {
        int32_t id[SEG_UNROLL];
        float wj[SEG_UNROLL];
        Raw<XT, E> raw[SEG_UNROLL];
#pragma unroll
        for (int u = 0; u < SEG_UNROLL; ++u) {
          const bool in = j + u < j1;
          id[u] = in ? src[j + u] : -1;
          wj[u] = (in && w) ? w[j + u] : 1.f;
        }
#pragma unroll
        for (int u = 0; u < SEG_UNROLL; ++u) raw_load<XT, E>(raw[u], X + (int64_t)id[u] * C + c * E, id[u] >= 0);
#pragma unroll
        for (int u = 0; u < SEG_UNROLL; ++u)
          if (id[u] >= 0) raw_fma<XT, E>(raw[u], wj[u], acc);
      }
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] *= sc;
      store_piece<YT, E>(Y + m * C + c * E, acc);
    }
  }
}

int row_blocks(int64_t M, int32_t C, int e) {
  const int lpr = C / e;
  const int64_t rpb = lpr >= THREADS ? 1 : THREADS / lpr;
  const int64_t b = (M + rpb - 1) / rpb;
  return (int)(b < 1 ? 1 : (b > (1 << 20) ? (1 << 20) : b));
}

template <typename XT, typename YT>
void launch_interp(const void *X, const int32_t *idx, const float *w, int64_t M, int K, int C, void *Y, hipStream_t s) {
  const dim3 grid(row_blocks(M, C, Piece<XT, YT>::E)), block(THREADS);
  const XT *x = static_cast<const XT *>(X);
  YT *y = static_cast<YT *>(Y);
  if (K == 1)
    hipLaunchKernelGGL((rows_interp_kernel<XT, YT, 1>), grid, block, 0, s, x, idx, w, M, K, C, y);
  else if (K == 8)
    hipLaunchKernelGGL((rows_interp_kernel<XT, YT, 8>), grid, block, 0, s, x, idx, w, M, K, C, y);
  else
    hipLaunchKernelGGL((rows_interp_kernel<XT, YT, 0>), grid, block, 0, s, x, idx, w, M, K, C, y);
}

template <typename XT, typename YT>
void launch_segsum(const void *X, const int32_t *src, const float *w, const int64_t *seg_off, const float *scale,
                   int64_t M, int C, void *Y, hipStream_t s) {
  hipLaunchKernelGGL((rows_segsum_kernel<XT, YT>), dim3(row_blocks(M, C, Piece<XT, YT>::E)), dim3(THREADS), 0, s,
                     static_cast<const XT *>(X), src, w, seg_off, scale, M, C, static_cast<YT *>(Y));
}

}  // namespace

extern "C" int pcs_trilinear_index(const float *points, const int64_t *offsets, int64_t num_scenes, int64_t T,
                                   int32_t grid, float lo_x, float lo_y, float lo_z, float hi_x, float hi_y,
                                   float hi_z, const uint64_t *table_keys, const int32_t *table_vals,
                                   int64_t capacity, int32_t *own, int32_t *corner, float *weight,
                                   pcs_stream_t stream) {
  if (T < 0 || num_scenes < 1) return pcs_set_einval("pcs_trilinear_index", "T >= 0 and num_scenes >= 1 required");
  if (grid < 1 || grid > (1 << 20)) return pcs_set_einval("pcs_trilinear_index", "1 <= grid <= 2^20 required");
  if (capacity < 1 || (capacity & (capacity - 1)) != 0)
    return pcs_set_einval("pcs_trilinear_index", "capacity must be a power of two");
  if (!(hi_x > lo_x && hi_y > lo_y && hi_z > lo_z)) return pcs_set_einval("pcs_trilinear_index", "hi > lo required");
  if ((double)grid * grid * grid * (double)num_scenes >= 18446744073709551615.0)
    return pcs_set_einval("pcs_trilinear_index", "key overflow (num_scenes * grid^3 >= 2^64 - 1)");
  if (!offsets || !table_keys || !table_vals || (T > 0 && (!points || !own || !corner || !weight)))
    return pcs_set_einval("pcs_trilinear_index", "NULL pointer");
  if (T == 0) return 0;
  const Box b = {{lo_x, lo_y, lo_z}, {hi_x, hi_y, hi_z}};
  hipLaunchKernelGGL(trilinear_index_kernel<HashLevel>, dim3(pcs_geom::blocks_1d(T)), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), points, offsets, (int)num_scenes, T, (int)grid, b,
                     HashLevel{table_keys, table_vals, (uint64_t)(capacity - 1)}, own, corner, weight);
  PCS_CHECK_LAUNCH();
  return 0;
}

extern "C" int pcs_dense_trilinear_index(const float *points, const int64_t *offsets, int64_t num_scenes, int64_t T,
                                         int32_t grid, float lo_x, float lo_y, float lo_z, float hi_x, float hi_y,
                                         float hi_z, int32_t *own, int32_t *corner, float *weight,
                                         pcs_stream_t stream) {
  if (T < 0 || num_scenes < 1) return pcs_set_einval(__func__, "T >= 0 and num_scenes >= 1 required");
  if (grid < 1 || grid > (1 << 20)) return pcs_set_einval(__func__, "1 <= grid <= 2^20 required");
  if (!(hi_x > lo_x && hi_y > lo_y && hi_z > lo_z)) return pcs_set_einval(__func__, "hi > lo required");
  if ((double)grid * grid * grid * (double)num_scenes >= 2147483648.0)
    return pcs_set_einval(__func__, "row overflow (num_scenes * grid^3 >= 2^31)");
  if (!offsets || (T > 0 && (!points || !own || !corner || !weight))) return pcs_set_einval(__func__, "NULL pointer");
  if (T == 0) return 0;
  const Box b = {{lo_x, lo_y, lo_z}, {hi_x, hi_y, hi_z}};
  hipLaunchKernelGGL(trilinear_index_kernel<DenseLevel>, dim3(pcs_geom::blocks_1d(T)), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), points, offsets, (int)num_scenes, T, (int)grid, b,
                     DenseLevel{}, own, corner, weight);
  PCS_CHECK_LAUNCH();
  return 0;
}

extern "C" int pcs_rows_interp(const void *X, int32_t xdtype, const int32_t *idx, const float *w, int64_t M,
                               int32_t K, int32_t C, void *Y, int32_t ydtype, pcs_stream_t stream) {
  if (M < 0) return pcs_set_einval("pcs_rows_interp", "M >= 0 required");
  if (K < 1 || K > MAX_K) return pcs_set_einval("pcs_rows_interp", "1 <= K <= 8 required");
  if (const char *msg = check_width(xdtype, ydtype, C)) return pcs_set_einval("pcs_rows_interp", msg);
  if (M > 0 && (!X || !idx || !Y)) return pcs_set_einval("pcs_rows_interp", "NULL pointer");
  if (M == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for_dtype_pair(xdtype, ydtype, [&](auto x, auto y) {
    launch_interp<decltype(x), decltype(y)>(X, idx, w, M, K, C, Y, s);
  });
  PCS_CHECK_LAUNCH();
  return 0;
}

extern "C" int pcs_rows_segsum(const void *X, int32_t xdtype, const int32_t *src, const float *w,
                               const int64_t *seg_off, const float *scale, int64_t M, int32_t C, void *Y,
                               int32_t ydtype, pcs_stream_t stream) {
  if (M < 0) return pcs_set_einval("pcs_rows_segsum", "M >= 0 required");
  if (const char *msg = check_width(xdtype, ydtype, C)) return pcs_set_einval("pcs_rows_segsum", msg);
  if (M > 0 && (!X || !src || !seg_off || !Y)) return pcs_set_einval("pcs_rows_segsum", "NULL pointer");
  if (M == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for_dtype_pair(xdtype, ydtype, [&](auto x, auto y) {
    launch_segsum<decltype(x), decltype(y)>(X, src, w, seg_off, scale, M, C, Y, s);
  });
  PCS_CHECK_LAUNCH();
  return 0;
}
