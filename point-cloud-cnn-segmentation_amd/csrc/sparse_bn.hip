// BatchNorm (+ residual) (+ ReLU) on the occupied-voxel path: the normalisation / activation layer
// between the sparse convolutions (pcs_amd/sparse_norm.py), forward and backward, on a flat row
// array X [V, C] (the per-voxel features of one level; no scene structure).  Build-defined like the
// rest of the voxel vocabulary: the numpy statement is tests/sparse_norm_refs.py.
//
//   stats       per-block (mean, M2) of X's columns: per-thread Welford, Chan-merged in the block
//               (colstats_kernel's scheme), merged over the blocks by pcs_bn_fwd_finalize
//   apply       y = act(fma(x, scale[c], shift[c]) (+ r)),  act = relu or the identity
//   bwd_reduce  dz = relu ? (y > 0 ? dy : 0) : dy, stored; per-block S1 = sum dz,
//               S2 = sum dz (x - mean) rstd, summed over the blocks by pcs_bn_bwd_finalize
//   bwd_apply   dx = fma(alpha[c], dz, fma(gamma_c[c], x, beta_c[c]))
//
// All four are bandwidth-bound streams (no MFMA) over the lanes-of-E-elements row scheme of
// row_piece.h, and every lane issues the loads of UNROLL passes before it uses the first.
// Arithmetic is fp32.  Nothing is added atomically, every output row is stored once and every sum
// runs in a fixed order: results are bitwise reproducible.
#include "row_piece.h"

namespace {

using namespace pcs_rows;

constexpr int UNROLL = 4;   // row passes a lane keeps in flight

// rows lo + j, lo + j + rpp, ... below lo + n: how many slot j reads (per = n / rpp, rem = n % rpp)
PCS_DEV float slot_rows(int64_t per, int rem, int j) { return (float)(per + (j < rem ? 1 : 0)); }

template <typename XT, int E>
__global__ __launch_bounds__(THREADS) void sbn_stats_kernel(const XT *__restrict__ X, int64_t V, int C, int64_t rpb,
                                                            float *__restrict__ stats) {
  __shared__ float sm[2][E][THREADS];
  int rpp, r0, cc;
  const int lpr = C / E, tid = threadIdx.x;
  const bool active = lane_slot(lpr, rpp, r0, cc);
  const int64_t lo = (int64_t)blockIdx.x * rpb, hi = pcs_min64(lo + rpb, V);
  float mean[E], m2[E], cnt = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) { mean[e] = 0.f; m2[e] = 0.f; }
  if (active) {
    const XT *base = X + cc * E;
    for (int64_t r = lo + r0; r < hi; r += (int64_t)rpp * UNROLL) {
      Raw<XT, E> raw[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t row = r + (int64_t)u * rpp;
        raw_load<XT, E>(raw[u], base + row * C, row < hi);
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        if (r + (int64_t)u * rpp < hi) {
          float v[E];
          raw_unpack<XT, E>(raw[u], v);
          cnt += 1.f;
          const float rn = 1.f / cnt;
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const float d = v[e] - mean[e];
            mean[e] = fmaf(d, rn, mean[e]);
            m2[e] = fmaf(d, v[e] - mean[e], m2[e]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) { sm[0][e][tid] = mean[e]; sm[1][e][tid] = m2[e]; }
  __syncthreads();
  // one thread per column merges the rpp slots that share it, in slot order
  for (int c = tid; c < C; c += THREADS) {
    const int pc = c / E, e = c - pc * E;
    const int64_t per = (hi - lo) / rpp;
    const int rem = (int)((hi - lo) - per * rpp);
    float n = 0.f, mu = 0.f, q = 0.f;
    for (int j = 0; j < rpp; ++j)
      chan_merge(n, mu, q, slot_rows(per, rem, j), sm[0][e][j * lpr + pc], sm[1][e][j * lpr + pc]);
    *reinterpret_cast<float2 *>(stats + ((int64_t)blockIdx.x * C + c) * 2) = make_float2(mu, q);
  }
}

template <typename XT, typename YT>
__global__ __launch_bounds__(THREADS) void sbn_apply_kernel(const XT *__restrict__ X, const YT *__restrict__ R,
                                                            const float *__restrict__ scale,
                                                            const float *__restrict__ shift, int act, int64_t V, int C,
                                                            YT *__restrict__ Y) {
  constexpr int E = Piece<XT, YT>::E;
  int rpp, r0, cc;
  if (!lane_slot(C / E, rpp, r0, cc)) return;
  const int c0 = cc * E;
  float s[E], t[E];
  load_vec<E>(scale, c0, s);
  load_vec<E>(shift, c0, t);
  const int64_t step = (int64_t)rpp * UNROLL;
  for (int64_t r = (int64_t)blockIdx.x * step + r0; r < V; r += (int64_t)gridDim.x * step) {
    Raw<XT, E> rx[UNROLL];
    Raw<YT, E> rr[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t row = r + (int64_t)u * rpp;
      raw_load<XT, E>(rx[u], X + row * C + c0, row < V);
      raw_load<YT, E>(rr[u], R + row * C + c0, R != nullptr && row < V);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t row = r + (int64_t)u * rpp;
      if (row < V) {
        float x[E], a[E];
        raw_unpack<XT, E>(rx[u], x);
        raw_unpack<YT, E>(rr[u], a);   // zeros without a residual
#pragma unroll
        for (int e = 0; e < E; ++e) {
          float pre = fmaf(x[e], s[e], t[e]);
          if (R) pre += a[e];
          x[e] = act ? relu(pre) : pre;
        }
        store_piece<YT, E, true>(Y + row * C + c0, x);
      }
    }
  }
}

template <typename XT, typename YT>
__global__ __launch_bounds__(THREADS) void sbn_bwd_reduce_kernel(const YT *__restrict__ dY, const YT *__restrict__ Y,
                                                                 const XT *__restrict__ X,
                                                                 const float *__restrict__ mean,
                                                                 const float *__restrict__ rstd, int act, int64_t V,
                                                                 int C, int64_t rpb, YT *__restrict__ DZ,
                                                                 float *__restrict__ stats) {
  constexpr int E = Piece<XT, YT>::E;
  __shared__ float sm[2][E][THREADS];
  int rpp, r0, cc;
  const int lpr = C / E, tid = threadIdx.x;
  const bool active = lane_slot(lpr, rpp, r0, cc);
  const int64_t lo = (int64_t)blockIdx.x * rpb, hi = pcs_min64(lo + rpb, V);
  float s1[E], s2[E];
#pragma unroll
  for (int e = 0; e < E; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
  if (active) {
    const int c0 = cc * E;
    float mu[E], rs[E];
    load_vec<E>(mean, c0, mu);
    load_vec<E>(rstd, c0, rs);
    for (int64_t r = lo + r0; r < hi; r += (int64_t)rpp * UNROLL) {
      Raw<YT, E> rd[UNROLL], ry[UNROLL];
      Raw<XT, E> rx[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t row = r + (int64_t)u * rpp;
        const bool in = row < hi;
        raw_load<YT, E>(rd[u], dY + row * C + c0, in);
        raw_load<YT, E>(ry[u], Y + row * C + c0, in && act);
        raw_load<XT, E>(rx[u], X + row * C + c0, in);
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t row = r + (int64_t)u * rpp;
        if (row < hi) {
          float dz[E], y[E], x[E];
          raw_unpack<YT, E>(rd[u], dz);
          raw_unpack<YT, E>(ry[u], y);
          raw_unpack<XT, E>(rx[u], x);
#pragma unroll
          for (int e = 0; e < E; ++e) {
            if (act) dz[e] = y[e] > 0.f ? dz[e] : 0.f;
            s1[e] += dz[e];
            s2[e] = fmaf(dz[e], (x[e] - mu[e]) * rs[e], s2[e]);
          }
          if (DZ) store_piece<YT, E, true>(DZ + row * C + c0, dz);
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) { sm[0][e][tid] = s1[e]; sm[1][e][tid] = s2[e]; }
  __syncthreads();
  for (int c = tid; c < C; c += THREADS) {
    const int pc = c / E, e = c - pc * E;
    float a1 = 0.f, a2 = 0.f;
    for (int j = 0; j < rpp; ++j) { a1 += sm[0][e][j * lpr + pc]; a2 += sm[1][e][j * lpr + pc]; }
    *reinterpret_cast<float2 *>(stats + ((int64_t)blockIdx.x * C + c) * 2) = make_float2(a1, a2);
  }
}

template <typename XT, typename YT>
__global__ __launch_bounds__(THREADS) void sbn_bwd_apply_kernel(const YT *__restrict__ DZ, const XT *__restrict__ X,
                                                                const float *__restrict__ alpha,
                                                                const float *__restrict__ beta_c,
                                                                const float *__restrict__ gamma_c, int64_t V, int C,
                                                                XT *__restrict__ dX) {
  constexpr int E = Piece<XT, YT>::E;
  int rpp, r0, cc;
  if (!lane_slot(C / E, rpp, r0, cc)) return;
  const int c0 = cc * E;
  float ca[E], cb[E], cg[E];
  load_vec<E>(alpha, c0, ca);
  load_vec<E>(beta_c, c0, cb);
  load_vec<E>(gamma_c, c0, cg);
  const int64_t step = (int64_t)rpp * UNROLL;
  for (int64_t r = (int64_t)blockIdx.x * step + r0; r < V; r += (int64_t)gridDim.x * step) {
    Raw<YT, E> rd[UNROLL];
    Raw<XT, E> rx[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t row = r + (int64_t)u * rpp;
      raw_load<YT, E>(rd[u], DZ + row * C + c0, row < V);
      raw_load<XT, E>(rx[u], X + row * C + c0, row < V);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t row = r + (int64_t)u * rpp;
      if (row < V) {
        float dz[E], x[E];
        raw_unpack<YT, E>(rd[u], dz);
        raw_unpack<XT, E>(rx[u], x);
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = fmaf(ca[e], dz[e], fmaf(cg[e], x[e], cb[e]));
        store_piece<XT, E, true>(dX + row * C + c0, x);
      }
    }
  }
}

// the blocks tile [0, V) and none is empty
const char *check_blocks(int64_t V, int32_t num_blocks, int64_t rows_per_block) {
  if (num_blocks < 1 || rows_per_block < 1) return "num_blocks >= 1 and rows_per_block >= 1 required";
  if ((V - 1) / rows_per_block + 1 != num_blocks)   // ceil(V / rows_per_block), V >= 1
    return "geometry leaves an empty block or misses rows (take it from pcs_sparse_bn_geometry)";
  return nullptr;
}

// grid of the two elementwise passes: UNROLL passes of rpp rows per block and loop trip
int stream_blocks(int64_t V, int32_t C, int e) {
  const int64_t step = (int64_t)(THREADS / (C / e)) * UNROLL;
  const int64_t b = (V + step - 1) / step;
  return (int)(b > (1 << 16) ? (1 << 16) : b);
}

}  // namespace

extern "C" int64_t pcs_sparse_bn_geometry(int64_t V, int32_t C, int32_t *num_blocks) {
  if (!num_blocks) return pcs_set_einval("pcs_sparse_bn_geometry", "NULL pointer");
  if (V < 0) return pcs_set_einval("pcs_sparse_bn_geometry", "V >= 0 required");
  if (C < 4 || C % 4 != 0 || C > MAX_C)
    return pcs_set_einval("pcs_sparse_bn_geometry", "C % 4 == 0, 4 <= C <= 1024 required");
  const Blocks b = reduction_blocks(V, ROW_TILE);
  *num_blocks = b.n;   // 0 for an empty level
  return b.per;
}

extern "C" int pcs_sparse_bn_stats(const void *X, int32_t xdtype, int64_t V, int32_t C, int32_t num_blocks,
                                   int64_t rows_per_block, float *stats, pcs_stream_t stream) {
  if (V < 0) return pcs_set_einval("pcs_sparse_bn_stats", "V >= 0 required");
  if (const char *msg = check_width(xdtype, xdtype, C, true)) return pcs_set_einval("pcs_sparse_bn_stats", msg);
  if (V == 0) return 0;
  if (!X || !stats) return pcs_set_einval("pcs_sparse_bn_stats", "NULL pointer");
  if (const char *msg = check_blocks(V, num_blocks, rows_per_block)) return pcs_set_einval("pcs_sparse_bn_stats", msg);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (xdtype == PCS_BF16)
    hipLaunchKernelGGL((sbn_stats_kernel<bf16_t, 8>), dim3(num_blocks), dim3(THREADS), 0, s,
                       static_cast<const bf16_t *>(X), V, (int)C, rows_per_block, stats);
  else
    hipLaunchKernelGGL((sbn_stats_kernel<float, 4>), dim3(num_blocks), dim3(THREADS), 0, s,
                       static_cast<const float *>(X), V, (int)C, rows_per_block, stats);
  PCS_CHECK_LAUNCH();
  return 0;
}

extern "C" int pcs_sparse_bn_apply(const void *X, int32_t xdtype, const void *R, const float *scale,
                                   const float *shift, int32_t relu, int64_t V, int32_t C, void *Y, int32_t ydtype,
                                   pcs_stream_t stream) {
  if (V < 0) return pcs_set_einval("pcs_sparse_bn_apply", "V >= 0 required");
  if (const char *msg = check_width(xdtype, ydtype, C, true)) return pcs_set_einval("pcs_sparse_bn_apply", msg);
  if (V == 0) return 0;
  if (!X || !scale || !shift || !Y) return pcs_set_einval("pcs_sparse_bn_apply", "NULL pointer");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for_dtype_pair(xdtype, ydtype, [&](auto x, auto y) {
    using XT = decltype(x);
    using YT = decltype(y);
    hipLaunchKernelGGL((sbn_apply_kernel<XT, YT>), dim3(stream_blocks(V, C, Piece<XT, YT>::E)), dim3(THREADS), 0, s,
                       static_cast<const XT *>(X), static_cast<const YT *>(R), scale, shift, (int)(relu != 0), V,
                       (int)C, static_cast<YT *>(Y));
  });
  PCS_CHECK_LAUNCH();
  return 0;
}

extern "C" int pcs_sparse_bn_bwd_reduce(const void *dY, const void *Y, int32_t ydtype, const void *X, int32_t xdtype,
                                        const float *mean, const float *rstd, int32_t relu, int64_t V, int32_t C,
                                        int32_t num_blocks, int64_t rows_per_block, void *DZ, float *stats,
                                        pcs_stream_t stream) {
  if (V < 0) return pcs_set_einval("pcs_sparse_bn_bwd_reduce", "V >= 0 required");
  if (const char *msg = check_width(xdtype, ydtype, C, true)) return pcs_set_einval("pcs_sparse_bn_bwd_reduce", msg);
  if (V == 0) return 0;
  if (!dY || !X || !mean || !rstd || !stats) return pcs_set_einval("pcs_sparse_bn_bwd_reduce", "NULL pointer");
  if (relu && (!Y || !DZ))
    return pcs_set_einval("pcs_sparse_bn_bwd_reduce", "NULL pointer (Y and DZ are required with relu)");
  if (const char *msg = check_blocks(V, num_blocks, rows_per_block))
    return pcs_set_einval("pcs_sparse_bn_bwd_reduce", msg);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for_dtype_pair(xdtype, ydtype, [&](auto x, auto y) {
    using XT = decltype(x);
    using YT = decltype(y);
    hipLaunchKernelGGL((sbn_bwd_reduce_kernel<XT, YT>), dim3(num_blocks), dim3(THREADS), 0, s,
                       static_cast<const YT *>(dY), static_cast<const YT *>(Y), static_cast<const XT *>(X), mean,
                       rstd, (int)(relu != 0), V, (int)C, rows_per_block, static_cast<YT *>(DZ), stats);
  });
  PCS_CHECK_LAUNCH();
  return 0;
}

extern "C" int pcs_sparse_bn_bwd_apply(const void *DZ, int32_t ydtype, const void *X, int32_t xdtype,
                                       const float *alpha, const float *beta_c, const float *gamma_c, int64_t V,
                                       int32_t C, void *dX, pcs_stream_t stream) {
  if (V < 0) return pcs_set_einval("pcs_sparse_bn_bwd_apply", "V >= 0 required");
  if (const char *msg = check_width(xdtype, ydtype, C, true)) return pcs_set_einval("pcs_sparse_bn_bwd_apply", msg);
  if (V == 0) return 0;
  if (!DZ || !X || !alpha || !beta_c || !gamma_c || !dX)
    return pcs_set_einval("pcs_sparse_bn_bwd_apply", "NULL pointer");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for_dtype_pair(xdtype, ydtype, [&](auto x, auto y) {
    using XT = decltype(x);
    using YT = decltype(y);
    hipLaunchKernelGGL((sbn_bwd_apply_kernel<XT, YT>), dim3(stream_blocks(V, C, Piece<XT, YT>::E)), dim3(THREADS), 0,
                       s, static_cast<const YT *>(DZ), static_cast<const XT *>(X), alpha, beta_c, gamma_c, V, (int)C,
                       static_cast<XT *>(dX));
  });
  PCS_CHECK_LAUNCH();
  return 0;
}
