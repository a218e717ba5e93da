// Occupied-voxel (sparse) indexing for the north star's "sparse occupied-only voxel path
// (hash-indexed gather)" (BASELINE configs[2]).  Build-defined: the reference has no
// voxel grid, so the oracle is oracle/sparse_oracle.py (numpy, dict-based), "not reference parity".
//
//   key          scene * G^3 + (ix * G + iy) * G + iz, the voxel key of voxel.hip (voxel_of, voxel_geom.h)
//   hash table   open addressing over a power-of-two capacity (>= 2 n): slot = mix(key) & (cap-1),
//                linear probing; keys inserted with a 64-bit compare-and-swap, the value is the
//                voxel's row.  Keys are unique, so the final table (which slot holds which key)
//                can depend on insertion order but every lookup result cannot.
//   neighbours   nbr[v][t] = row of the voxel at (ix + a - 1, iy + b - 1, iz + c - 1) of the same
//                scene, t = (a * 3 + b) * 3 + c, or -1 (empty or outside the grid): the 27 taps of
//                a 3x3x3 submanifold convolution in the tap order of a torch Conv3d weight
//                [Cout, Cin, 3, 3, 3] applied to a dense [B, C, G(x), G(y), G(z)] grid.
//   coarse level the occupied 2x2x2 cells of an even grid (key of the cell on the G / 2 grid) and
//                the child / parent / up maps of a k = 2, s = 2 convolution between the levels
#include "common.h"
#include "voxel_geom.h"
#include "voxel_hash.h"

namespace {

using pcs_geom::blocks_1d;
using pcs_geom::Box;
using pcs_geom::voxel_of;
using pcs_hash::EMPTY;
using pcs_hash::hash_find;
using pcs_hash::mix64;

constexpr int THREADS = 256;

// keys[voxel_of_point[p]] = key of p (every point of a voxel writes the same value)
__global__ __launch_bounds__(THREADS) void voxel_keys_kernel(const float *__restrict__ pts,
                                                             const int64_t *__restrict__ offsets, int B, int64_t T,
                                                             int G, Box b, const int64_t *__restrict__ vop,
                                                             uint64_t *__restrict__ keys) {
  const uint64_t G3 = (uint64_t)G * G * G;
  for (int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x; t < T; t += (int64_t)gridDim.x * THREADS) {
    int lo = 0, hi = B;   // scene: last b with offsets[b] <= t
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (offsets[mid] <= t) lo = mid; else hi = mid;
    }
    keys[vop[t]] = (uint64_t)lo * G3 + (uint64_t)voxel_of(pts + t * 4, G, b);
  }
}

__global__ __launch_bounds__(THREADS) void hash_clear_kernel(uint64_t *__restrict__ tk, int32_t *__restrict__ tv, int64_t cap) {
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < cap; i += (int64_t)gridDim.x * THREADS) {
    tk[i] = EMPTY;
    tv[i] = -1;
  }
}

// every probe sequence ends: the capacity is at least twice the key count, so an empty slot or
// the key itself is always found within cap probes
__global__ __launch_bounds__(THREADS) void hash_insert_kernel(const uint64_t *__restrict__ keys, int64_t n,
                                                              unsigned long long *__restrict__ tk,
                                                              int32_t *__restrict__ tv, uint64_t mask) {
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
    const uint64_t k = keys[i];
    uint64_t h = mix64(k) & mask;
    for (uint64_t probe = 0; probe <= mask; ++probe) {
      const unsigned long long prev = atomicCAS(tk + h, (unsigned long long)EMPTY, (unsigned long long)k);
      if (prev == EMPTY || prev == k) {
        tv[h] = (int32_t)i;
        break;
      }
      h = (h + 1) & mask;
    }
  }
}

__global__ __launch_bounds__(THREADS) void hash_find_kernel(const uint64_t *__restrict__ tk, const int32_t *__restrict__ tv,
                                                            uint64_t mask, const uint64_t *__restrict__ q, int64_t nq,
                                                            int32_t *__restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < nq; i += (int64_t)gridDim.x * THREADS)
    out[i] = hash_find(tk, tv, mask, q[i]);
}

// one thread per (voxel, tap)
__global__ __launch_bounds__(THREADS) void neighbors_kernel(const uint64_t *__restrict__ tk, const int32_t *__restrict__ tv,
                                                            uint64_t mask, const uint64_t *__restrict__ keys, int64_t n,
                                                            int G, int32_t *__restrict__ nbr) {
  const uint64_t G3 = (uint64_t)G * G * G;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n * 27; i += (int64_t)gridDim.x * THREADS) {
    const int64_t v = i / 27;
    const int t = (int)(i - v * 27);
    const uint64_t k = keys[v];
    const uint64_t scene = k / G3, loc = k - scene * G3;
    const int ix = (int)(loc / ((uint64_t)G * G)), iy = (int)((loc / G) % G), iz = (int)(loc % G);
    const int jx = ix + t / 9 - 1, jy = iy + (t / 3) % 3 - 1, jz = iz + t % 3 - 1;
    int32_t r = -1;
    if (jx >= 0 && jx < G && jy >= 0 && jy < G && jz >= 0 && jz < G)
      r = hash_find(tk, tv, mask, scene * G3 + ((uint64_t)jx * G + jy) * G + jz);
    nbr[i] = r;
  }
}

// coarse level of a stride-2 (k = 2) convolution: the parent cell of a fine voxel and the tap
// (its corner of the 2x2x2 cell) it sits at, t = ((ix & 1) * 2 + (iy & 1)) * 2 + (iz & 1)
__global__ __launch_bounds__(THREADS) void coarse_keys_kernel(const uint64_t *__restrict__ keys, int64_t n, int G,
                                                              uint64_t *__restrict__ pkey, int32_t *__restrict__ tap) {
  const uint64_t G3 = (uint64_t)G * G * G, Gc = (uint64_t)(G >> 1), Gc3 = Gc * Gc * Gc;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
    const uint64_t k = keys[i];
    const uint64_t scene = k / G3, loc = k - scene * G3;
    const uint64_t ix = loc / ((uint64_t)G * G), iy = (loc / G) % G, iz = loc % G;
    pkey[i] = scene * Gc3 + ((ix >> 1) * Gc + (iy >> 1)) * Gc + (iz >> 1);
    tap[i] = (int32_t)(((ix & 1) * 2 + (iy & 1)) * 2 + (iz & 1));
  }
}

__global__ __launch_bounds__(THREADS) void fill_i32_kernel(int32_t *__restrict__ p, int64_t n, int32_t v) {
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) p[i] = v;
}

// one thread per fine voxel f: parent[f], the one-hot row up[f][0..7] and child[parent[f]][tap[f]]
// = f (child cleared to -1 before).  (coarse row, tap) names one fine voxel, so no two threads
// write the same child entry.  A row or tap outside its range (not produced by the kernels
// above) writes nothing but parent[f] = -1 and an empty up row.
__global__ __launch_bounds__(THREADS) void coarse_maps_kernel(const int64_t *__restrict__ crow,
                                                              const int32_t *__restrict__ tap, int64_t nf, int64_t nc,
                                                              int32_t *__restrict__ child, int32_t *__restrict__ parent,
                                                              int32_t *__restrict__ up) {
  for (int64_t f = (int64_t)blockIdx.x * THREADS + threadIdx.x; f < nf; f += (int64_t)gridDim.x * THREADS) {
    const int64_t m = crow[f];
    const int t = tap[f];
    const bool ok = m >= 0 && m < nc && t >= 0 && t < 8;
    parent[f] = ok ? (int32_t)m : -1;
#pragma unroll
    for (int a = 0; a < 8; ++a) up[f * 8 + a] = (ok && a == t) ? (int32_t)m : -1;
    if (ok) child[m * 8 + t] = (int32_t)f;
  }
}

}  // namespace

extern "C" int pcs_voxel_keys(const float *points, const int64_t *offsets, int64_t num_scenes, int64_t T, int32_t grid,
                              float lo_x, float lo_y, float lo_z, float hi_x, float hi_y, float hi_z,
                              const int64_t *voxel_of_point, uint64_t *keys, pcs_stream_t stream) {
  if (!points || !offsets || !voxel_of_point || !keys || num_scenes < 1 || T < 0 || grid < 1 || grid > (1 << 20) ||
      !(hi_x > lo_x && hi_y > lo_y && hi_z > lo_z))
    return pcs_set_einval("pcs_voxel_keys", "bad arguments");
  // keys are scene * G^3 + voxel: they must stay below the hash table's EMPTY sentinel (2^64 - 1)
  if ((double)grid * grid * grid * (double)num_scenes >= 18446744073709551615.0)
    return pcs_set_einval("pcs_voxel_keys", "key overflow (num_scenes * grid^3 >= 2^64 - 1)");
  if (T == 0) return 0;
  const Box b = {{lo_x, lo_y, lo_z}, {hi_x, hi_y, hi_z}};
  hipLaunchKernelGGL(voxel_keys_kernel, dim3(blocks_1d(T)), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     points, offsets, (int)num_scenes, T, (int)grid, b, voxel_of_point, keys);
  PCS_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t pcs_voxel_hash_capacity(int64_t n) {
  if (n < 0 || n > ((int64_t)1 << 31)) return pcs_set_einval("pcs_voxel_hash_capacity", "0 <= n <= 2^31");
  int64_t cap = 64;
  while (cap < 2 * n) cap <<= 1;
  return cap;
}

extern "C" int pcs_voxel_hash_build(const uint64_t *keys, int64_t n, uint64_t *table_keys, int32_t *table_vals,
                                    int64_t capacity, pcs_stream_t stream) {
  if ((!keys && n > 0) || !table_keys || !table_vals || n < 0 || capacity < 2 * n || capacity < 1 ||
      (capacity & (capacity - 1)) != 0)
    return pcs_set_einval("pcs_voxel_hash_build", "bad arguments (capacity: a power of two >= 2 n)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(hash_clear_kernel, dim3(blocks_1d(capacity)), dim3(THREADS), 0, s, table_keys, table_vals, capacity);
  if (n > 0)
    hipLaunchKernelGGL(hash_insert_kernel, dim3(blocks_1d(n)), dim3(THREADS), 0, s, keys, n,
                       reinterpret_cast<unsigned long long *>(table_keys), table_vals, (uint64_t)(capacity - 1));
  PCS_CHECK_LAUNCH();
  return 0;
}

extern "C" int pcs_voxel_hash_find(const uint64_t *table_keys, const int32_t *table_vals, int64_t capacity,
                                   const uint64_t *queries, int64_t nq, int32_t *out, pcs_stream_t stream) {
  if (!table_keys || !table_vals || (!queries && nq > 0) || (!out && nq > 0) || nq < 0 || capacity < 1 ||
      (capacity & (capacity - 1)) != 0)
    return pcs_set_einval("pcs_voxel_hash_find", "bad arguments");
  if (nq == 0) return 0;
  hipLaunchKernelGGL(hash_find_kernel, dim3(blocks_1d(nq)), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     table_keys, table_vals, (uint64_t)(capacity - 1), queries, nq, out);
  PCS_CHECK_LAUNCH();
  return 0;
}

extern "C" int pcs_sparse_neighbors(const uint64_t *table_keys, const int32_t *table_vals, int64_t capacity,
                                    const uint64_t *keys, int64_t n, int32_t grid, int32_t *nbr, pcs_stream_t stream) {
  if (!table_keys || !table_vals || (!keys && n > 0) || (!nbr && n > 0) || n < 0 || grid < 1 || grid > (1 << 20) ||
      capacity < 1 || (capacity & (capacity - 1)) != 0)
    return pcs_set_einval("pcs_sparse_neighbors", "bad arguments");
  if (n == 0) return 0;
  hipLaunchKernelGGL(neighbors_kernel, dim3(blocks_1d(n * 27)), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), table_keys, table_vals, (uint64_t)(capacity - 1), keys, n,
                     (int)grid, nbr);
  PCS_CHECK_LAUNCH();
  return 0;
}

// ---- coarse level of a k = 2, s = 2 convolution (see coarse_keys_kernel)
extern "C" int pcs_sparse_coarse_keys(const uint64_t *keys, int64_t n, int32_t grid, uint64_t *parent_key, int32_t *tap,
                                      pcs_stream_t stream) {
  if (grid < 2 || grid > (1 << 20) || (grid & 1) != 0)
    return pcs_set_einval("pcs_sparse_coarse_keys", "the grid must be even (2 <= grid <= 2^20)");
  if (n < 0 || n > ((int64_t)1 << 31) || (n > 0 && (!keys || !parent_key || !tap)))
    return pcs_set_einval("pcs_sparse_coarse_keys", "keys, parent_key and tap are required (0 <= n <= 2^31)");
  if (n == 0) return 0;
  hipLaunchKernelGGL(coarse_keys_kernel, dim3(blocks_1d(n)), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     keys, n, (int)grid, parent_key, tap);
  PCS_CHECK_LAUNCH();
  return 0;
}

extern "C" int pcs_sparse_coarse_maps(const int64_t *coarse_row, const int32_t *tap, int64_t n_fine, int64_t n_coarse,
                                      int32_t *child, int32_t *parent, int32_t *up, pcs_stream_t stream) {
  if (n_fine < 0 || n_coarse < 0 || n_coarse > n_fine || n_fine >= ((int64_t)1 << 28) ||
      (n_fine > 0 && (!coarse_row || !tap || !parent || !up)) || (n_coarse > 0 && !child))
    return pcs_set_einval("pcs_sparse_coarse_maps",
                          "coarse_row, tap, child, parent and up are required (n_coarse <= n_fine < 2^28)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (n_coarse > 0)
    hipLaunchKernelGGL(fill_i32_kernel, dim3(blocks_1d(n_coarse * 8)), dim3(THREADS), 0, s, child, n_coarse * 8, -1);
  if (n_fine > 0)
    hipLaunchKernelGGL(coarse_maps_kernel, dim3(blocks_1d(n_fine)), dim3(THREADS), 0, s, coarse_row, tap, n_fine,
                       n_coarse, child, parent, up);
  PCS_CHECK_LAUNCH();
  return 0;
}
