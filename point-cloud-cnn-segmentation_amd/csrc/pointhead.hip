// The two per-point ends of the occupied-voxel U-Net (pcs_amd/pointhead.py), fused so that no
// [T, C] array exists in either direction.  Build-defined like the rest of the voxel vocabulary:
// the numpy statement is tests/point_head_refs.py.
//
//   lift     Y[v] = inv_count[v] * sum over v's points of relu(W p + b): the Linear + ReLU of a
//            Cin <= 8 float point is recomputed while the voxel's points are walked; the backward
//            recomputes the gate z > 0 the same way and reduces dW, db over per-block partials
//   lift max Y[v] = relu(max over v's points of W p + b), the first maximum in point order (the
//            statement is tests/segmax_refs.py): the backward re-finds that point per channel and
//            gives it the whole gradient where its z is positive
//   project  Z = X W^T, fp32 [V, K]: trilinear interpolation and the head's Linear are both
//            linear, so the K <= 16 class scores are interpolated instead of the C channels
//   logits   one thread per point: l = b + sum of the eight corner rows of Z, and (with labels) the
//            weighted cross-entropy, its gradient dlogits and the per-block partials of loss and db
//   bwd      dZ[v] = g * the sum of weight * dlogits over v's (point, corner) pairs (fp32 [V, K], the
//            only per-voxel array of the backward), then dX = dZ W and the partials of dW = dZ^T X
//
// All are bandwidth-bound (no MFMA; LDS only for the block reductions) over the lanes-of-E-elements
// row scheme of row_piece.h, with E = 8 for either dtype.  Arithmetic is fp32.  Nothing is added
// atomically, every output row is stored once, and every sum runs in a fixed order (per-thread
// ascending, then a fixed block order, then pcs_reduce_partials over at most 2048 non-empty
// blocks): results are bitwise reproducible.
#include "../../include/pcs_segmax.h"
#include "row_piece.h"

namespace {

using namespace pcs_rows;

constexpr int E = 8;            // channels of a lane
constexpr int MAX_CIN = 8;
constexpr int MAX_K = 16;
constexpr int CORNERS = 8;
constexpr int SEG_UNROLL = 4;   // entries of a segment a lane keeps in flight

// sm[e][slot * lpr + piece] holds one value per lane: column c = piece * 8 + e summed over the row
// slots in slot order
PCS_DEV float column_sum(const float (&sm)[E][THREADS], int c, int lpr, int rpp) {
  const int pc = c / E, e = c - pc * E;
  float s = 0.f;
  for (int j = 0; j < rpp; ++j) s += sm[e][j * lpr + pc];
  return s;
}

// ---- lift
template <int CIN>
PCS_DEV void load_point(const float *__restrict__ P, int64_t ldp, int32_t id, float (&p)[CIN]) {
#pragma unroll
  for (int i = 0; i < CIN; ++i) p[i] = id >= 0 ? P[(int64_t)id * ldp + i] : 0.f;
}

// the pre-activation of one channel, the one expression of the forward and of the backward's gate
template <int CIN>
PCS_DEV float lift_z(const float (&w)[CIN], float b, const float (&p)[CIN]) {
  float z = b;
#pragma unroll
  for (int i = 0; i < CIN; ++i) z = fmaf(w[i], p[i], z);
  return z;
}

template <int CIN>
PCS_DEV void load_lift_weights(const float *__restrict__ W, const float *__restrict__ bias, int c0,
                               float (&w)[E][CIN], float (&b)[E]) {
#pragma unroll
  for (int e = 0; e < E; ++e) {
#pragma unroll
    for (int i = 0; i < CIN; ++i) w[e][i] = W[(int64_t)(c0 + e) * CIN + i];
    b[e] = bias ? bias[c0 + e] : 0.f;
  }
}

template <typename YT, int CIN>
__global__ __launch_bounds__(THREADS) void lift_mean_kernel(const float *__restrict__ P, int64_t ldp,
                                                            const float *__restrict__ W,
                                                            const float *__restrict__ bias,
                                                            const int32_t *__restrict__ order,
                                                            const int64_t *__restrict__ seg_off,
                                                            const float *__restrict__ inv_count, int64_t V, int C,
                                                            YT *__restrict__ Y) {
  int rpp, r0, cc;
  if (!lane_slot(C / E, rpp, r0, cc)) return;
  const int c0 = cc * E;
  float w[E][CIN], b[E];
  load_lift_weights<CIN>(W, bias, c0, w, b);
  for (int64_t v = (int64_t)blockIdx.x * rpp + r0; v < V; v += (int64_t)gridDim.x * rpp) {
    const int64_t j0 = seg_off[v], j1 = seg_off[v + 1];
    float acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
    for (int64_t j = j0; j < j1; j += SEG_UNROLL) {
      int32_t id[SEG_UNROLL];
      float p[SEG_UNROLL][CIN];
#pragma unroll
      for (int u = 0; u < SEG_UNROLL; ++u) id[u] = j + u < j1 ? order[j + u] : -1;
#pragma unroll
      for (int u = 0; u < SEG_UNROLL; ++u) load_point<CIN>(P, ldp, id[u], p[u]);
#pragma unroll
      for (int u = 0; u < SEG_UNROLL; ++u) {
        if (id[u] >= 0) {
#pragma unroll
          for (int e = 0; e < E; ++e) acc[e] += relu(lift_z<CIN>(w[e], b[e], p[u]));
        }
      }
    }
    const float sc = inv_count[v];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] *= sc;
    store_piece<YT, E>(Y + v * C + c0, acc);
  }
}

// part_w [blocks][C][CIN], part_b [blocks][C] (NULL: no db): each block's sums over its rows
template <typename DT, int CIN>
__global__ __launch_bounds__(THREADS) void lift_bwd_kernel(const DT *__restrict__ dV, const float *__restrict__ P,
                                                           int64_t ldp, const float *__restrict__ W,
                                                           const float *__restrict__ bias,
                                                           const int32_t *__restrict__ order,
                                                           const int64_t *__restrict__ seg_off,
                                                           const float *__restrict__ inv_count, int64_t V, int C,
                                                           int64_t rpb, float *__restrict__ part_w,
                                                           float *__restrict__ part_b) {
  __shared__ float sm[E][THREADS];
  int rpp, r0, cc;
  const int lpr = C / E, tid = threadIdx.x;
  const bool active = lane_slot(lpr, rpp, r0, cc);
  const int64_t lo = (int64_t)blockIdx.x * rpb, hi = pcs_min64(lo + rpb, V);
  float aw[E][CIN], ab[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    ab[e] = 0.f;
#pragma unroll
    for (int i = 0; i < CIN; ++i) aw[e][i] = 0.f;
  }
  if (active) {
    const int c0 = cc * E;
    float w[E][CIN], b[E];
    load_lift_weights<CIN>(W, bias, c0, w, b);
    for (int64_t v = lo + r0; v < hi; v += rpp) {
      Raw<DT, E> rd;
      raw_load<DT, E>(rd, dV + v * C + c0, true);
      const int64_t j0 = seg_off[v], j1 = seg_off[v + 1];
      const float sc = inv_count[v];
      float d[E];
      raw_unpack<DT, E>(rd, d);
#pragma unroll
      for (int e = 0; e < E; ++e) d[e] *= sc;
      for (int64_t j = j0; j < j1; j += SEG_UNROLL) {
        int32_t id[SEG_UNROLL];
        float p[SEG_UNROLL][CIN];
#pragma unroll
        for (int u = 0; u < SEG_UNROLL; ++u) id[u] = j + u < j1 ? order[j + u] : -1;
#pragma unroll
        for (int u = 0; u < SEG_UNROLL; ++u) load_point<CIN>(P, ldp, id[u], p[u]);
#pragma unroll
        for (int u = 0; u < SEG_UNROLL; ++u) {
          if (id[u] >= 0) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
              const float g = lift_z<CIN>(w[e], b[e], p[u]) > 0.f ? d[e] : 0.f;
              ab[e] += g;
#pragma unroll
              for (int i = 0; i < CIN; ++i) aw[e][i] = fmaf(g, p[u][i], aw[e][i]);
            }
          }
        }
      }
    }
  }
  // one pass per input column (and one for the bias): a thread per channel sums the row slots
#pragma unroll
  for (int q = 0; q <= CIN; ++q) {
    if (q < CIN || part_b) {   // uniform
#pragma unroll
      for (int e = 0; e < E; ++e) sm[e][tid] = q < CIN ? aw[e][q < CIN ? q : 0] : ab[e];
      __syncthreads();
      for (int c = tid; c < C; c += THREADS) {
        const float s = column_sum(sm, c, lpr, rpp);
        if (q < CIN) part_w[((int64_t)blockIdx.x * C + c) * CIN + q] = s;
        else part_b[(int64_t)blockIdx.x * C + c] = s;
      }
      __syncthreads();
    }
  }
}

// ---- lift, max form: Y[v] = relu(max over v's points of z), the first maximum in point order
// (common.h's pool_max_step over ascending entries; max relu = relu max)
// (The mean kernels above keep their loops written out: routed through load_entries or a shared
// epilogue their device code changes, register allocation at least; tools/asm_equal.py shows it.)
// SEG_UNROLL entries of a segment from j on: the point ids (-1 past the end j1) and their points
template <int CIN>
PCS_DEV void load_entries(const float *__restrict__ P, int64_t ldp, const int32_t *__restrict__ order, int64_t j,
                          int64_t j1, int32_t (&id)[SEG_UNROLL], float (&p)[SEG_UNROLL][CIN]) {
#pragma unroll
  for (int u = 0; u < SEG_UNROLL; ++u) id[u] = j + u < j1 ? order[j + u] : -1;
#pragma unroll
  for (int u = 0; u < SEG_UNROLL; ++u) load_point<CIN>(P, ldp, id[u], p[u]);
}

// the running pick over these entries: pick[e] is the point of channel e's largest z so far,
// PCS_POOL_NONE until the first present point, which always makes the pick
template <int CIN>
PCS_DEV void lift_pick_step(const float (&w)[E][CIN], const float (&b)[E], const int32_t (&id)[SEG_UNROLL],
                            const float (&p)[SEG_UNROLL][CIN], float (&best)[E], int (&pick)[E]) {
#pragma unroll
  for (int u = 0; u < SEG_UNROLL; ++u) {
    if (id[u] >= 0) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float z = lift_z<CIN>(w[e], b[e], p[u]);
        const bool wins = pool_max_step(z, best[e], pick[e]);
        best[e] = wins ? z : best[e];
        pick[e] = wins ? id[u] : pick[e];
      }
    }
  }
}

// d[e] * (1, p) of the picked point into the sums
template <int CIN>
PCS_DEV void lift_pick_grad(const int (&pick)[E], const float (&d)[E], const int32_t (&id)[SEG_UNROLL],
                            const float (&p)[SEG_UNROLL][CIN], float (&aw)[E][CIN], float (&ab)[E]) {
#pragma unroll
  for (int u = 0; u < SEG_UNROLL; ++u) {
    if (id[u] >= 0) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float g = pick[e] == id[u] ? d[e] : 0.f;
        ab[e] += g;
#pragma unroll
        for (int i = 0; i < CIN; ++i) aw[e][i] = fmaf(g, p[u][i], aw[e][i]);
      }
    }
  }
}

template <typename YT, int CIN>
__global__ __launch_bounds__(THREADS) void lift_max_kernel(const float *__restrict__ P, int64_t ldp,
                                                           const float *__restrict__ W,
                                                           const float *__restrict__ bias,
                                                           const int32_t *__restrict__ order,
                                                           const int64_t *__restrict__ seg_off, int64_t V, int C,
                                                           YT *__restrict__ Y) {
  int rpp, r0, cc;
  if (!lane_slot(C / E, rpp, r0, cc)) return;
  const int c0 = cc * E;
  float w[E][CIN], b[E];
  load_lift_weights<CIN>(W, bias, c0, w, b);
  for (int64_t v = (int64_t)blockIdx.x * rpp + r0; v < V; v += (int64_t)gridDim.x * rpp) {
    const int64_t j0 = seg_off[v], j1 = seg_off[v + 1];
    float best[E];
    int seen = PCS_POOL_NONE;   // until the first present point, which always makes the pick
#pragma unroll
    for (int e = 0; e < E; ++e) best[e] = 0.f;
    for (int64_t j = j0; j < j1; j += SEG_UNROLL) {
      int32_t id[SEG_UNROLL];
      float p[SEG_UNROLL][CIN];
      load_entries<CIN>(P, ldp, order, j, j1, id, p);
#pragma unroll
      for (int u = 0; u < SEG_UNROLL; ++u) {
        if (id[u] >= 0) {
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const float z = lift_z<CIN>(w[e], b[e], p[u]);
            best[e] = pool_max_step(z, best[e], seen) ? z : best[e];
          }
          seen = 0;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) best[e] = relu(best[e]);   // (a voxel without points: relu(0))
    store_piece<YT, E>(Y + v * C + c0, best);
  }
}

// The gradient goes to the one point the forward picked, where its z is positive: a first walk of
// the segment re-finds the pick per channel, a second one adds dV[v][c] * (1, p_pick) into the sums.
// The first SEG_UNROLL entries stay in registers between the walks, so a voxel of at most that many
// points (nearly all of them) loads its points once; a longer one reloads the rest from cache.
// part_w, part_b as lift_bwd_kernel's.
template <typename DT, int CIN>
__global__ __launch_bounds__(THREADS) void lift_max_bwd_kernel(const DT *__restrict__ dV, const float *__restrict__ P,
                                                               int64_t ldp, const float *__restrict__ W,
                                                               const float *__restrict__ bias,
                                                               const int32_t *__restrict__ order,
                                                               const int64_t *__restrict__ seg_off, int64_t V, int C,
                                                               int64_t rpb, float *__restrict__ part_w,
                                                               float *__restrict__ part_b) {
  __shared__ float sm[E][THREADS];
  int rpp, r0, cc;
  const int lpr = C / E, tid = threadIdx.x;
  const bool active = lane_slot(lpr, rpp, r0, cc);
  const int64_t lo = (int64_t)blockIdx.x * rpb, hi = pcs_min64(lo + rpb, V);
  float aw[E][CIN], ab[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    ab[e] = 0.f;
#pragma unroll
    for (int i = 0; i < CIN; ++i) aw[e][i] = 0.f;
  }
  if (active) {
    const int c0 = cc * E;
    float w[E][CIN], b[E];
    load_lift_weights<CIN>(W, bias, c0, w, b);
    for (int64_t v = lo + r0; v < hi; v += rpp) {
      Raw<DT, E> rd;
      raw_load<DT, E>(rd, dV + v * C + c0, true);
      const int64_t j0 = seg_off[v], j1 = seg_off[v + 1];
      float best[E];
      int pick[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        best[e] = 0.f;
        pick[e] = PCS_POOL_NONE;
      }
      int32_t id0[SEG_UNROLL], id[SEG_UNROLL];
      float p0[SEG_UNROLL][CIN], p[SEG_UNROLL][CIN];
      load_entries<CIN>(P, ldp, order, j0, j1, id0, p0);
      lift_pick_step<CIN>(w, b, id0, p0, best, pick);
      for (int64_t j = j0 + SEG_UNROLL; j < j1; j += SEG_UNROLL) {
        load_entries<CIN>(P, ldp, order, j, j1, id, p);
        lift_pick_step<CIN>(w, b, id, p, best, pick);
      }
      float d[E];
      raw_unpack<DT, E>(rd, d);
#pragma unroll
      for (int e = 0; e < E; ++e) pick[e] = best[e] > 0.f ? pick[e] : PCS_POOL_NONE;   // the gate (no point id is NONE)
      lift_pick_grad<CIN>(pick, d, id0, p0, aw, ab);
      for (int64_t j = j0 + SEG_UNROLL; j < j1; j += SEG_UNROLL) {
        load_entries<CIN>(P, ldp, order, j, j1, id, p);
        lift_pick_grad<CIN>(pick, d, id, p, aw, ab);
      }
    }
  }
  // one pass per input column (and one for the bias): a thread per channel sums the row slots
#pragma unroll
  for (int q = 0; q <= CIN; ++q) {
    if (q < CIN || part_b) {   // uniform
#pragma unroll
      for (int e = 0; e < E; ++e) sm[e][tid] = q < CIN ? aw[e][q < CIN ? q : 0] : ab[e];
      __syncthreads();
      for (int c = tid; c < C; c += THREADS) {
        const float s = column_sum(sm, c, lpr, rpp);
        if (q < CIN) part_w[((int64_t)blockIdx.x * C + c) * CIN + q] = s;
        else part_b[(int64_t)blockIdx.x * C + c] = s;
      }
      __syncthreads();
    }
  }
}

// ---- head
// rows a lane keeps in flight: fewer for more classes (registers, LDS)
template <int KT>
struct HeadUnroll {
  static constexpr int U = KT <= 4 ? 4 : (KT == 8 ? 2 : 1);
};

// w[k][e] = W[k][c0 + e], zero rows for k >= K
template <int KT>
PCS_DEV void load_head_weights(const float *__restrict__ W, int K, int C, int c0, float (&w)[KT][E]) {
#pragma unroll
  for (int k = 0; k < KT; ++k) {
#pragma unroll
    for (int e = 0; e < E; ++e) w[k][e] = k < K ? W[(int64_t)k * C + c0 + e] : 0.f;
  }
}

// Z[v][k] = sum_c X[v][c] W[k][c]: a lane's 8 channels, then the lanes of the row in lane order
template <typename XT, int KT>
__global__ __launch_bounds__(THREADS) void head_project_kernel(const XT *__restrict__ X, int64_t V, int C,
                                                               const float *__restrict__ W, int K,
                                                               float *__restrict__ Z) {
  constexpr int U = HeadUnroll<KT>::U;
  constexpr int LD = KT + 1;   // odd stride: the K sums of a lane sit in consecutive banks
  __shared__ float sm[U][THREADS * LD];
  int rpp, r0, cc;
  const int lpr = C / E, tid = threadIdx.x;
  const bool active = lane_slot(lpr, rpp, r0, cc);
  const int c0 = cc * E;
  float w[KT][E];
  load_head_weights<KT>(W, active ? K : 0, C, c0, w);
  const int64_t step = (int64_t)rpp * U;
  const int per_u = rpp * KT;
  for (int64_t base = (int64_t)blockIdx.x * step; base < V; base += (int64_t)gridDim.x * step) {
    Raw<XT, E> rx[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = base + (int64_t)u * rpp + r0;
      raw_load<XT, E>(rx[u], X + row * C + c0, active && row < V);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float x[E];
      raw_unpack<XT, E>(rx[u], x);
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e) s = fmaf(x[e], w[k][e], s);
        sm[u][tid * LD + k] = s;
      }
    }
    __syncthreads();
    for (int t = tid; t < U * per_u; t += THREADS) {
      const int u = t / per_u, rem = t - u * per_u;
      const int r = rem / KT, k = rem - r * KT;
      const int64_t row = base + (int64_t)u * rpp + r;
      if (row < V && k < K) {
        float s = 0.f;
        for (int c = 0; c < lpr; ++c) s += sm[u][(r * lpr + c) * LD + k];
        Z[row * K + k] = s;
      }
    }
    __syncthreads();
  }
}

// one thread per point; CE: the loss, its gradient and the per-block partials
template <int KT, bool CE>
__global__ __launch_bounds__(THREADS) void head_logits_kernel(
    const float *__restrict__ Z, const int32_t *__restrict__ corner, const float *__restrict__ weight, int64_t T, int K,
    const float *__restrict__ bias, const int64_t *__restrict__ labels, const float *__restrict__ class_weight,
    const float *__restrict__ inv_wsum, float *__restrict__ logits, float *__restrict__ dlogits, int64_t ppb,
    float *__restrict__ part_loss, float *__restrict__ part_db) {
  __shared__ float sm[THREADS / 64][KT + 1];
  const int tid = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * ppb, hi = pcs_min64(lo + ppb, T);
  float b[KT], sdb[KT], sl = 0.f;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    b[k] = (bias && k < K) ? bias[k] : 0.f;
    sdb[k] = 0.f;
  }
  const float inv = CE ? *inv_wsum : 0.f;
  for (int64_t p = lo + tid; p < hi; p += THREADS) {
    int32_t id[CORNERS];
    float wk[CORNERS];
#pragma unroll
    for (int h = 0; h < CORNERS / 4; ++h) {
      const int4 ci = reinterpret_cast<const int4 *>(corner + p * CORNERS)[h];
      const float4 cw = reinterpret_cast<const float4 *>(weight + p * CORNERS)[h];
      id[4 * h] = ci.x; id[4 * h + 1] = ci.y; id[4 * h + 2] = ci.z; id[4 * h + 3] = ci.w;
      wk[4 * h] = cw.x; wk[4 * h + 1] = cw.y; wk[4 * h + 2] = cw.z; wk[4 * h + 3] = cw.w;
    }
    float z[CORNERS][KT];
#pragma unroll
    for (int j = 0; j < CORNERS; ++j) {
#pragma unroll
      for (int k = 0; k < KT; ++k) z[j][k] = (id[j] >= 0 && k < K) ? Z[(int64_t)id[j] * K + k] : 0.f;
    }
    float l[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) l[k] = b[k];
#pragma unroll
    for (int j = 0; j < CORNERS; ++j) {
      if (id[j] >= 0) {
#pragma unroll
        for (int k = 0; k < KT; ++k) l[k] = fmaf(wk[j], z[j][k], l[k]);
      }
    }
    if (logits) {
#pragma unroll
      for (int k = 0; k < KT; ++k)
        if (k < K) logits[p * K + k] = l[k];
    }
    if (CE) {
      const int64_t y = labels[p];
      const bool valid = y >= 0 && y < K;   // anything else (-1 = ignored) contributes nothing
      float m = l[0];
#pragma unroll
      for (int k = 1; k < KT; ++k)
        if (k < K) m = fmaxf(m, l[k]);
      float ex[KT], se = 0.f, ly = 0.f;
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        ex[k] = k < K ? expf(l[k] - m) : 0.f;
        se += ex[k];
        ly = (int64_t)k == y ? l[k] : ly;
      }
      const float cwy = valid ? class_weight[y] : 0.f;
      if (valid) sl += cwy * (logf(se) + m - ly);
      const float gs = cwy * inv, rs = 1.f / se;
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        const float d = valid ? gs * (ex[k] * rs - ((int64_t)k == y ? 1.f : 0.f)) : 0.f;
        if (k < K) {
          if (dlogits) dlogits[p * K + k] = d;
          sdb[k] += d;
        }
      }
    }
  }
  if (CE) {
    const int wave = tid / 64, lane = tid % 64;
    sl = wave_sum(sl);
#pragma unroll
    for (int k = 0; k < KT; ++k) sdb[k] = wave_sum(sdb[k]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < KT; ++k) sm[wave][k] = sdb[k];
      sm[wave][KT] = sl;
    }
    __syncthreads();
    if (tid <= KT) {
      float s = 0.f;
      for (int wv = 0; wv < THREADS / 64; ++wv) s += sm[wv][tid];
      // without a valid label pcs_ce_weight_sum reports inv_wsum = 0: NaN, the 0 / 0 torch reports
      if (tid == KT) part_loss[blockIdx.x] = inv > 0.f ? inv * s : __builtin_nanf("");
      else if (tid < K && part_db) part_db[(int64_t)blockIdx.x * K + tid] = s;
    }
  }
}

// one thread per voxel: dZ[v][k] = g * sum_j pair_weight[j] * dlogits[pair_point[j]][k], ascending j
template <int KT>
__global__ __launch_bounds__(THREADS) void head_dz_kernel(const float *__restrict__ dlogits,
                                                          const int32_t *__restrict__ pair_point,
                                                          const float *__restrict__ pair_weight,
                                                          const int64_t *__restrict__ seg_off, int64_t V, int K,
                                                          const float *__restrict__ gscale, float *__restrict__ dZ) {
  const float g = gscale ? *gscale : 1.f;
  for (int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * THREADS) {
    const int64_t j0 = seg_off[v], j1 = seg_off[v + 1];
    float a[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) a[k] = 0.f;
    for (int64_t j = j0; j < j1; j += SEG_UNROLL) {
      int32_t id[SEG_UNROLL];
      float wj[SEG_UNROLL], d[SEG_UNROLL][KT];
#pragma unroll
      for (int u = 0; u < SEG_UNROLL; ++u) {
        const bool in = j + u < j1;
        id[u] = in ? pair_point[j + u] : -1;
        wj[u] = in ? pair_weight[j + u] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < SEG_UNROLL; ++u) {
#pragma unroll
        for (int k = 0; k < KT; ++k) d[u][k] = (id[u] >= 0 && k < K) ? dlogits[(int64_t)id[u] * K + k] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < SEG_UNROLL; ++u) {
        if (id[u] >= 0) {
#pragma unroll
          for (int k = 0; k < KT; ++k) a[k] = fmaf(wj[u], d[u][k], a[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < KT; ++k)
      if (k < K) dZ[v * K + k] = g * a[k];
  }
}

// dX[v] = dZ[v] W (NULL: skipped) and part [blocks][K][C] = each block's sum of dZ[v]^T X[v] (NULL:
// skipped)
template <typename XT, int KT>
__global__ __launch_bounds__(THREADS) void head_bwd_kernel(const float *__restrict__ dZ, const XT *__restrict__ X,
                                                           int64_t V, int C, const float *__restrict__ W, int K,
                                                           int64_t rpb, XT *__restrict__ dX,
                                                           float *__restrict__ part) {
  constexpr int U = HeadUnroll<KT>::U;
  __shared__ float sm[E][THREADS];
  int rpp, r0, cc;
  const int lpr = C / E, tid = threadIdx.x;
  const bool active = lane_slot(lpr, rpp, r0, cc);
  const int64_t lo = (int64_t)blockIdx.x * rpb, hi = pcs_min64(lo + rpb, V);
  float acc[KT][E];
#pragma unroll
  for (int k = 0; k < KT; ++k) {
#pragma unroll
    for (int e = 0; e < E; ++e) acc[k][e] = 0.f;
  }
  if (active) {
    const int c0 = cc * E;
    float w[KT][E];
    load_head_weights<KT>(W, dX ? K : 0, C, c0, w);
    for (int64_t v = lo + r0; v < hi; v += (int64_t)rpp * U) {
      Raw<XT, E> rx[U];
      float dz[U][KT];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t row = v + (int64_t)u * rpp;
        const bool in = row < hi;
        raw_load<XT, E>(rx[u], X + row * C + c0, in && part != nullptr);
#pragma unroll
        for (int k = 0; k < KT; ++k) dz[u][k] = (in && k < K) ? dZ[row * K + k] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t row = v + (int64_t)u * rpp;
        if (row < hi) {
          if (part) {
            float x[E];
            raw_unpack<XT, E>(rx[u], x);
#pragma unroll
            for (int k = 0; k < KT; ++k) {
#pragma unroll
              for (int e = 0; e < E; ++e) acc[k][e] = fmaf(dz[u][k], x[e], acc[k][e]);
            }
          }
          if (dX) {
            float o[E];
#pragma unroll
            for (int e = 0; e < E; ++e) o[e] = 0.f;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
#pragma unroll
              for (int e = 0; e < E; ++e) o[e] = fmaf(dz[u][k], w[k][e], o[e]);
            }
            store_piece<XT, E>(dX + row * C + c0, o);
          }
        }
      }
    }
  }
  if (!part) return;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    if (k < K) {   // uniform
#pragma unroll
      for (int e = 0; e < E; ++e) sm[e][tid] = acc[k][e];
      __syncthreads();
      for (int c = tid; c < C; c += THREADS) part[((int64_t)blockIdx.x * K + k) * C + c] = column_sum(sm, c, lpr, rpp);
      __syncthreads();
    }
  }
}

// ---- host side
int stream_blocks(int64_t rows, int64_t rows_per_block, int64_t cap) {
  const int64_t b = (rows + rows_per_block - 1) / rows_per_block;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

bool bad_channels(int32_t C) { return C < E || C % E != 0 || C > MAX_C; }
bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }
int64_t round4(int64_t n) { return (n + 3) / 4 * 4; }

const char *const MSG_C = "C % 8 == 0, 8 <= C <= 1024 required";
const char *const MSG_CIN = "1 <= Cin <= 8 required";
const char *const MSG_K = "1 <= K <= 16 required";
const char *const MSG_DTYPE = "unknown dtype (PCS_F32 | PCS_BF16)";
const char *const MSG_WS = "workspace NULL, not 16-byte aligned or smaller than the workspace query's size";

int64_t lift_bwd_bytes(int64_t V, int32_t C, int32_t Cin) {
  return (int64_t)reduction_blocks(V, ROW_TILE).n * ((int64_t)C * Cin + C) * (int64_t)sizeof(float);
}

int64_t head_logits_floats(int64_t T, int32_t K) { return (int64_t)reduction_blocks(T, THREADS).n * (K + 1); }
int64_t head_bwd_floats(int64_t V, int32_t C, int32_t K) {
  return round4(V * K) + (int64_t)reduction_blocks(V, ROW_TILE).n * K * C;
}

#define PCS_PH_CIN(Cin, CALL)                                           \
  switch (Cin) {                                                        \
    case 1: CALL(1); break;                                             \
    case 2: CALL(2); break;                                             \
    case 3: CALL(3); break;                                             \
    case 4: CALL(4); break;                                             \
    case 5: CALL(5); break;                                             \
    case 6: CALL(6); break;                                             \
    case 7: CALL(7); break;                                             \
    default: CALL(8); break;                                            \
  }

// K padded to a power of two at compile time
#define PCS_PH_K(K, CALL)                                               \
  do {                                                                  \
    if (K <= 1) { CALL(1); }                                            \
    else if (K <= 2) { CALL(2); }                                       \
    else if (K <= 4) { CALL(4); }                                       \
    else if (K <= 8) { CALL(8); }                                       \
    else { CALL(16); }                                                  \
  } while (0)

}  // namespace

extern "C" int pcs_point_lift_mean(const float *P, int64_t ldp, int32_t Cin, const float *W, const float *bias,
                                   const int32_t *order, const int64_t *seg_off, const float *inv_count, int64_t V,
                                   int32_t C, void *Y, int32_t ydtype, pcs_stream_t stream) {
  const char *fn = "pcs_point_lift_mean";
  if (V < 0) return pcs_set_einval(fn, "V >= 0 required");
  if (Cin < 1 || Cin > MAX_CIN) return pcs_set_einval(fn, MSG_CIN);
  if (ldp < Cin) return pcs_set_einval(fn, "ldp >= Cin required");
  if (bad_channels(C)) return pcs_set_einval(fn, MSG_C);
  if (!known(ydtype)) return pcs_set_einval(fn, MSG_DTYPE);
  if (V == 0) return 0;
  if (!P || !W || !order || !seg_off || !inv_count || !Y) return pcs_set_einval(fn, "NULL pointer");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(stream_blocks(V, THREADS / (C / E), 1 << 20)), block(THREADS);
#define PCS_PH_CALL(CIN)                                                                                              \
  do {                                                                                                                \
    if (ydtype == PCS_BF16)                                                                                           \
      hipLaunchKernelGGL((lift_mean_kernel<bf16_t, CIN>), grid, block, 0, s, P, ldp, W, bias, order, seg_off,          \
                         inv_count, V, (int)C, static_cast<bf16_t *>(Y));                                             \
    else                                                                                                              \
      hipLaunchKernelGGL((lift_mean_kernel<float, CIN>), grid, block, 0, s, P, ldp, W, bias, order, seg_off, inv_count, \
                         V, (int)C, static_cast<float *>(Y));                                                         \
  } while (0)
  PCS_PH_CIN(Cin, PCS_PH_CALL)
#undef PCS_PH_CALL
  PCS_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t pcs_point_lift_bwd_workspace(int64_t V, int32_t C, int32_t Cin) {
  const char *fn = "pcs_point_lift_bwd_workspace";
  if (V < 0) return pcs_set_einval(fn, "V >= 0 required");
  if (Cin < 1 || Cin > MAX_CIN) return pcs_set_einval(fn, MSG_CIN);
  if (bad_channels(C)) return pcs_set_einval(fn, MSG_C);
  return lift_bwd_bytes(V, C, Cin);
}

extern "C" int pcs_point_lift_mean_bwd(const void *dV, int32_t dvdtype, const float *P, int64_t ldp, int32_t Cin,
                                       const float *W, const float *bias, const int32_t *order, const int64_t *seg_off,
                                       const float *inv_count, int64_t V, int32_t C, void *workspace,
                                       int64_t workspace_bytes, float *dW, float *db, pcs_stream_t stream) {
  const char *fn = "pcs_point_lift_mean_bwd";
  if (V < 0) return pcs_set_einval(fn, "V >= 0 required");
  if (Cin < 1 || Cin > MAX_CIN) return pcs_set_einval(fn, MSG_CIN);
  if (ldp < Cin) return pcs_set_einval(fn, "ldp >= Cin required");
  if (bad_channels(C)) return pcs_set_einval(fn, MSG_C);
  if (!known(dvdtype)) return pcs_set_einval(fn, MSG_DTYPE);
  if (V == 0) return 0;
  if (!dV || !P || !W || !order || !seg_off || !inv_count || !dW) return pcs_set_einval(fn, "NULL pointer");
  if (!workspace || misaligned(workspace) || workspace_bytes < lift_bwd_bytes(V, C, Cin))
    return pcs_set_einval(fn, MSG_WS);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const Blocks b = reduction_blocks(V, ROW_TILE);
  float *part_w = static_cast<float *>(workspace);
  float *part_b = part_w + (int64_t)b.n * C * Cin;
  float *pb = db ? part_b : nullptr;
  const dim3 grid(b.n), block(THREADS);
#define PCS_PH_CALL(CIN)                                                                                            \
  do {                                                                                                              \
    if (dvdtype == PCS_BF16)                                                                                        \
      hipLaunchKernelGGL((lift_bwd_kernel<bf16_t, CIN>), grid, block, 0, s, static_cast<const bf16_t *>(dV), P, ldp, \
                         W, bias, order, seg_off, inv_count, V, (int)C, b.per, part_w, pb);                         \
    else                                                                                                            \
      hipLaunchKernelGGL((lift_bwd_kernel<float, CIN>), grid, block, 0, s, static_cast<const float *>(dV), P, ldp, W, \
                         bias, order, seg_off, inv_count, V, (int)C, b.per, part_w, pb);                            \
  } while (0)
  PCS_PH_CIN(Cin, PCS_PH_CALL)
#undef PCS_PH_CALL
  PCS_CHECK_LAUNCH();
  const int64_t nw = (int64_t)C * Cin;
  if (int rc = pcs_reduce_partials(part_w, b.n, nw, 1.f, dW, nw, nw, stream)) return rc;
  if (db)
    if (int rc = pcs_reduce_partials(part_b, b.n, C, 1.f, db, C, C, stream)) return rc;
  return 0;
}

extern "C" int pcs_point_lift_max(const float *P, int64_t ldp, int32_t Cin, const float *W, const float *bias,
                                  const int32_t *order, const int64_t *seg_off, int64_t V, int32_t C, void *Y,
                                  int32_t ydtype, pcs_stream_t stream) {
  const char *fn = "pcs_point_lift_max";
  if (V < 0) return pcs_set_einval(fn, "V >= 0 required");
  if (Cin < 1 || Cin > MAX_CIN) return pcs_set_einval(fn, MSG_CIN);
  if (ldp < Cin) return pcs_set_einval(fn, "ldp >= Cin required");
  if (bad_channels(C)) return pcs_set_einval(fn, MSG_C);
  if (!known(ydtype)) return pcs_set_einval(fn, MSG_DTYPE);
  if (V == 0) return 0;
  if (!P || !W || !order || !seg_off || !Y) return pcs_set_einval(fn, "NULL pointer");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(stream_blocks(V, THREADS / (C / E), 1 << 20)), block(THREADS);
#define PCS_PH_CALL(CIN)                                                                                              \
  do {                                                                                                                \
    if (ydtype == PCS_BF16)                                                                                           \
      hipLaunchKernelGGL((lift_max_kernel<bf16_t, CIN>), grid, block, 0, s, P, ldp, W, bias, order, seg_off, V,        \
                         (int)C, static_cast<bf16_t *>(Y));                                                           \
    else                                                                                                              \
      hipLaunchKernelGGL((lift_max_kernel<float, CIN>), grid, block, 0, s, P, ldp, W, bias, order, seg_off, V, (int)C, \
                         static_cast<float *>(Y));                                                                    \
  } while (0)
  PCS_PH_CIN(Cin, PCS_PH_CALL)
#undef PCS_PH_CALL
  PCS_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t pcs_point_lift_max_bwd_workspace(int64_t V, int32_t C, int32_t Cin) {
  const char *fn = "pcs_point_lift_max_bwd_workspace";
  if (V < 0) return pcs_set_einval(fn, "V >= 0 required");
  if (Cin < 1 || Cin > MAX_CIN) return pcs_set_einval(fn, MSG_CIN);
  if (bad_channels(C)) return pcs_set_einval(fn, MSG_C);
  return lift_bwd_bytes(V, C, Cin);
}

extern "C" int pcs_point_lift_max_bwd(const void *dV, int32_t dvdtype, const float *P, int64_t ldp, int32_t Cin,
                                      const float *W, const float *bias, const int32_t *order, const int64_t *seg_off,
                                      int64_t V, int32_t C, void *workspace, int64_t workspace_bytes, float *dW,
                                      float *db, pcs_stream_t stream) {
  const char *fn = "pcs_point_lift_max_bwd";
  if (V < 0) return pcs_set_einval(fn, "V >= 0 required");
  if (Cin < 1 || Cin > MAX_CIN) return pcs_set_einval(fn, MSG_CIN);
  if (ldp < Cin) return pcs_set_einval(fn, "ldp >= Cin required");
  if (bad_channels(C)) return pcs_set_einval(fn, MSG_C);
  if (!known(dvdtype)) return pcs_set_einval(fn, MSG_DTYPE);
  if (V == 0) return 0;
  if (!dV || !P || !W || !order || !seg_off || !dW) return pcs_set_einval(fn, "NULL pointer");
  if (!workspace || misaligned(workspace) || workspace_bytes < lift_bwd_bytes(V, C, Cin))
    return pcs_set_einval(fn, MSG_WS);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const Blocks b = reduction_blocks(V, ROW_TILE);
  float *part_w = static_cast<float *>(workspace);
  float *part_b = part_w + (int64_t)b.n * C * Cin;
  float *pb = db ? part_b : nullptr;
  const dim3 grid(b.n), block(THREADS);
#define PCS_PH_CALL(CIN)                                                                                             \
  do {                                                                                                               \
    if (dvdtype == PCS_BF16)                                                                                         \
      hipLaunchKernelGGL((lift_max_bwd_kernel<bf16_t, CIN>), grid, block, 0, s, static_cast<const bf16_t *>(dV), P,   \
                         ldp, W, bias, order, seg_off, V, (int)C, b.per, part_w, pb);                                \
    else                                                                                                             \
      hipLaunchKernelGGL((lift_max_bwd_kernel<float, CIN>), grid, block, 0, s, static_cast<const float *>(dV), P, ldp, \
                         W, bias, order, seg_off, V, (int)C, b.per, part_w, pb);                                     \
  } while (0)
  PCS_PH_CIN(Cin, PCS_PH_CALL)
#undef PCS_PH_CALL
  PCS_CHECK_LAUNCH();
  const int64_t nw = (int64_t)C * Cin;
  if (int rc = pcs_reduce_partials(part_w, b.n, nw, 1.f, dW, nw, nw, stream)) return rc;
  if (db)
    if (int rc = pcs_reduce_partials(part_b, b.n, C, 1.f, db, C, C, stream)) return rc;
  return 0;
}

extern "C" int pcs_point_head_project(const void *X, int32_t xdtype, int64_t V, int32_t C, const float *W, int32_t K,
                                      float *Z, pcs_stream_t stream) {
  const char *fn = "pcs_point_head_project";
  if (V < 0) return pcs_set_einval(fn, "V >= 0 required");
  if (K < 1 || K > MAX_K) return pcs_set_einval(fn, MSG_K);
  if (bad_channels(C)) return pcs_set_einval(fn, MSG_C);
  if (!known(xdtype)) return pcs_set_einval(fn, MSG_DTYPE);
  if (V == 0) return 0;
  if (!X || !W || !Z) return pcs_set_einval(fn, "NULL pointer");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 block(THREADS);
  const int rpp = THREADS / (C / E);
#define PCS_PH_CALL(KT)                                                                                            \
  do {                                                                                                             \
    const dim3 grid(stream_blocks(V, (int64_t)rpp * HeadUnroll<KT>::U, 1 << 16));                                  \
    if (xdtype == PCS_BF16)                                                                                        \
      hipLaunchKernelGGL((head_project_kernel<bf16_t, KT>), grid, block, 0, s, static_cast<const bf16_t *>(X), V,   \
                         (int)C, W, (int)K, Z);                                                                    \
    else                                                                                                           \
      hipLaunchKernelGGL((head_project_kernel<float, KT>), grid, block, 0, s, static_cast<const float *>(X), V,     \
                         (int)C, W, (int)K, Z);                                                                    \
  } while (0)
  PCS_PH_K(K, PCS_PH_CALL);
#undef PCS_PH_CALL
  PCS_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t pcs_point_head_workspace(int64_t T, int64_t V, int32_t C, int32_t K) {
  const char *fn = "pcs_point_head_workspace";
  if (T < 0 || V < 0) return pcs_set_einval(fn, "T >= 0 and V >= 0 required");
  if (K < 1 || K > MAX_K) return pcs_set_einval(fn, MSG_K);
  if (bad_channels(C)) return pcs_set_einval(fn, MSG_C);
  return pcs_max64(head_logits_floats(T, K), head_bwd_floats(V, C, K)) * (int64_t)sizeof(float);
}

extern "C" int pcs_point_head_logits(const float *Z, const int32_t *corner, const float *weight, int64_t T, int32_t K,
                                     const float *bias, const int64_t *labels, const float *class_weight,
                                     const float *inv_wsum, float *logits, float *dlogits, void *workspace,
                                     int64_t workspace_bytes, float *loss, float *db, pcs_stream_t stream) {
  const char *fn = "pcs_point_head_logits";
  if (T < 0) return pcs_set_einval(fn, "T >= 0 required");
  if (K < 1 || K > MAX_K) return pcs_set_einval(fn, MSG_K);
  if (T == 0) return 0;
  if (!Z || !corner || !weight) return pcs_set_einval(fn, "NULL pointer");
  if (misaligned(corner) || misaligned(weight)) return pcs_set_einval(fn, "corner and weight must be 16-byte aligned");
  if (!labels && !logits) return pcs_set_einval(fn, "NULL pointer (logits are required without labels)");
  if (labels && (!class_weight || !inv_wsum || !loss))
    return pcs_set_einval(fn, "NULL pointer (class_weight, inv_wsum and loss are required with labels)");
  if (labels && (!workspace || misaligned(workspace) ||
                 workspace_bytes < head_logits_floats(T, K) * (int64_t)sizeof(float)))
    return pcs_set_einval(fn, MSG_WS);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const Blocks b = reduction_blocks(T, THREADS);
  float *part_db = static_cast<float *>(workspace);
  float *part_loss = part_db ? part_db + (int64_t)b.n * K : nullptr;
  const dim3 grid(b.n), block(THREADS);
#define PCS_PH_CALL(KT)                                                                                               \
  do {                                                                                                                \
    if (labels)                                                                                                       \
      hipLaunchKernelGGL((head_logits_kernel<KT, true>), grid, block, 0, s, Z, corner, weight, T, (int)K, bias, labels, \
                         class_weight, inv_wsum, logits, dlogits, b.per, part_loss, db ? part_db : nullptr);          \
    else                                                                                                              \
      hipLaunchKernelGGL((head_logits_kernel<KT, false>), grid, block, 0, s, Z, corner, weight, T, (int)K, bias,       \
                         labels, class_weight, inv_wsum, logits, nullptr, b.per, nullptr, nullptr);                   \
  } while (0)
  PCS_PH_K(K, PCS_PH_CALL);
#undef PCS_PH_CALL
  PCS_CHECK_LAUNCH();
  if (!labels) return 0;
  if (int rc = pcs_reduce_partials(part_loss, b.n, 1, 1.f, loss, 1, 1, stream)) return rc;
  if (db)
    if (int rc = pcs_reduce_partials(part_db, b.n, K, 1.f, db, K, K, stream)) return rc;
  return 0;
}

extern "C" int pcs_point_head_bwd(const float *dlogits, const int32_t *pair_point, const float *pair_weight,
                                  const int64_t *seg_off, const void *X, int32_t xdtype, int64_t V, int32_t C,
                                  const float *W, int32_t K, const float *gscale, void *dX, void *workspace,
                                  int64_t workspace_bytes, float *dW, pcs_stream_t stream) {
  const char *fn = "pcs_point_head_bwd";
  if (V < 0) return pcs_set_einval(fn, "V >= 0 required");
  if (K < 1 || K > MAX_K) return pcs_set_einval(fn, MSG_K);
  if (bad_channels(C)) return pcs_set_einval(fn, MSG_C);
  if (!known(xdtype)) return pcs_set_einval(fn, MSG_DTYPE);
  if (V == 0) return 0;
  if (!dlogits || !pair_point || !pair_weight || !seg_off) return pcs_set_einval(fn, "NULL pointer");
  if ((dX && !W) || (dW && !X)) return pcs_set_einval(fn, "NULL pointer (dX needs W, dW needs X)");
  if (!workspace || misaligned(workspace) || workspace_bytes < head_bwd_floats(V, C, K) * (int64_t)sizeof(float))
    return pcs_set_einval(fn, MSG_WS);
  if (!dX && !dW) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const Blocks b = reduction_blocks(V, ROW_TILE);
  float *dZ = static_cast<float *>(workspace);
  float *part = dZ + round4(V * K);
  const dim3 block(THREADS), grid_dz(stream_blocks(V, THREADS, 1 << 16)), grid(b.n);
#define PCS_PH_CALL(KT)                                                                                              \
  do {                                                                                                               \
    hipLaunchKernelGGL((head_dz_kernel<KT>), grid_dz, block, 0, s, dlogits, pair_point, pair_weight, seg_off, V,      \
                       (int)K, gscale, dZ);                                                                          \
    if (xdtype == PCS_BF16)                                                                                          \
      hipLaunchKernelGGL((head_bwd_kernel<bf16_t, KT>), grid, block, 0, s, dZ, static_cast<const bf16_t *>(X), V,     \
                         (int)C, W, (int)K, b.per, static_cast<bf16_t *>(dX), dW ? part : nullptr);                  \
    else                                                                                                             \
      hipLaunchKernelGGL((head_bwd_kernel<float, KT>), grid, block, 0, s, dZ, static_cast<const float *>(X), V,       \
                         (int)C, W, (int)K, b.per, static_cast<float *>(dX), dW ? part : nullptr);                   \
  } while (0)
  PCS_PH_K(K, PCS_PH_CALL);
#undef PCS_PH_CALL
  PCS_CHECK_LAUNCH();
  if (dW) {
    const int64_t nw = (int64_t)K * C;
    if (int rc = pcs_reduce_partials(part, b.n, nw, 1.f, dW, nw, nw, stream)) return rc;
  }
  return 0;
}
