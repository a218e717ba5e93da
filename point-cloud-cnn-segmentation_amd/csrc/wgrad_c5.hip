// conv5's R = dz5^T a4 (a4 = relu(bn4(y4))) as one LDS-DMA stream: the alpha-term of conv5's
// weight gradient and, through pcs_bn_s2_from_r, bn5's S2 (autograd of P:110 at P:254).
//
// The register-staged pcs_wgrad kernel (gemm_tn.hip, 128 x 128 tiles, 64-row steps, a barrier
// and a register round trip per step) read dz5 and y4 at 4.5-4.9 TB/s (3.95-4.26 ms at cfg2).
// Here the fused seg backward's weight-gradient half (the r03 fused_seg.hip, now in git history) without its input gradient:
// * a workgroup (8 waves) owns NB = 256 dz5 columns and all 128 a4 channels of a scene-aligned
//   row slice: the [256 x 128] fp32 partial of R stays in registers (64 per lane), the slice's
//   partial goes out once, summed over the slices by pcs_reduce_partials (fixed order);
// * 32-row steps of dz5 (16 KB) and y4 (8 KB) through a 2-stage LDS ring by LDS-DMA, counted
//   waits; relu(bn4(y4)) formed once per element into a double-buffered x tile (the 4 column
//   blocks of a slice repeat this 128-wide transform, on one XCD, through L2);
// * MFMA operands by ds_read_b64_tr_b16 of the row-major dz5 and x tiles (k = rows), the
//   layouts (slot permutations, padded x rows) of the r03 fused_seg.hip, now in git history: bank-conflict free.
#include "kernel_prims.h"

namespace {

constexpr int THREADS = 512;
constexpr int MS = 32;           // rows per step
constexpr int NB = 256;          // dz5 columns per workgroup
constexpr int CIN = 128;         // a4 channels
static_assert(MS == route::WC5_MS && NB == route::WC5_NB && CIN == route::WC5_CIN, "route.h");
// two stages (66 KB of LDS) so that two workgroups share a CU (512 in the grid): 3.85 -> 3.64 ms
// in tools/bench_wc5.py against four stages at one workgroup per CU (three: 3.85)
#ifndef WC5_NST
#define WC5_NST 2
#endif
constexpr int NST = WC5_NST;     // ring stages
constexpr int ROWB = NB * 2;     // 512-B dz5 rows in LDS
constexpr int SPR = ROWB / 16;   // 32 slots
constexpr int DZB = MS * ROWB;   // 16 KB
constexpr int YROW = CIN * 2;    // 256-B y4 rows
constexpr int YB = MS * YROW;    // 8 KB
constexpr int STAGE = DZB + YB;
constexpr int XR = CIN * 2 + 32;  // x row stride (32-B pad, prow rows)
constexpr int XB = MS * XR;
constexpr int OFF_X = NST * STAGE;
constexpr int BYTES = OFF_X + 2 * XB;
static_assert(BYTES <= 160 * 1024, "LDS budget");
constexpr int DZP = DZB / 1024 / 8;   // dz5 pieces per wave per step (2)
constexpr int LPS = DZP + 1;          // + one y4 piece
constexpr int OBW = NB / 128;         // 16-column output tiles of dz5 per wave (2)

// slot permutations (the r03 fused_seg.hip, now in git history): dz5 rows chunk c at c ^ ftr(r); y4 rows at c ^ (r & 15);
// x rows permuted (prow: bits 2 <-> 3) and padded

__global__ __launch_bounds__(THREADS) void wgrad_c5_kernel(pcs_wgrad_args a, int64_t rows_per_split) {
  __shared__ __attribute__((aligned(16))) char lds[BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Cout = a.Cout, ncb = Cout / NB;
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int split = __builtin_amdgcn_readfirstlane(L / ncb), n0 = __builtin_amdgcn_readfirstlane((L % ncb) * NB);
  const int sps = a.splits_per_scene;
  const int scene = __builtin_amdgcn_readfirstlane(split / sps), sis = __builtin_amdgcn_readfirstlane(split % sps);
  const int64_t N = a.scene_rows;
  const int64_t lo = (int64_t)sis * rows_per_split;
  const int64_t hi = pcs_min64(lo + rows_per_split, N);
  const int64_t sbase = (int64_t)scene * N;
  // <= 0 for an empty trailing slice (a caller's splits_per_scene whose rounded slices pass the scene's
  // end, hi <= lo): the prologue's DMA clamps to row hi - 1 = N - 1, its transform writes zeros
  // (rem <= 0), no step runs and the partial is zeros
  const int nsteps = (int)((hi - lo + MS - 1) / MS);
  const char *Dg = reinterpret_cast<const char *>(a.dZ) + n0 * 2;   // dz5 [M][Cout], this block's columns
  const char *Yg = reinterpret_cast<const char *>(a.X);             // y4 [M][128]
  const int64_t drow = (int64_t)Cout * 2;

  // transform: thread -> y4 row tid / 16, logical 16-B chunk tid % 16 (8 channels: bn4 scale /
  // shift in registers)
  const int xlc = tid & 15, xrr = tid >> 4;
  float xs[8], xt[8];
  load_vec<8>(a.s, 8 * xlc, xs);
  load_vec<8>(a.t, 8 * xlc, xt);
#pragma unroll
  for (int e = 0; e < 8; ++e) asm volatile("" ::"v"(xs[e]), "v"(xt[e]));   // retired before the DMA
  __syncthreads();

  // ---- DMA of step s into stage sidx: dz5 pieces j = wid + 8 i (2 rows of 512 B each), the y4
  // piece wid (4 rows of 256 B); rows past the slice clamp to its last row (their x rows are
  // zeroed by the transform, so they add nothing)
  auto dz_off = [&](int i, int lastr) -> uint32_t {
    const int j = wid + 8 * i;
    const int r = j * 2 + lane / SPR, ps = lane % SPR;
    return (uint32_t)((int64_t)min(r, lastr) * drow + ((ps ^ ftr(r)) << 4));
  };
  auto y_off = [&](int lastr) -> uint32_t {
    const int r = wid * 4 + (lane >> 4);
    return (uint32_t)(min(r, lastr) * YROW + (((lane & 15) ^ (r & 15)) << 4));
  };
  uint32_t voff[LPS];
#pragma unroll
  for (int i = 0; i < DZP; ++i) voff[i] = dz_off(i, MS - 1);
  voff[DZP] = y_off(MS - 1);
  const uint32_t lds_m0 = (uint32_t)(uintptr_t)(lds_void_t *)lds;
  auto dma_issue = [&](int sidx, int64_t m0, const uint32_t (&vo)[LPS]) {
    const uint32_t mb = lds_m0 + sidx * STAGE + wid * 1024;
    const char *bd = Dg + (sbase + m0) * drow;
    const char *by = Yg + (sbase + m0) * YROW;
    const uint32_t keep = m0_save();
    glds16o<0>(bd, vo[0], mb);
    glds16o<8192>(bd, vo[1], mb);
    glds16o<DZB>(by, vo[2], mb);
    m0_restore(keep);
  };
  static_assert(DZP == 2, "two dz5 pieces per wave per step");
  auto dma_step = [&](int s, int sidx) {
    const int64_t m0 = pcs_min64(lo + (int64_t)s * MS, hi - 1);
    const int lastr = (int)pcs_min64(hi - 1 - m0, MS - 1);
    if (lastr == MS - 1) {   // uniform: a full step
      dma_issue(sidx, m0, voff);
    } else {
      uint32_t vt[LPS];
#pragma unroll
      for (int i = 0; i < DZP; ++i) vt[i] = dz_off(i, lastr);
      vt[DZP] = y_off(lastr);
      dma_issue(sidx, m0, vt);
    }
  };

  // x = relu(bn4(y4)) of step s into x buffer s & 1; rows past the slice -> 0
  const int o_yx = DZB + xrr * YROW + ((xlc ^ (xrr & 15)) << 4);
  const int o_xw = prow(xrr) * XR + xlc * 16;
  auto transform = [&](int s, int sidx) {
    const int rem = (int)pcs_min64(hi - (lo + (int64_t)s * MS), MS);
    float v[8];
    unpack_chunk(*reinterpret_cast<const u32x4 *>(lds + sidx * STAGE + o_yx), v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = relu(fmaf(v[e], xs[e], xt[e]));
    u32x4 out = pack_chunk(v);
    if (xrr >= rem) out = mk_u32x4(0, 0, 0, 0);
    *reinterpret_cast<u32x4 *>(lds + OFF_X + (s & 1) * XB + o_xw) = out;
  };

  // transposed-read offsets (the r03 fused_seg.hip, now in git history's weight-gradient half): dz5 columns 16 (2 wid + ob) +
  // 4 p of rows 8 g + q and 8 g + 4 + q; x columns 16 u + 4 p of the same rows
  const int g = lane >> 4, l16 = lane & 15, q = (lane >> 2) & 3, p = lane & 3;
  const int tr0 = 8 * g + q, tr1 = 8 * g + 4 + q;
  int o_td[OBW][2];
#pragma unroll
  for (int ob = 0; ob < OBW; ++ob) {
    const int s = 2 * (OBW * wid + ob) + (p >> 1);   // logical chunk of columns 16 (OBW wid + ob) + 4 p
    o_td[ob][0] = tr0 * ROWB + ((s ^ ftr(tr0)) << 4) + 8 * (p & 1);
    o_td[ob][1] = tr1 * ROWB + ((s ^ ftr(tr1)) << 4) + 8 * (p & 1);
  }
  const int o_tx0 = prow(tr0) * XR + 8 * p, o_tx1 = prow(tr1) * XR + 8 * p;   // + u 32 B

  f32x4 acc[OBW][8];
#pragma unroll
  for (int ob = 0; ob < OBW; ++ob)
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[ob][u] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- prologue: steps 0 .. NST-2 in flight, step 0 landed and transformed
#pragma unroll
  for (int s = 0; s < NST - 1; ++s) dma_step(s, s);
  wait_vm<(NST - 2) * LPS>();
  barrier_lds();
  transform(0, 0);
  barrier_lds();

  int sc = 0;
  for (int t = 0; t < nsteps; ++t) {
    const int sn = sc + 1 == NST ? 0 : sc + 1;
    dma_step(t + NST - 1, sc == 0 ? NST - 1 : sc - 1);   // into the stage of step t-1
    const char *st = lds + sc * STAGE;
    const char *xb = lds + OFF_X + (t & 1) * XB;
    bf16x8 dt[OBW], xf[2];
#pragma unroll
    for (int ob = 0; ob < OBW; ++ob) dt[ob] = tr_frag2(st + o_td[ob][0], st + o_td[ob][1]);
    xf[0] = tr_frag2(xb + o_tx0, xb + o_tx1);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (u + 1 < 8) xf[(u + 1) & 1] = tr_frag2(xb + o_tx0 + (u + 1) * 32, xb + o_tx1 + (u + 1) * 32);
#pragma unroll
      for (int ob = 0; ob < OBW; ++ob)
        acc[ob][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[u & 1], dt[ob], acc[ob][u], 0, 0, 0);
    }
    // step t+1 landed (newer: NST-2 steps' pieces)
    wait_vm<(NST - 2) * LPS>();
    barrier_lds();
    if (t + 1 < nsteps) transform(t + 1, sn);
    barrier_lds();
    sc = sn;
  }
  wait_vm<0>();   // the clamped DMAs past the end

  // ---- this slice's partial: R[n0 + 16 (OBW wid + ob) + l16][16 u + 4 g .. + 4]
  float *out = a.partial + ((int64_t)split * Cout + n0) * CIN;
#pragma unroll
  for (int ob = 0; ob < OBW; ++ob)
#pragma unroll
    for (int u = 0; u < 8; ++u)
      *reinterpret_cast<float4 *>(out + (int64_t)(16 * (OBW * wid + ob) + l16) * CIN + 16 * u + 4 * g) =
          make_float4(acc[ob][u][0], acc[ob][u][1], acc[ob][u][2], acc[ob][u][3]);
}

// ---------------------------------------------------------------------------------------
// The Gram of a4 = relu(bn4(y4)) (pcs_gram at C = 128: bn5's statistics from G = a4^T a4 and the
// column sums of a4, fwd_stats:conv5).  The generic tiled kernel reads y4 once per 64-wide tile
// column (3.2 TB/s, 0.66 ms at cfg2); here one workgroup owns all 128 x 128 of a row slice:
// * 64-row steps of y4 (16 KB) through an NST-stage LDS ring by LDS-DMA, rows in the transposed-
//   read layout (chunk c at c ^ ftr(r)); relu(bn4(.)) applied in place, rows past the slice zeroed;
// * both MFMA operands are transposed reads of that tile: wave w accumulates G[16 w + l16][all]
//   (8 blocks, 32 fp32 per lane); the fp32 column sums ride the transform.
constexpr int G_MS = 64;                  // rows per step
static_assert(G_MS == route::GRAM128_MS, "route.h");
#ifndef GRAM_NST
#define GRAM_NST 4
#endif
constexpr int G_NST = GRAM_NST;
constexpr int G_YB = G_MS * YROW;         // 16 KB
constexpr int G_LPS = G_YB / 1024 / 8;    // 1-KB DMA pieces per wave per step (2)
constexpr int G_BYTES = G_NST * G_YB;
static_assert(G_BYTES + 8 * CIN * 4 <= 160 * 1024, "LDS budget");

__global__ __launch_bounds__(THREADS) void gram128_kernel(pcs_wgrad_args a, int64_t rows_per_split) {
  __shared__ __attribute__((aligned(16))) char lds[G_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int split = xcd_remap(blockIdx.x, gridDim.x);
  const int sps = a.splits_per_scene;
  const int scene = __builtin_amdgcn_readfirstlane(split / sps), sis = __builtin_amdgcn_readfirstlane(split % sps);
  const int64_t N = a.scene_rows;
  const int64_t lo = (int64_t)sis * rows_per_split;
  const int64_t hi = pcs_min64(lo + rows_per_split, N);
  const int64_t sbase = (int64_t)scene * N;
  // an empty trailing slice (splits x rounded rows past the scene) runs no step and writes zeros
  const int nsteps = hi > lo ? (int)((hi - lo + G_MS - 1) / G_MS) : 0;
  const char *Yg = reinterpret_cast<const char *>(a.Y);

  // transform: thread -> rows tid / 16 and 32 + tid / 16, logical chunk tid % 16 (8 channels)
  const int xlc = tid & 15, xrr = tid >> 4;
  float xs[8], xt[8], cs[8];
  load_vec<8>(a.s, 8 * xlc, xs);
  load_vec<8>(a.t, 8 * xlc, xt);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    asm volatile("" ::"v"(xs[e]), "v"(xt[e]));   // retired before the DMA
    cs[e] = 0.f;
  }
  __syncthreads();

  // DMA pieces j = wid + 8 i: 4 rows of 256 B each; rows past the slice clamp to its last row
  auto y_off = [&](int i, int lastr) -> uint32_t {
    const int r = (wid + 8 * i) * 4 + (lane >> 4), ps = lane & 15;
    return (uint32_t)(min(r, lastr) * YROW + ((ps ^ ftr(r)) << 4));
  };
  uint32_t voff[G_LPS];
#pragma unroll
  for (int i = 0; i < G_LPS; ++i) voff[i] = y_off(i, G_MS - 1);
  const uint32_t lds_m0 = (uint32_t)(uintptr_t)(lds_void_t *)lds;
  static_assert(G_LPS == 2, "two y4 pieces per wave per step");
  auto dma_issue = [&](int sidx, int64_t m0, const uint32_t (&vo)[G_LPS]) {
    const uint32_t mb = lds_m0 + sidx * G_YB + wid * 1024;
    const char *by = Yg + (sbase + m0) * YROW;
    const uint32_t keep = m0_save();
    glds16o<0>(by, vo[0], mb);
    glds16o<8192>(by, vo[1], mb);
    m0_restore(keep);
  };
  auto dma_step = [&](int s) {
    const int64_t m0 = pcs_min64(lo + (int64_t)s * G_MS, hi - 1);
    const int lastr = (int)pcs_min64(hi - 1 - m0, G_MS - 1);
    const int sidx = s % G_NST;
    if (lastr == G_MS - 1) {   // uniform: a full step
      dma_issue(sidx, m0, voff);
    } else {
      uint32_t vt[G_LPS];
#pragma unroll
      for (int i = 0; i < G_LPS; ++i) vt[i] = y_off(i, lastr);
      dma_issue(sidx, m0, vt);
    }
  };
  // in place: a4 over y4 in the stage, rows past the slice -> 0
  auto transform = [&](int s) {
    const int rem = (int)pcs_min64(hi - (lo + (int64_t)s * G_MS), G_MS);
    char *st = lds + (s % G_NST) * G_YB;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = xrr + 32 * h;
      u32x4 *pc = reinterpret_cast<u32x4 *>(st + r * YROW + ((xlc ^ ftr(r)) << 4));
      float v[8];
      unpack_chunk(*pc, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = r < rem ? relu(fmaf(v[e], xs[e], xt[e])) : 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) cs[e] += v[e];   // column sums in fp32 (as the tiled kernel)
      *pc = pack_chunk(v);
    }
  };

  // transposed reads: columns 16 u + 4 p of rows 32 kk + 8 g + q and 32 kk + 8 g + 4 + q
  const int g = lane >> 4, l16 = lane & 15, q = (lane >> 2) & 3, p = lane & 3;
  const int tr0 = 8 * g + q, tr1 = 8 * g + 4 + q;
  auto o_frag = [&](int u, int row) { return row * YROW + (((2 * u + (p >> 1)) ^ ftr(row)) << 4) + 8 * (p & 1); };
  // symmetric: wave w forms the 16-wide blocks (w, w + d mod 8), d = 0 .. 3 (and d = 4 for w < 4):
  // the 36 blocks of one triangle; the partial gets each block and its transpose
  constexpr int NU = 5;
  const int nu = wid < 4 ? 5 : 4;
  int o_u[NU][2];
#pragma unroll
  for (int d = 0; d < NU; ++d) {
    const int u = (wid + d) & 7;
    o_u[d][0] = o_frag(u, tr0);
    o_u[d][1] = o_frag(u, tr1);
  }
  const int o_w0 = o_frag(wid, tr0), o_w1 = o_frag(wid, tr1);

  f32x4 acc[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int s = 0; s < G_NST - 1; ++s) dma_step(s);
  for (int t = 0; t < nsteps; ++t) {
    wait_vm<(G_NST - 2) * G_LPS>();   // step t landed (t+1 .. t+NST-2 in flight)
    barrier_lds();                     // ... for every wave; all done with step t-1's stage
    dma_step(t + G_NST - 1);           // into step t-1's stage
    transform(t);
    barrier_lds();
    const char *st = lds + (t % G_NST) * G_YB;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int kb = kk * 32 * YROW;
      const bf16x8 w = tr_frag2(st + kb + o_w0, st + kb + o_w1);
      bf16x8 xf[2];
      xf[0] = tr_frag2(st + kb + o_u[0][0], st + kb + o_u[0][1]);
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        if (u + 1 < NU) xf[(u + 1) & 1] = tr_frag2(st + kb + o_u[u + 1][0], st + kb + o_u[u + 1][1]);
        if (u < 4 || u < nu) acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[u & 1], w, acc[u], 0, 0, 0);
      }
    }
  }
  wait_vm<0>();   // the clamped DMAs past the end

  // G partial: [16 wid + l16][16 u + 4 g .. + 4]
  float *out = a.partial + (int64_t)split * CIN * CIN;
#pragma unroll
  for (int d = 0; d < NU; ++d) {
    if (d >= nu) continue;
    const int u = (wid + d) & 7;
    *reinterpret_cast<float4 *>(out + (int64_t)(16 * wid + l16) * CIN + 16 * u + 4 * g) =
        make_float4(acc[d][0], acc[d][1], acc[d][2], acc[d][3]);
    if (d > 0) {   // the transposed block
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(int64_t)(16 * u + 4 * g + r) * CIN + 16 * wid + l16] = acc[d][r];
    }
  }
  // column sums: lanes l, l + 16, l + 32, l + 48 of a wave, then the 8 waves through LDS
  __syncthreads();
  float *red = reinterpret_cast<float *>(lds);   // [8 waves][128]
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float v = cs[e];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    cs[e] = v;
  }
  if (lane < 16) {
#pragma unroll
    for (int e = 0; e < 8; ++e) red[wid * CIN + 8 * lane + e] = cs[e];
  }
  __syncthreads();
  if (tid < CIN) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) v += red[w * CIN + tid];
    const int64_t nsplit = a.num_scenes * (int64_t)sps;
    a.partial[nsplit * CIN * CIN + (int64_t)split * CIN + tid] = v;
  }
}

}  // namespace

int pcs_gram128_launch(const pcs_wgrad_args &a, hipStream_t s) {
  const int64_t rps = route::rows_per_split(a.scene_rows, a.splits_per_scene, G_MS);
  const int nb = (int)(a.num_scenes * a.splits_per_scene);
  hipLaunchKernelGGL(gram128_kernel, dim3(nb), dim3(THREADS), 0, s, a, rps);
  PCS_CHECK_LAUNCH();
  return 0;
}

int pcs_wgrad_c5_launch(const pcs_wgrad_args &a, int64_t rows_per_split, hipStream_t s) {
  if (rows_per_split % MS) return pcs_set_einval("pcs_wgrad", "conv5 R: rows per split must be a multiple of 32");
  const int nb = (int)(a.num_scenes * a.splits_per_scene) * (a.Cout / NB);
  hipLaunchKernelGGL(wgrad_c5_kernel, dim3(nb), dim3(THREADS), 0, s, a, rows_per_split);
  PCS_CHECK_LAUNCH();
  return 0;
}
