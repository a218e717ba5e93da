// Dense 3-D convolution on channels-last voxel grids: the north star's "3x3x3 Conv3d U-Net with
// LDS-staged stencils, transposed conv" building blocks.  Build-defined: the
// reference (P) has no voxel grid, so parity is against torch.nn.functional.conv3d /
// conv_transpose3d in fp64 (tests/test_gpu_conv3d.py), not against the reference.
//
// Layouts: X [B, D, H, W, C] bf16 (channels innermost), W [Cout, k, k, k, Cin] bf16 (one row of
// taps x input channels per output channel), Y [B, D', H', W', Cout] f32 or bf16.
//   conv       Y[o] = b + sum_t W_t X[o s - p + t]
//   transposed Y[o] = b + sum_t W_t X[(o + p - t) / s]   (only where o + p - t is a multiple of s)
// The input gradient of one is the other with W_t transposed (pcs_conv3d_weight_t), so one
// kernel serves the forward and the input gradient of both; the weight gradient uses the
// forward's index map.
//
// Every gather convolution in this file is one of two loops with a different row index:
//   gather_gemm_tile + store_tile: the forward / input-gradient implicit GEMM, rows = output rows,
//     columns = output channels, k = (tap, channel slice).  A k-step gathers the tile's input rows
//     of one tap into LDS (zero rows where there is none): a stencil is shifted gathers of the
//     same channels-last rows, so after the first tap the re-reads come from L2.  Instantiated by
//     conv3d_kernel (rows from the grid geometry), sparse_conv_kernel (rows from a neighbour map,
//     only the taps a tile meets), pair_gemm_kernel and pair_rows_kernel (rows from one tap's
//     pair list; the first stores raw products, the second scatters through pair_out).
//   wgrad_tile + store_wgrad_tile: dW_t = dY^T X_t over rows in 32-row k-steps, both operands
//     staged row-major and read transposed (ds_read_b64_tr_b16) so the MFMA's k runs over rows;
//     split over row slices with fp32 partials summed in a fixed order (deterministic).
//     Instantiated by conv3d_wgrad_kernel, sparse_wgrad_kernel (up to TG taps share one dY image)
//     and pair_wgrad_kernel (one tap's pair list).
// The sparse kernels take their X operand as one array or as two column blocks (Rows1 / Rows2) and
// their output likewise (Out1 / Out2): the two-source layer pcs_sparse_conv_cat*, a decoder's
// convolution of [up | skip] without the concatenated array, in the same k-step order.
// The 3x3x3 stride-1 stencil has its own halo-staged kernels (stencil3_kernel, stencil3_wgrad_kernel).
// Every forward kernel stores its rows through an epilogue policy (EpiNone / EpiAffine below): the
// pcs_*_affine entry points of include/pcs_fold.h fold an eval-mode BatchNorm (+ residual) (+ ReLU) into
// the store, for inference.
#include "../../include/pcs_dense.h"
#include "../../include/pcs_fold.h"
#include "kernel_prims.h"

namespace {

constexpr int THREADS = 256;
constexpr int BN = 64, KS = 32;   // output channels per tile, k-step (bf16 elements)

// 16-B slot swizzle of a 64-B LDS row: conflict-free ds_read_b128 fragment reads (rows 4 apart
// land on different slots of a 256-B bank row)
PCS_DEV int cswz(int row, int slot) { return slot ^ ((-(row >> 2)) & 3); }

// Where the rows of a gathered X operand live: one [rows, Cin] array (Rows1), or two column blocks
// [rows, CA] | [rows, Cin - CA] read as their concatenation along channels (Rows2: a U-Net decoder's
// [up, skip] without the copy).  Arg is what a kernel takes (a plain pointer for one array, so the
// single-source kernels keep their arguments) and at(X, row, Cin, c) the address of channel c of a
// row.  In the sparse kernels c and CA are multiples of 64, the widest channel slice a k-step or a
// weight-gradient tile reads, so a slice never straddles the blocks and the choice is uniform over
// the workgroup; the dense stencil kernels call at() per 16-byte chunk (c a multiple of 8, CA of 32),
// so a 64-channel slice may straddle the blocks.  Either way the order of k-steps is that of the
// concatenated array, so the sums are bit-identical to it.
struct Rows1 {
  static constexpr bool SPLIT = false;
  using Arg = const bf16_t *__restrict__;
  static PCS_DEV const bf16_t *at(const bf16_t *X, int64_t row, int Cin, int c) { return X + row * Cin + c; }
};
struct Rows2 {
  static constexpr bool SPLIT = true;
  using Arg = Rows2;
  const bf16_t *XA, *XB;
  int CA;
  static PCS_DEV const bf16_t *at(const Rows2 &X, int64_t row, int Cin, int c) {
    return c < X.CA ? X.XA + row * X.CA + c : X.XB + row * (Cin - X.CA) + (c - X.CA);
  }
};
// The same for an output Y [rows, Cout]: pick(Y, c0, ld) takes the first channel c0 of a 64-channel
// tile (or 8-channel chunk; the dense stencil: of a 4-channel store group, so a tile may straddle
// the blocks) and ld = Cout, returns the array that holds it and turns (c0, ld) into the channel and
// the leading dimension there (Out2: an input gradient written as two column blocks).
struct Out1 {
  static constexpr bool SPLIT = false;
  using Arg = void *__restrict__;
  static PCS_DEV void *pick(void *Y, int &, int &) { return Y; }
};
struct Out2 {
  static constexpr bool SPLIT = true;
  using Arg = Out2;
  void *YA, *YB;
  int CA;
  static PCS_DEV void *pick(const Out2 &Y, int &c0, int &ld) {
    if (c0 < Y.CA) { ld = Y.CA; return Y.YA; }
    c0 -= Y.CA; ld -= Y.CA;
    return Y.YB;
  }
};

// What a forward kernel does to its fp32 accumulators (+ bias) where it stores them, at the three
// places rows are stored (store_tile, the end of stencil3_kernel, pair_reduce_kernel).  EpiNone:
// nothing, the plain convolution.  EpiAffine (include/pcs_fold.h): an eval-mode BatchNorm (+ residual)
// (+ ReLU) folded into the store,
//   y = act(fmaf(v, scale[c], shift[c]) (+ R[row][c])),  act = relu or the identity
// which is pcs_sparse_bn_apply's statement in its operation order (an explicit fmaf, then the
// residual's own add), so a folded layer is bit-identical to that pass run on the convolution's fp32
// output.  R: rows in Y's dtype, row indexing and leading dimension, or NULL.  relu and R are run-time
// (uniform) flags: a kernel has one affine instantiation per plain one.  Affine kernels write one
// array (Out1).
struct EpiNone { static constexpr bool AFFINE = false; };
struct EpiAffine {
  static constexpr bool AFFINE = true;
  const float *scale, *shift;   // f32 [Cout]
  const void *R;
  int relu;
};
// a lane's coefficients of N consecutive channels (4 or 8): loaded once per column tile, outside the row loop
template <int N> struct EpiCoef { float s[N], t[N]; };
template <int N>
PCS_DEV EpiCoef<N> epi_coef(const EpiAffine &ep, int c) {
  EpiCoef<N> k;
  load_vec<N>(ep.scale, c, k.s);
  load_vec<N>(ep.shift, c, k.t);
  return k;
}
template <int N> PCS_DEV EpiNone epi_coef(const EpiNone &, int) { return EpiNone{}; }
// v[0 .. N) = the N channels stored at element offset off of Y (and of R, read in the store's width)
template <bool OUT_BF16, int N>
PCS_DEV void epi_apply(const EpiAffine &ep, const EpiCoef<N> &k, int64_t off, float (&v)[N]) {
#pragma unroll
  for (int e = 0; e < N; ++e) v[e] = fmaf(v[e], k.s[e], k.t[e]);
  if (ep.R) {
    float r[N];
    if constexpr (OUT_BF16 && N == 4) {
      const uint2 q = *reinterpret_cast<const uint2 *>(static_cast<const bf16_t *>(ep.R) + off);
      r[0] = bf2f(q.x & 0xffffu); r[1] = bf2f(q.x >> 16); r[2] = bf2f(q.y & 0xffffu); r[3] = bf2f(q.y >> 16);
    } else if constexpr (OUT_BF16) {
      unpack_chunk(*reinterpret_cast<const u32x4 *>(static_cast<const bf16_t *>(ep.R) + off), r);
    } else {
      load_vec<N>(static_cast<const float *>(ep.R) + off, 0, r);
    }
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] += r[e];
  }
  if (ep.relu) {
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = relu(v[e]);
  }
}
// A kernel takes its epilogue as a trailing parameter pack of zero or one EpiAffine, so that the plain
// kernels keep exactly their parameters; epi_of(ep...) is the pack's epilogue.  The store sites call
// epi_apply behind an if constexpr: even a call that compiles to nothing there moved the register
// allocation of ten plain instantiations by 2 to 4 VGPRs; with it they compile to their former figures.
PCS_DEV EpiNone epi_of() { return EpiNone{}; }
PCS_DEV EpiAffine epi_of(const EpiAffine &e) { return e; }

// input voxel feeding output voxel (b, z, y, x) through tap (dz, dy, dx); -1 = none (zero)
PCS_DEV int64_t in_voxel(const pcs_conv3d_geom &g, int b, int z, int y, int x, int dz, int dy, int dx) {
  int iz, iy, ix;
  if (!g.transposed) {
    iz = z * g.s - g.p + dz;
    iy = y * g.s - g.p + dy;
    ix = x * g.s - g.p + dx;
  } else {
    const int tz = z + g.p - dz, ty = y + g.p - dy, tx = x + g.p - dx;
    if (tz < 0 || ty < 0 || tx < 0) return -1;
    if (g.s == 2 && ((tz | ty | tx) & 1)) return -1;
    const int sh = g.s == 2 ? 1 : 0;
    iz = tz >> sh;
    iy = ty >> sh;
    ix = tx >> sh;
  }
  if (iz < 0 || iy < 0 || ix < 0 || iz >= g.Di || iy >= g.Hi || ix >= g.Wi) return -1;
  return (((int64_t)b * g.Di + iz) * g.Hi + iy) * g.Wi + ix;
}

// output voxel u -> (b, z, y, x); 32-bit divisions when u fits (a 64-bit division is ~10x dearer)
PCS_DEV void decode(const pcs_conv3d_geom &g, int64_t u, int &b, int &z, int &y, int &x) {
  if (u < ((int64_t)1 << 31)) {
    uint32_t v = (uint32_t)u;
    x = (int)(v % (uint32_t)g.Wo);
    v /= (uint32_t)g.Wo;
    y = (int)(v % (uint32_t)g.Ho);
    v /= (uint32_t)g.Ho;
    z = (int)(v % (uint32_t)g.Do);
    b = (int)(v / (uint32_t)g.Do);
    return;
  }
  x = (int)(u % g.Wo);
  u /= g.Wo;
  y = (int)(u % g.Ho);
  u /= g.Ho;
  z = (int)(u % g.Do);
  b = (int)(u / g.Do);
}

// Transposed form with stride 2: an output voxel o only meets the taps t with o + p - t even, so
// the outputs fall into 8 parity classes c (o = 2 o' + c per dimension), each with its own tap
// subset (t = (c + p) mod 2, + 2, ... < k: one tap per dimension for k = 2).  Tiles are cut per
// class, so no MFMA runs on a tap that is off the lattice for every row.
struct PClass {
  int cz, cy, cx;   // parity of the class
  int nz, ny, nx;   // class sub-grid (output voxels 2 o' + c inside the grid)
  int tz0, ty0, tx0, ntz, nty, ntx;   // first tap and tap count per dimension
};

PCS_DEV PClass pclass(const pcs_conv3d_geom &g, int c) {
  PClass q;
  q.cz = (c >> 2) & 1; q.cy = (c >> 1) & 1; q.cx = c & 1;
  q.nz = (g.Do - q.cz + 1) >> 1; q.ny = (g.Ho - q.cy + 1) >> 1; q.nx = (g.Wo - q.cx + 1) >> 1;
  q.tz0 = (q.cz + g.p) & 1; q.ty0 = (q.cy + g.p) & 1; q.tx0 = (q.cx + g.p) & 1;
  q.ntz = q.tz0 < g.k ? (g.k - q.tz0 + 1) >> 1 : 0;
  q.nty = q.ty0 < g.k ? (g.k - q.ty0 + 1) >> 1 : 0;
  q.ntx = q.tx0 < g.k ? (g.k - q.tx0 + 1) >> 1 : 0;
  return q;
}

// class row u (b, z', y', x' over the class sub-grid) -> output voxel (b, z, y, x)
PCS_DEV void decode_class(const PClass &q, int64_t u, int &b, int &z, int &y, int &x) {
  if (u < ((int64_t)1 << 31)) {
    uint32_t v = (uint32_t)u;
    x = 2 * (int)(v % (uint32_t)q.nx) + q.cx;
    v /= (uint32_t)q.nx;
    y = 2 * (int)(v % (uint32_t)q.ny) + q.cy;
    v /= (uint32_t)q.ny;
    z = 2 * (int)(v % (uint32_t)q.nz) + q.cz;
    b = (int)(v / (uint32_t)q.nz);
    return;
  }
  x = 2 * (int)(u % q.nx) + q.cx;
  u /= q.nx;
  y = 2 * (int)(u % q.ny) + q.cy;
  u /= q.ny;
  z = 2 * (int)(u % q.nz) + q.cz;
  b = (int)(u / q.nz);
}

// ---- The gather-GEMM tile loop of every forward kernel here (conv3d_kernel, sparse_conv_kernel,
// pair_gemm_kernel, pair_rows_kernel): acc = sum over the tile's nrun taps j of W[wtap(j)] X[in_row],
// fp32, for BMT rows and the BNT output channels from n0.  The kernels differ only in where a row
// comes from: in_row(h, r, j) is the input row of staged row r = srow + RPP h (this thread's h-th
// staging pass) at run-tap j, or -1 for a zero row; wtap(j) is the weight tap of run-tap j.
// BMT = 64 or 128 rows per tile (4 waves as 2 x 2: wave tile BMT/2 x BNT/2); KST = 32 or 64 input
// channels per k-step (64: whole 128-B rows per load, 2x the MFMAs per barrier); BNT = 64 or 32
// output channels per tile (32: a 32-channel U-Net level without zero channels).  A k-step stages
// the rows of one (tap, channel slice) through registers into swizzled LDS; the next k-step is loaded
// while the MFMAs of this one run, one barrier per k-step.  Lane (lr, lg) of wave (wr, wc) ends
// with row wr BMT/2 + 16 i + lr, channels n0 + wc BNT/2 + 16 j + 4 lg .. + 3 in acc[i][j].
// XF is Rows1 or Rows2 (Cin = all its channels, the weight's).
template <int BMT, int KST, int BNT, class XF, class RowF, class TapF>
PCS_DEV void gather_gemm_tile(typename XF::Arg X, int Cin, const bf16_t *__restrict__ W, int taps, int n0,
                              int nrun, RowF in_row, TapF wtap, f32x4 (&acc_out)[BMT / 32][BNT / 32]) {
  constexpr int RB = KST * 2;          // LDS row bytes
  constexpr int CPR = KST / 8;         // 16-B chunks per row
  constexpr int RPP = THREADS / CPR;   // rows staged per pass
  constexpr int HA = BMT / RPP, HB = (BNT + RPP - 1) / RPP;
  constexpr bool WPART = BNT % RPP != 0;   // BNT < RPP (32 channels, 32-deep k-steps): the first BNT rows' threads
  constexpr int TI = BMT / 32;         // 16-row MFMA tiles per wave
  constexpr int TJ = BNT / 32;         // 16-channel MFMA tiles per wave
  constexpr int KK = KST / 32;         // MFMA k-steps per k-step
  __shared__ __attribute__((aligned(16))) char lds[2][(BMT + BNT) * RB];   // per buffer: A | B
  auto swzf = [](int row, int slot) { return KST == 32 ? cswz(row, slot) : (slot ^ ((row >> 1) & 7)); };
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1, lr = lane & 15, lg = lane >> 4;
  const int srow = tid / CPR, q = tid % CPR;   // staging: chunk q of rows srow + RPP h
  const int nks = nrun * (Cin / KST);
  const bf16_t *wrow = W + (int64_t)(n0 + srow) * taps * Cin + q * 8;
  const int64_t wstep = (int64_t)RPP * taps * Cin;

  u32x4 ra[HA], rb[HB];
  int lj = 0, lc = 0;   // the next k-step to load: run-tap lj, channels lc .. lc + KST (no division per k-step)
  auto load = [&]() {
    const int t = wtap(lj);
#pragma unroll
    for (int h = 0; h < HA; ++h) {
      const int64_t iv = in_row(h, srow + RPP * h, lj);
      ra[h] = iv >= 0 ? *reinterpret_cast<const u32x4 *>(XF::at(X, iv, Cin, lc) + q * 8) : mk_u32x4(0, 0, 0, 0);
    }
#pragma unroll
    for (int h = 0; h < HB; ++h)
      if (!WPART || srow + RPP * h < BNT) rb[h] = *reinterpret_cast<const u32x4 *>(wrow + h * wstep + (int64_t)t * Cin + lc);
    lc += KST;
    if (lc == Cin) { lc = 0; ++lj; }
  };
  auto stage = [&](int buf) {
    char *tA = lds[buf], *tB = lds[buf] + BMT * RB;
#pragma unroll
    for (int h = 0; h < HA; ++h) {
      const int r = srow + RPP * h;
      *reinterpret_cast<u32x4 *>(tA + r * RB + swzf(r, q) * 16) = ra[h];
    }
#pragma unroll
    for (int h = 0; h < HB; ++h) {
      const int r = srow + RPP * h;
      if (!WPART || r < BNT) *reinterpret_cast<u32x4 *>(tB + r * RB + swzf(r, q) * 16) = rb[h];
    }
  };

  f32x4 acc[TI][TJ];   // (locals, handed over once at the end: see wgrad_tile)
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (nks > 0) {
    load();
    stage(0);
  }
  __syncthreads();
  for (int ks = 0; ks < nks; ++ks) {
    const int buf = ks & 1;
    if (ks + 1 < nks) load();
    const char *tA = lds[buf], *tB = lds[buf] + BMT * RB;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      bf16x8 af[TI], bw[TJ];
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        const int r = wr * (BMT / 2) + i * 16 + lr;
        af[i] = *reinterpret_cast<const bf16x8 *>(tA + r * RB + swzf(r, kk * 4 + lg) * 16);
      }
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        const int r = wc * (BNT / 2) + j * 16 + lr;
        bw[j] = *reinterpret_cast<const bf16x8 *>(tB + r * RB + swzf(r, kk * 4 + lg) * 16);
      }
      // W rows as the MFMA A operand: each lane ends with 4 consecutive output channels of one row
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[j], af[i], acc[i][j], 0, 0, 0);
    }
    if (ks + 1 < nks) stage(buf ^ 1);   // buf ^ 1 was last read before the previous barrier
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc_out[i][j] = acc[i][j];
}

// The forward epilogue on gather_gemm_tile's accumulators: Y[out_row(r)][n0 ..] = acc + bias, 4
// channels of one row per store (bf16 or fp32); out_row(r) is the output row of tile row r, or -1
// to skip it.  ep (EpiNone or EpiAffine) acts on the biased sums before the store.
template <int BMT, int BNT, bool OUT_BF16, class RowF, class EP = EpiNone>
PCS_DEV void store_tile(const f32x4 (&acc)[BMT / 32][BNT / 32], RowF out_row, int n0, int Cout,
                        const float *__restrict__ bias, void *__restrict__ Y, const EP &ep = EP{}) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wr = wid >> 1, wc = wid & 1, lr = lane & 15, lg = lane >> 4;
  decltype(epi_coef<4>(ep, 0)) ek[BNT / 32];
  if constexpr (EP::AFFINE) {
#pragma unroll
    for (int j = 0; j < BNT / 32; ++j) ek[j] = epi_coef<4>(ep, n0 + wc * (BNT / 2) + j * 16 + 4 * lg);
  }
#pragma unroll
  for (int i = 0; i < BMT / 32; ++i) {
    const int64_t uo = out_row(wr * (BMT / 2) + i * 16 + lr);
    if (uo < 0) continue;
#pragma unroll
    for (int j = 0; j < BNT / 32; ++j) {
      const int co = n0 + wc * (BNT / 2) + j * 16 + 4 * lg;
      float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      if (bias) {
        const float4 bb = *reinterpret_cast<const float4 *>(bias + co);
        v[0] += bb.x; v[1] += bb.y; v[2] += bb.z; v[3] += bb.w;
      }
      if constexpr (EP::AFFINE) epi_apply<OUT_BF16>(ep, ek[j], uo * Cout + co, v);
      if constexpr (OUT_BF16) {
        *reinterpret_cast<uint2 *>(reinterpret_cast<bf16_t *>(Y) + uo * Cout + co) =
            make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
      } else {
        *reinterpret_cast<float4 *>(reinterpret_cast<float *>(Y) + uo * Cout + co) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  }
}

// The dense gather: rows = output voxels, zero rows off the grid or off the stride lattice
template <int BMT, int KST, bool OUT_BF16, int BNT = BN, class... EP>
__global__ __launch_bounds__(THREADS) void conv3d_kernel(pcs_conv3d_geom g, const bf16_t *__restrict__ X,
                                                         const bf16_t *__restrict__ W, const float *__restrict__ bias,
                                                         void *__restrict__ Y, int64_t M, EP... ep) {
  constexpr int RPP = THREADS / (KST / 8), HA = BMT / RPP;   // gather_gemm_tile's staging passes
  // class mode (transposed, stride 2): blockIdx.x = tile * 8 + class, rows index the class sub-grid
  const bool cm = g.transposed && g.s == 2;
  PClass pc{};
  int64_t Mrows = M;
  int64_t m0 = (int64_t)blockIdx.x * BMT;
  if (cm) {
    pc = pclass(g, blockIdx.x & 7);
    Mrows = g.B * pc.nz * pc.ny * pc.nx;
    m0 = (int64_t)(blockIdx.x >> 3) * BMT;
    if (m0 >= Mrows) return;   // uniform: this class has fewer tiles than the largest
  }
  const int srow = threadIdx.x / (KST / 8);
  bool rv[HA];
  int vb[HA], vz[HA], vy[HA], vx[HA];
#pragma unroll
  for (int h = 0; h < HA; ++h) {
    const int64_t u = m0 + srow + RPP * h;
    rv[h] = u < Mrows;
    vb[h] = vz[h] = vy[h] = vx[h] = 0;
    if (rv[h]) {
      if (cm) decode_class(pc, u, vb[h], vz[h], vy[h], vx[h]);
      else decode(g, u, vb[h], vz[h], vy[h], vx[h]);
    }
  }
  const int k = g.k, taps = k * k * k, n0 = blockIdx.y * BNT;
  // run-tap j of this tile: every tap, or every second one from the class's first (without a
  // branch, so that the decodes of one k-step's in_row and wtap calls fold into one)
  const int ts = cm ? 2 : 1, tny = cm ? pc.nty : k, tnx = cm ? pc.ntx : k;
  auto tap3 = [&](int j, int &dz, int &dy, int &dx) {
    dz = pc.tz0 + ts * (j / (tny * tnx)); dy = pc.ty0 + ts * ((j / tnx) % tny); dx = pc.tx0 + ts * (j % tnx);
  };
  auto in_row = [&](int h, int, int j) -> int64_t {
    int dz, dy, dx;
    tap3(j, dz, dy, dx);
    return rv[h] ? in_voxel(g, vb[h], vz[h], vy[h], vx[h], dz, dy, dx) : -1;
  };
  auto wtap = [&](int j) {
    int dz, dy, dx;
    tap3(j, dz, dy, dx);
    return (dz * k + dy) * k + dx;
  };
  f32x4 acc[BMT / 32][BNT / 32];
  gather_gemm_tile<BMT, KST, BNT, Rows1>(X, g.Cin, W, taps, n0, cm ? pc.ntz * pc.nty * pc.ntx : taps, in_row, wtap, acc);
  auto out_row = [&](int r) -> int64_t {
    const int64_t uo = m0 + r;
    if (uo >= Mrows) return -1;
    if (!cm) return uo;
    int ob, oz, oy, ox;   // class row -> output voxel
    decode_class(pc, uo, ob, oz, oy, ox);
    return (((int64_t)ob * g.Do + oz) * g.Ho + oy) * g.Wo + ox;
  };
  store_tile<BMT, BNT, OUT_BF16>(acc, out_row, n0, g.Cout, bias, Y, ep...);
}

// ---- 3x3x3 stride-1 stencil (both forms) with the input block's halo staged in LDS once per
// CS-channel slice (CS = 64, or 32 for a 32-channel level): a 4 x 4 x 8 block of output voxels
// reads its 6 x 6 x 10 input halo (360 voxel rows) from L2 once and every tap's A operand from
// LDS at a shifted row, instead of 27 gathers; the 27 taps' NT x CS weight tiles (NT = 64 or 32
// output channels) stream through a double buffer.  The LDS images keep 128-B rows whatever CS
// (a 32-channel slice fills the first four swizzled slots of a row).  X: Rows1, or Rows2 (the
// two-source forward pcs_conv3d_cat: the halo staging picks the source per 16-byte chunk); Y: Out1,
// or Out2 (its input gradient, the transposed form writing dXA | dXB per 4-channel store group).
constexpr int SZ = 4, SY = 4, SX = 8;                      // output block: 128 voxels
constexpr int GZ = SZ + 2, GY = SY + 2, GX = SX + 2;
constexpr int HROWS = GZ * GY * GX;                        // 360 halo voxels
constexpr int HIMG = HROWS * 128, WTILE = 64 * 128;        // halo image (64 ch), one tap's W tile

PCS_DEV int swz8(int row, int ch) { return ch ^ ((row >> 1) & 7); }

template <int CS, int NT, bool OUT_BF16, class XF = Rows1, class YF = Out1, class... EP>
__global__ __launch_bounds__(THREADS) void stencil3_kernel(pcs_conv3d_geom g, typename XF::Arg X,
                                                           const bf16_t *__restrict__ W, const float *__restrict__ bias,
                                                           typename YF::Arg Y, EP... epp) {
  static_assert(sizeof...(EP) == 0 || !YF::SPLIT, "the affine epilogue writes one array");
  __shared__ __attribute__((aligned(16))) char lds[HIMG + 2 * WTILE];   // 45 KB + 16 KB
  char *halo = lds, *wt = lds + HIMG;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1, lr = lane & 15, lg = lane >> 4;
  const int nbx = (g.Wo + SX - 1) / SX, nby = (g.Ho + SY - 1) / SY, nbz = (g.Do + SZ - 1) / SZ;
  uint32_t bid = blockIdx.x;
  const int bx = (int)(bid % nbx); bid /= nbx;
  const int by = (int)(bid % nby); bid /= nby;
  const int bz = (int)(bid % nbz);
  const int b = (int)(bid / nbz);
  const int oz0 = bz * SZ, oy0 = by * SY, ox0 = bx * SX;
  const bool tr = g.transposed;
  // first halo voxel: conv reads o - p + t, the transposed form o + p - t (t = 0..2)
  const int hz0 = tr ? oz0 + g.p - 2 : oz0 - g.p, hy0 = tr ? oy0 + g.p - 2 : oy0 - g.p,
            hx0 = tr ? ox0 + g.p - 2 : ox0 - g.p;
  constexpr int CCH = CS / 8;                 // 16-B chunks per staged row
  constexpr int WCH = NT * CCH;               // W tile chunks
  constexpr int HW = (WCH + THREADS - 1) / THREADS;
  constexpr int TJ = NT / 32, KK = CS / 32;
  const int n0 = blockIdx.y * NT, Cin = g.Cin, cps = Cin / CS;
  // wave tile: output rows wr*64 .. +64 (4 MFMA tiles), channels wc*NT/2 ..; row r = (rz, ry, rx)
  int hrow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = wr * 64 + i * 16 + lr;
    hrow[i] = ((r >> 5) * GY + ((r >> 3) & 3)) * GX + (r & 7);
  }
  u32x4 rw[HW];   // W staging: NT rows x CCH chunks
  auto loadw = [&](int t, int c0) {
#pragma unroll
    for (int h = 0; h < HW; ++h) {
      const int c = tid + THREADS * h, row = c / CCH, ch = c % CCH;
      if (c < WCH) rw[h] = *reinterpret_cast<const u32x4 *>(W + ((int64_t)(n0 + row) * 27 + t) * Cin + c0 + ch * 8);
    }
  };
  auto stagew = [&](int buf) {
#pragma unroll
    for (int h = 0; h < HW; ++h) {
      const int c = tid + THREADS * h, row = c / CCH, ch = c % CCH;
      if (c < WCH) *reinterpret_cast<u32x4 *>(wt + buf * WTILE + row * 128 + swz8(row, ch) * 16) = rw[h];
    }
  };
  f32x4 acc[4][TJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int cs = 0; cs < cps; ++cs) {
    const int c0 = cs * CS;
    __syncthreads();   // the previous slice's halo and W reads are done
    for (int c = tid; c < HROWS * CCH; c += THREADS) {
      const int hr = c / CCH, ch = c % CCH;
      const int hx = hr % GX, hy = (hr / GX) % GY, hz = hr / (GX * GY);
      const int iz = hz0 + hz, iy = hy0 + hy, ix = hx0 + hx;
      u32x4 v = mk_u32x4(0, 0, 0, 0);
      if (iz >= 0 && iy >= 0 && ix >= 0 && iz < g.Di && iy < g.Hi && ix < g.Wi)
        v = *reinterpret_cast<const u32x4 *>(XF::at(X, (((int64_t)b * g.Di + iz) * g.Hi + iy) * g.Wi + ix, Cin, c0 + ch * 8));
      *reinterpret_cast<u32x4 *>(halo + hr * 128 + swz8(hr, ch) * 16) = v;
    }
    loadw(0, c0);
    stagew(0);
    __syncthreads();
    for (int t = 0; t < 27; ++t) {
      const int buf = t & 1;
      if (t + 1 < 27) loadw(t + 1, c0);
      const int dz = t / 9, dy = (t / 3) % 3, dx = t % 3;
      const int hoff = tr ? ((2 - dz) * GY + (2 - dy)) * GX + (2 - dx) : (dz * GY + dy) * GX + dx;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        bf16x8 af[4], bw[TJ];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int h = hrow[i] + hoff;
          af[i] = *reinterpret_cast<const bf16x8 *>(halo + h * 128 + swz8(h, kk * 4 + lg) * 16);
        }
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          const int r = wc * (NT / 2) + j * 16 + lr;
          bw[j] = *reinterpret_cast<const bf16x8 *>(wt + buf * WTILE + r * 128 + swz8(r, kk * 4 + lg) * 16);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[j], af[i], acc[i][j], 0, 0, 0);
      }
      if (t + 1 < 27) stagew(buf ^ 1);   // buf ^ 1 was last read before the previous barrier
      __syncthreads();
    }
  }
  const auto ep = epi_of(epp...);
  decltype(epi_coef<4>(ep, 0)) ek[TJ];
  if constexpr (sizeof...(EP) != 0) {
#pragma unroll
    for (int j = 0; j < TJ; ++j) ek[j] = epi_coef<4>(ep, n0 + wc * (NT / 2) + j * 16 + 4 * lg);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = wr * 64 + i * 16 + lr;
    const int oz = oz0 + (r >> 5), oy = oy0 + ((r >> 3) & 3), ox = ox0 + (r & 7);
    if (oz >= g.Do || oy >= g.Ho || ox >= g.Wo) continue;
    const int64_t uo = (((int64_t)b * g.Do + oz) * g.Ho + oy) * g.Wo + ox;
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int co = n0 + wc * (NT / 2) + j * 16 + 4 * lg;
      float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      if (bias) {
        const float4 bb = *reinterpret_cast<const float4 *>(bias + co);
        v[0] += bb.x; v[1] += bb.y; v[2] += bb.z; v[3] += bb.w;
      }
      int cy = co, ld = g.Cout;
      void *y = YF::pick(Y, cy, ld);
      if constexpr (sizeof...(EP) != 0) epi_apply<OUT_BF16>(ep, ek[j], uo * ld + cy, v);
      if constexpr (OUT_BF16) {
        *reinterpret_cast<uint2 *>(reinterpret_cast<bf16_t *>(y) + uo * ld + cy) =
            make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
      } else {
        *reinterpret_cast<float4 *>(reinterpret_cast<float *>(y) + uo * ld + cy) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  }
}

// ---- weight gradient: dW[co][t][ci] = sum_o dY[o][co] X[in(o, t)][ci], one (co, ci) 64x64 tile
// of one tap per workgroup and voxel slice.  Both operands are staged row-major ([32 voxels][64
// channels], whole 128-B rows, double-buffered) and read as MFMA operands with k over voxels by
// ds_read_b64_tr_b16 (4 voxels x 16 channels per 16-lane group, delivered column-major)
constexpr int WV = 32;   // voxels per k-step
constexpr int WIMG = WV * 128;   // one [32][64] bf16 image

// 16-B chunk swizzle of image row r (even values: a 32-B pair of chunks stays adjacent): the
// eight rows a 32-lane half reads (8g + 4h + q, two groups) land on distinct 32-B bank slots
PCS_DEV int wsw(int r) { return 2 * (((r >> 1) & 1) | ((r >> 2) & 2)); }
PCS_DEV int woff(int r, int byte) { return r * 128 + ((((byte >> 4) ^ wsw(r)) << 4) | (byte & 15)); }

// MFMA operand rows = channels cb .. cb+15 (lane & 15), k = voxels 8 (lane >> 4) .. + 8
PCS_DEV bf16x8 wfrag(const char *img, int cb, int lane) {
  const int g = lane >> 4, i = lane & 15;
  const int byte = (cb + 4 * (i & 3)) * 2;   // this lane supplies row 8g (+4) + i/4, columns cb + 4 (i%4)
  return tr_frag2(img + woff(8 * g + (i >> 2), byte), img + woff(8 * g + 4 + (i >> 2), byte));
}

// One workgroup covers the dx taps of one (dz, dy) (all k of them, sharing the dY image; one tap
// in class mode, where the dx taps meet different voxel sets)
constexpr int TG = 3;

// The k-over-voxels loop of every weight-gradient kernel here (conv3d_wgrad_kernel,
// sparse_wgrad_kernel, pair_wgrad_kernel): acc[a] += dY^T X_a over nks k-steps of WV voxels for the
// first ntg (uniform, <= NT) of NT X images that share one dY image.  load_rows(ks, rd, rx) fills
// this thread's 16-B chunks (voxel row tid >> 3 of k-step ks, channels 8 (tid & 7) ..) of dY and of
// the X images; they arrive zeroed, so a row or tap without a voxel is left alone.  COT x CIT = the
// workgroup's (co, ci) tile, 64 or 32 each (a 32-channel level stages half rows).  The next k-step's
// rows are loaded into registers while this one's MFMAs run.
template <int COT, int CIT, int NT, class LoadF>
PCS_DEV void wgrad_tile(LoadF load_rows, int nks, int ntg, f32x4 (&acc_out)[NT][COT / 32][CIT / 32]) {
  __shared__ __attribute__((aligned(16))) char lds[2][(1 + NT) * WIMG];   // per buffer: dY | X per image
  constexpr int NI = COT / 32, NJ = CIT / 32;   // 16-channel MFMA tiles per wave (co, ci)
  // the loop accumulates in locals and hands them over once: accumulating through the reference
  // left the compiler with two copies of every accumulator (30 more VGPRs, a wave less per SIMD)
  f32x4 acc[NT][NI][NJ];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int sv = tid >> 3, q8 = tid & 7;   // staging: voxel row sv, 16-B chunk q8
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[a][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x4 rd, rx[NT];
  auto load = [&](int ks) {
    rd = mk_u32x4(0, 0, 0, 0);
#pragma unroll
    for (int a = 0; a < NT; ++a) rx[a] = mk_u32x4(0, 0, 0, 0);
    load_rows(ks, rd, rx);
  };
  auto stage = [&](int buf) {
    *reinterpret_cast<u32x4 *>(lds[buf] + woff(sv, q8 * 16)) = rd;
#pragma unroll
    for (int a = 0; a < NT; ++a)
      if (a < ntg) *reinterpret_cast<u32x4 *>(lds[buf] + (1 + a) * WIMG + woff(sv, q8 * 16)) = rx[a];
  };
  if (nks > 0) {
    load(0);
    stage(0);
  }
  __syncthreads();
  for (int ks = 0; ks < nks; ++ks) {
    const int buf = ks & 1;
    if (ks + 1 < nks) load(ks + 1);
    bf16x8 fd[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) fd[i] = wfrag(lds[buf], wr * (COT / 2) + i * 16, lane);
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      if (a < ntg) {   // uniform
        bf16x8 fx[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) fx[j] = wfrag(lds[buf] + (1 + a) * WIMG, wc * (CIT / 2) + j * 16, lane);
        // lane: dW rows co = 4 lg + v of tile i, column ci = lr of tile j
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            acc[a][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd[i], fx[j], acc[a][i][j], 0, 0, 0);
      }
    }
    if (ks + 1 < nks) stage(buf ^ 1);   // buf ^ 1 was last read before the previous barrier
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc_out[a][i][j] = acc[a][i][j];
}

// one image's accumulators of wgrad_tile, the (co0, ci0) tile of tap t -> out[co][t][ci]
template <int COT, int CIT>
PCS_DEV void store_wgrad_tile(const f32x4 (&acc)[COT / 32][CIT / 32], float *__restrict__ out, int co0, int taps, int t,
                              int ci0, int Cin) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wr = wid >> 1, wc = wid & 1, lr = lane & 15, lg = lane >> 4;
#pragma unroll
  for (int i = 0; i < COT / 32; ++i)
#pragma unroll
    for (int j = 0; j < CIT / 32; ++j) {
      const int ci = ci0 + wc * (CIT / 2) + j * 16 + lr;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int co = co0 + wr * (COT / 2) + i * 16 + 4 * lg + v;
        out[((int64_t)co * taps + t) * Cin + ci] = acc[i][j][v];
      }
    }
}

template <int COT, int CIT>
__global__ __launch_bounds__(THREADS) void conv3d_wgrad_kernel(pcs_conv3d_geom g, const bf16_t *__restrict__ X,
                                                               const bf16_t *__restrict__ dY, float *__restrict__ ws,
                                                               int64_t M, int64_t vps) {
  const int nco = g.Cout / COT;
  const int co0 = (blockIdx.x % nco) * COT, ci0 = (blockIdx.x / nco) * CIT;
  const int split = blockIdx.z;
  const int k = g.k, taps = k * k * k;
  // transposed, stride 2: tap t only meets the output voxels of parity class (t + p) mod 2, so
  // the slices run over that class's sub-grid, one tap per workgroup
  const bool cm = g.transposed && g.s == 2;
  int dz, dy, dx0, ntg;
  if (cm) {
    const int t = blockIdx.y;
    dz = t / (k * k); dy = (t / k) % k; dx0 = t % k; ntg = 1;
  } else {
    dz = blockIdx.y / k; dy = blockIdx.y % k; dx0 = 0; ntg = k;
  }
  PClass pc{};
  int64_t Mv = M, vs = vps;
  if (cm) {
    pc = pclass(g, (((dz + g.p) & 1) << 2) | (((dy + g.p) & 1) << 1) | ((dx0 + g.p) & 1));
    Mv = g.B * pc.nz * pc.ny * pc.nx;
    vs = ((Mv + gridDim.z - 1) / gridDim.z + WV - 1) / WV * WV;
  }
  const int64_t lo = (int64_t)split * vs, hi = pcs_min64(lo + vs, Mv);
  const int sv = threadIdx.x >> 3, q8 = threadIdx.x & 7;
  auto load_rows = [&](int ks, u32x4 &rd, u32x4 (&rx)[TG]) {
    const int64_t u = lo + (int64_t)ks * WV + sv;
    if (u >= hi) return;
    int b, z, y, x;
    int64_t uo = u;
    if (cm) {
      decode_class(pc, u, b, z, y, x);
      uo = (((int64_t)b * g.Do + z) * g.Ho + y) * g.Wo + x;
    } else {
      decode(g, u, b, z, y, x);
    }
    if (q8 < COT / 8) rd = *reinterpret_cast<const u32x4 *>(dY + uo * g.Cout + co0 + q8 * 8);
#pragma unroll
    for (int a = 0; a < TG; ++a) {
      if (a < ntg) {
        const int64_t iv = in_voxel(g, b, z, y, x, dz, dy, dx0 + a);
        if (iv >= 0 && q8 < CIT / 8) rx[a] = *reinterpret_cast<const u32x4 *>(X + iv * g.Cin + ci0 + q8 * 8);
      }
    }
  };
  f32x4 acc[TG][COT / 32][CIT / 32];
  wgrad_tile<COT, CIT, TG>(load_rows, (int)((hi - lo + WV - 1) / WV), ntg, acc);   // (uniform; 0 k-steps for an empty slice)
  float *out = ws + (int64_t)split * g.Cout * taps * g.Cin;
#pragma unroll
  for (int a = 0; a < TG; ++a) {
    if (a >= ntg) continue;
    store_wgrad_tile<COT, CIT>(acc[a], out, co0, taps, (dz * k + dy) * k + dx0 + a, ci0, g.Cin);
  }
}

// ---- weight gradient of the 3x3x3 stride-1 stencil (both forms) on halo tiles: a workgroup owns
// one (64 co x 64 ci) tile and one dz (9 taps, 144 accumulator VGPRs) and walks a range of 4 x 4 x 8
// output blocks; per block it stages the block's dY rows [128][64] and the 4 input planes of the
// halo it meets at this dz [4][6][10][64] once, and every tap's operand is a shifted set of halo
// rows read transposed (k over the block's voxels).  X: Rows1 or Rows2 (per 16-byte chunk, as above)
constexpr int XPL = SZ * GY * GX;   // 240 halo rows of one dz

template <int COT, int CIT, class XF = Rows1>   // the (co, ci) tile: 64 or 32 each
__global__ __launch_bounds__(THREADS) void stencil3_wgrad_kernel(pcs_conv3d_geom g, typename XF::Arg X,
                                                                 const bf16_t *__restrict__ dY, float *__restrict__ ws,
                                                                 int64_t nblk, int64_t bps) {
  __shared__ __attribute__((aligned(16))) char lds[(128 + XPL) * 128];   // dY image | halo planes (46 KB)
  char *dimg = lds, *ximg = lds + 128 * 128;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1, lr = lane & 15, lg = lane >> 4;
  constexpr int NI = COT / 32, NJ = CIT / 32;   // 16-channel MFMA tiles per wave (co, ci)
  const int nco = g.Cout / COT;
  const int co0 = (blockIdx.x % nco) * COT, ci0 = (blockIdx.x / nco) * CIT;
  const int dz = blockIdx.y, split = blockIdx.z;
  const bool tr = g.transposed;
  const int zoff = tr ? 2 - dz : dz;
  const int nbx = (g.Wo + SX - 1) / SX, nby = (g.Ho + SY - 1) / SY, nbz = (g.Do + SZ - 1) / SZ;
  const int64_t b0 = (int64_t)split * bps, b1 = pcs_min64(b0 + bps, nblk);
  // transposed operand read: rows = 16 channels from cb (lane & 15), k = 8 voxels from 8 (lane >> 4)
  // (4 per ds_read_b64_tr_b16); row_of(k) gives the image row of block voxel k
  auto trfrag = [&](const char *img, int cb, int kb, int dyo, int dxo, bool halo) {
    const int gq = lane >> 4, i = lane & 15;
    const int byte = (cb + 4 * (i & 3)) * 2;
    s16x4 part[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = kb + 8 * gq + 4 * h + (i >> 2);   // block voxel
      const int row = halo ? (((r >> 5) * GY + ((r >> 3) & 3) + dyo) * GX + (r & 7) + dxo) : r;
      part[h] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_s16x4 *)(img + row * 128 + ((((byte >> 4) ^ ((row >> 1) & 7)) << 4) | (byte & 15))));
    }
    const s16x8 v = {part[0][0], part[0][1], part[0][2], part[0][3], part[1][0], part[1][1], part[1][2], part[1][3]};
    return __builtin_bit_cast(bf16x8, v);
  };
  f32x4 acc[9][NI][NJ];
#pragma unroll
  for (int a = 0; a < 9; ++a)
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[a][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t blk = b0; blk < b1; ++blk) {
    uint32_t q = (uint32_t)blk;
    const int bx = (int)(q % nbx); q /= nbx;
    const int by = (int)(q % nby); q /= nby;
    const int bz = (int)(q % nbz);
    const int b = (int)(q / nbz);
    const int oz0 = bz * SZ, oy0 = by * SY, ox0 = bx * SX;
    const int hz0 = (tr ? oz0 + g.p - 2 : oz0 - g.p) + zoff, hy0 = tr ? oy0 + g.p - 2 : oy0 - g.p,
              hx0 = tr ? ox0 + g.p - 2 : ox0 - g.p;
    __syncthreads();   // the previous block's reads are done
    for (int c = tid; c < 128 * (COT / 8); c += THREADS) {   // dY rows of the block (zero outside the grid)
      const int r = c / (COT / 8), ch = c % (COT / 8);
      const int oz = oz0 + (r >> 5), oy = oy0 + ((r >> 3) & 3), ox = ox0 + (r & 7);
      u32x4 v = mk_u32x4(0, 0, 0, 0);
      if (oz < g.Do && oy < g.Ho && ox < g.Wo)
        v = *reinterpret_cast<const u32x4 *>(dY + ((((int64_t)b * g.Do + oz) * g.Ho + oy) * g.Wo + ox) * g.Cout + co0 + ch * 8);
      *reinterpret_cast<u32x4 *>(dimg + r * 128 + ((ch ^ ((r >> 1) & 7)) << 4)) = v;
    }
    for (int c = tid; c < XPL * (CIT / 8); c += THREADS) {   // the 4 halo planes of this dz
      const int hr = c / (CIT / 8), ch = c % (CIT / 8);
      const int hx = hr % GX, hy = (hr / GX) % GY, hz = hr / (GX * GY);
      const int iz = hz0 + hz, iy = hy0 + hy, ix = hx0 + hx;
      u32x4 v = mk_u32x4(0, 0, 0, 0);
      if (iz >= 0 && iy >= 0 && ix >= 0 && iz < g.Di && iy < g.Hi && ix < g.Wi)
        v = *reinterpret_cast<const u32x4 *>(XF::at(X, (((int64_t)b * g.Di + iz) * g.Hi + iy) * g.Wi + ix, g.Cin, ci0 + ch * 8));
      *reinterpret_cast<u32x4 *>(ximg + hr * 128 + ((ch ^ ((hr >> 1) & 7)) << 4)) = v;
    }
    __syncthreads();
#pragma unroll 1
    for (int kb = 0; kb < 128; kb += 32) {   // 32 block voxels per MFMA k-step
      bf16x8 fd[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) fd[i] = trfrag(dimg, wr * (COT / 2) + i * 16, kb, 0, 0, false);
#pragma unroll
      for (int a = 0; a < 9; ++a) {
        const int ty = a / 3, tx = a % 3;
        const int dyo = tr ? 2 - ty : ty, dxo = tr ? 2 - tx : tx;
        bf16x8 fx[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) fx[j] = trfrag(ximg, wc * (CIT / 2) + j * 16, kb, dyo, dxo, true);
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            acc[a][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd[i], fx[j], acc[a][i][j], 0, 0, 0);
      }
    }
  }
  float *out = ws + (int64_t)split * g.Cout * 27 * g.Cin;
#pragma unroll
  for (int a = 0; a < 9; ++a) {
    const int t = dz * 9 + a;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int ci = ci0 + wc * (CIT / 2) + j * 16 + lr;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int co = co0 + wr * (COT / 2) + i * 16 + 4 * lg + v;
          out[((int64_t)co * 27 + t) * g.Cin + ci] = acc[a][i][j][v];
        }
      }
  }
}

// db partials: column sums of dY over one voxel slice, [split][Cout]; a thread sums 8 channels
// (one 16-B chunk) of every 32nd row, then the 32 row groups are added in LDS in a fixed order
// (64 channels per workgroup; the last one of a 32-channel multiple runs half)
__global__ __launch_bounds__(THREADS) void conv3d_bgrad_kernel(const bf16_t *__restrict__ dY, int Cout, int64_t M,
                                                               int64_t vps, float *__restrict__ wsb) {
  __shared__ float red[32][64];
  const int ch = threadIdx.x & 7, rg = threadIdx.x >> 3;   // channels c0 + 8 ch .., row group 0..31
  const int c0 = blockIdx.x * 64;
  const int64_t lo = (int64_t)blockIdx.y * vps, hi = pcs_min64(lo + vps, M);
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool cv = c0 + ch * 8 < Cout;
  for (int64_t u = cv ? lo + rg : hi; u < hi; u += 32) {
    float v[8];
    unpack_chunk(*reinterpret_cast<const u32x4 *>(dY + u * Cout + c0 + ch * 8), v);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] += v[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[rg][ch * 8 + e] = s[e];
  __syncthreads();
  if (threadIdx.x < 64 && c0 + (int)threadIdx.x < Cout) {
    float t = 0.f;
    for (int r = 0; r < 32; ++r) t += red[r][threadIdx.x];
    wsb[(int64_t)blockIdx.y * Cout + c0 + threadIdx.x] = t;
  }
}

// out[i] = sum_s part[s * len + i], fixed order
__global__ __launch_bounds__(256) void conv3d_reduce_kernel(const float *__restrict__ part, int64_t nsl, int64_t len,
                                                            float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  float s = 0.f;
  for (int64_t sl = 0; sl < nsl; ++sl) s += part[sl * len + i];
  out[i] = s;
}

__global__ __launch_bounds__(256) void conv3d_weight_t_kernel(const bf16_t *__restrict__ W, int Cout, int taps, int Cin,
                                                              bf16_t *__restrict__ Wt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // index into Wt [Cin][taps][Cout]
  const int64_t n = (int64_t)Cout * taps * Cin;
  if (i >= n) return;
  const int co = (int)(i % Cout);
  const int64_t r = i / Cout;
  const int t = (int)(r % taps), ci = (int)(r / taps);
  Wt[i] = W[((int64_t)co * taps + t) * Cin + ci];
}

// ---- submanifold sparse convolution on occupied voxels (the north star's hash-indexed gather,
// BASELINE configs[2]): the rows are the occupied voxels, the input row of (row m, tap t) comes
// from the neighbour map nbr[m][t] (-1: an empty site, zeros) built by pcs_sparse_neighbors.  The
// same gather GEMM as conv3d_kernel; a tile runs only the taps some of its rows have a neighbour
// at (a bit mask collected in LDS first), which is where the sparsity saves MFMA work.
//   Y[m] = b + sum_t W[tw(t)] X[nbr[m][t]],  tw(t) = flip ? taps - 1 - t : t
// With flip and W^T (pcs_conv3d_weight_t) this is the input gradient: offset(taps-1-t) =
// -offset(t) for the centred 3x3x3 taps, so dX[n] = sum_t W_t^T dY[nbr[n][taps-1-t]].
// X: Rows1 or Rows2 (the two-source forward), Y: Out1 or Out2 (its input gradient to both sources).
template <int BMT, int KST, bool OUT_BF16, class XF = Rows1, class YF = Out1, class... EP>
__global__ __launch_bounds__(THREADS) void sparse_conv_kernel(const int32_t *__restrict__ nbr, int64_t M, int taps,
                                                              typename XF::Arg X, int Cin,
                                                              const bf16_t *__restrict__ W, int Cout,
                                                              const float *__restrict__ bias, typename YF::Arg Y,
                                                              int flip, EP... ep) {
  static_assert(sizeof...(EP) == 0 || !YF::SPLIT, "the affine epilogue writes one array");
  __shared__ uint32_t tmask;
  __shared__ int tlist[32];
  __shared__ int ntl;
  const int tid = threadIdx.x;
  const int64_t m0 = (int64_t)blockIdx.x * BMT;

  // the taps this tile meets
  if (tid == 0) tmask = 0u;
  __syncthreads();
  uint32_t mym = 0u;
  for (int i = tid; i < BMT * taps; i += THREADS) {
    const int r = i / taps, t = i - r * taps;
    if (m0 + r < M && nbr[(m0 + r) * taps + t] >= 0) mym |= 1u << t;
  }
  if (mym) atomicOr(&tmask, mym);
  __syncthreads();
  if (tid == 0) {
    int c = 0;
    const uint32_t m = tmask;
    for (int t = 0; t < taps; ++t)
      if ((m >> t) & 1u) tlist[c++] = t;
    ntl = c;
  }
  __syncthreads();
  auto in_row = [&](int, int r, int j) { return m0 + r < M ? nbr[(m0 + r) * taps + tlist[j]] : -1; };
  auto wtap = [&](int j) { return flip ? taps - 1 - tlist[j] : tlist[j]; };
  f32x4 acc[BMT / 32][2];
  const int n0 = blockIdx.y * BN;
  gather_gemm_tile<BMT, KST, BN, XF>(X, Cin, W, taps, n0, ntl, in_row, wtap, acc);
  int c0 = n0, ld = Cout;
  void *y = YF::pick(Y, c0, ld);
  if constexpr (YF::SPLIT) bias = bias ? bias + (n0 - c0) : nullptr;   // store_tile adds bias[c0 + ..]
  store_tile<BMT, BN, OUT_BF16>(acc, [&](int r) { return m0 + r < M ? m0 + r : -1; }, c0, ld, bias, y, ep...);
}

// weight gradient of the sparse convolution: dW[co][t][ci] = sum_m dY[m][co] X[nbr[m][t]][ci];
// a workgroup owns a (64 co x 64 ci) tile, TG consecutive taps and a slice of rows (the
// structure of conv3d_wgrad_kernel with the neighbour map as the index), partials per slice
// (X: Rows1 or Rows2; the workgroup's ci0 tile selects the source)
template <class XF = Rows1>
__global__ __launch_bounds__(THREADS) void sparse_wgrad_kernel(const int32_t *__restrict__ nbr, int64_t M, int taps,
                                                               typename XF::Arg X, int Cin,
                                                               const bf16_t *__restrict__ dY, int Cout,
                                                               float *__restrict__ ws, int64_t vps) {
  const int nco = Cout / 64;
  const int co0 = (blockIdx.x % nco) * 64, ci0 = (blockIdx.x / nco) * 64;
  const int t0 = blockIdx.y * TG, ntg = min(TG, taps - t0);
  const int64_t lo = (int64_t)blockIdx.z * vps, hi = pcs_min64(lo + vps, M);
  const int sv = threadIdx.x >> 3, q8 = threadIdx.x & 7;
  auto load_rows = [&](int ks, u32x4 &rd, u32x4 (&rx)[TG]) {
    const int64_t u = lo + (int64_t)ks * WV + sv;
    if (u >= hi) return;
    rd = *reinterpret_cast<const u32x4 *>(dY + u * Cout + co0 + q8 * 8);
#pragma unroll
    for (int a = 0; a < TG; ++a) {
      if (a < ntg) {
        const int iv = nbr[u * taps + t0 + a];
        if (iv >= 0) rx[a] = *reinterpret_cast<const u32x4 *>(XF::at(X, iv, Cin, ci0) + q8 * 8);
      }
    }
  };
  f32x4 acc[TG][2][2];
  wgrad_tile<64, 64, TG>(load_rows, (int)((hi - lo + WV - 1) / WV), ntg, acc);
  float *out = ws + (int64_t)blockIdx.z * Cout * taps * Cin;
#pragma unroll
  for (int a = 0; a < TG; ++a) {
    if (a >= ntg) continue;
    store_wgrad_tile<64, 64>(acc[a], out, co0, taps, t0 + a, ci0, Cin);
  }
}

int64_t sparse_wgrad_splits(int64_t M, int taps, int Cin, int Cout) {
  const int64_t tiles = (int64_t)(Cout / 64) * (Cin / 64) * ((taps + TG - 1) / TG);
  int64_t sp = (2048 + tiles - 1) / tiles;
  const int64_t maxsp = (M + 4 * WV - 1) / (4 * WV);
  if (sp > maxsp) sp = maxsp;
  return sp < 1 ? 1 : sp;
}

bool geom_ok(const pcs_conv3d_geom *g, const char **why) {
  if (!g) { *why = "null geometry"; return false; }
  if (g->B <= 0 || g->Di <= 0 || g->Hi <= 0 || g->Wi <= 0 || g->Do <= 0 || g->Ho <= 0 || g->Wo <= 0) {
    *why = "empty grid";
    return false;
  }
  if (g->k < 1 || g->k > 3 || (g->s != 1 && g->s != 2) || g->p < 0 || g->p >= g->k || (g->transposed != 0 && g->transposed != 1)) {
    *why = "k in 1..3, s in {1, 2}, 0 <= p < k, transposed 0 or 1";
    return false;
  }
  const int din[3] = {g->Di, g->Hi, g->Wi}, dout[3] = {g->Do, g->Ho, g->Wo};
  for (int d = 0; d < 3; ++d) {
    // transposed: + output_padding in [0, s) (torch's; the extra planes are plain gather rows)
    const int expect = g->transposed ? (din[d] - 1) * g->s - 2 * g->p + g->k : (din[d] + 2 * g->p - g->k) / g->s + 1;
    const int slack = g->transposed ? g->s - 1 : 0;
    if (dout[d] < expect || dout[d] > expect + slack || (!g->transposed && din[d] + 2 * g->p < g->k)) {
      *why = "output grid must be (in + 2p - k)/s + 1 (conv) or (in - 1)s - 2p + k + op, 0 <= op < s (transposed)";
      return false;
    }
  }
  if (g->B * g->Di * g->Hi * g->Wi >= ((int64_t)1 << 40) || g->B * g->Do * g->Ho * g->Wo >= ((int64_t)1 << 40)) {
    *why = "grid too large";
    return false;
  }
  return true;
}

int64_t out_voxels(const pcs_conv3d_geom &g) { return g.B * g.Do * g.Ho * g.Wo; }

bool stencil3(const pcs_conv3d_geom &g) { return g.k == 3 && g.s == 1; }
// channel tile of a layer: 64, or 32 where the count is an odd multiple of 32 (a 32-channel level)
int ctile(int c) { return c % 64 == 0 ? 64 : 32; }

int64_t stencil_blocks(const pcs_conv3d_geom &g) {
  return g.B * ((g.Do + SZ - 1) / SZ) * ((g.Ho + SY - 1) / SY) * ((g.Wo + SX - 1) / SX);
}

int64_t wgrad_splits(const pcs_conv3d_geom &g) {
  const int64_t M = out_voxels(g);
  if (stencil3(g)) {   // halo-tile kernel: 3 dz workgroups per (co, ci) tile and block range
    const int64_t tiles = (int64_t)(g.Cout / ctile(g.Cout)) * (g.Cin / ctile(g.Cin)) * 3;
    const int64_t sp = (1024 + tiles - 1) / tiles, nb = stencil_blocks(g);
    return sp > nb ? nb : sp;
  }
  const int64_t tiles = (int64_t)(g.Cout / ctile(g.Cout)) * (g.Cin / ctile(g.Cin)) *
                        (g.transposed && g.s == 2 ? g.k * g.k * g.k : g.k * g.k);
  int64_t sp = (2048 + tiles - 1) / tiles;
  const int64_t maxsp = (M + 4 * WV - 1) / (4 * WV);   // at least 4 k-steps per slice
  if (sp > maxsp) sp = maxsp;
  return sp < 1 ? 1 : sp;
}

int64_t wgrad_vps(const pcs_conv3d_geom &g, int64_t sp) {
  const int64_t M = out_voxels(g);
  return ((M + sp - 1) / sp + WV - 1) / WV * WV;
}

// ---- per-tap pair lists of a neighbour map: the sparse convolution as gather-GEMM-reduce.  The
// gather kernel above multiplies a zero row for every row of a tile that lacks a tap the tile
// meets; at low occupancy (1.5 occupied taps per voxel) that is most of its work.  Here each tap's
// (out row, in row) pairs are listed once per neighbour map (rows ascending within a tap, so the
// lists and every sum below are deterministic), the product of tap t is a GEMM over its own pairs
// only, and each output row sums its pairs' products in tap order.
constexpr int PT_MAX = 27;   // taps of the centred 3x3x3 map
struct PairTaps {            // host-built, passed by value: tap t's pairs [tap_off[t], tap_off[t + 1]),
  int64_t tap_off[PT_MAX + 1];   // its GEMM tiles [tile_off[t], tile_off[t + 1]), its weight-gradient
  int32_t tile_off[PT_MAX + 1];  // slices [slice_off[t], slice_off[t + 1]) of slice_len pairs each
  int32_t slice_off[PT_MAX + 1];
  int64_t slice_len;
  int32_t taps;
};

// a block's 256 rows of the neighbour map through LDS: coalesced loads (and, for pair_pos,
// coalesced stores) instead of 27 strided accesses per thread; [row][tap] words, stride 27 (odd:
// the per-tap reads are conflict-free)
PCS_DEV int pairs_rows(const int32_t *__restrict__ nbr, int64_t M, int taps, int32_t *rb) {
  const int64_t r0 = (int64_t)blockIdx.x * 256;
  const int nr = (int)pcs_min64(256, M - r0), n = nr * taps;
  for (int i = threadIdx.x; i < n; i += 256) rb[i] = nbr[r0 * taps + i];
  __syncthreads();
  return nr;
}

// per-block pair counts of every tap: cnt[block][t] (one thread per row)
__global__ __launch_bounds__(256) void pairs_count_kernel(const int32_t *__restrict__ nbr, int64_t M, int taps,
                                                          int32_t *__restrict__ cnt) {
  __shared__ int32_t wc[4][PT_MAX];
  __shared__ int32_t rb[256 * PT_MAX];
  const int tid = threadIdx.x, w = tid >> 6;
  const int nr = pairs_rows(nbr, M, taps, rb);
  for (int t = 0; t < taps; ++t) {
    const bool has = tid < nr && rb[tid * taps + t] >= 0;
    const uint64_t b = __ballot(has);
    if ((tid & 63) == 0) wc[w][t] = __popcll(b);
  }
  __syncthreads();
  if (tid < taps) cnt[(int64_t)blockIdx.x * taps + tid] = wc[0][tid] + wc[1][tid] + wc[2][tid] + wc[3][tid];
}

// exclusive prefix of the block counts per tap (one workgroup per tap) and the tap totals
__global__ __launch_bounds__(256) void pairs_scan_kernel(int32_t *__restrict__ cnt, int64_t nblk, int taps,
                                                         int64_t *__restrict__ tap_counts) {
  __shared__ int32_t ws[4];
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < nblk; b0 += 256) {
    const int64_t b = b0 + tid;
    const int32_t v = b < nblk ? cnt[b * taps + t] : 0;
    int32_t x = v;   // inclusive scan of the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    if (lane == 63) ws[w] = x;
    __syncthreads();
    int32_t before = 0;
    for (int i = 0; i < w; ++i) before += ws[i];
    if (b < nblk) cnt[b * taps + t] = (int32_t)(carry + before + x - v);
    const int32_t tot = ws[0] + ws[1] + ws[2] + ws[3];
    __syncthreads();
    carry += tot;
  }
  if (tid == 0) tap_counts[t] = carry;
}

// pair_in / pair_out at tap_off[t] + (block prefix) + (rank in the block), pair_pos[m][t]:
// two ballot passes (the block's per-wave counts first, then each lane's rank)
__global__ __launch_bounds__(256) void pairs_build_kernel(const int32_t *__restrict__ nbr, int64_t M, int taps,
                                                          const int32_t *__restrict__ pre,
                                                          const int64_t *__restrict__ tap_counts,
                                                          int32_t *__restrict__ pin, int32_t *__restrict__ pout,
                                                          int32_t *__restrict__ ppos) {
  __shared__ int32_t wc[4][PT_MAX];
  __shared__ int64_t toff[PT_MAX];
  __shared__ int32_t rb[256 * PT_MAX];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t m = (int64_t)blockIdx.x * 256 + tid;
  if (tid == 0) {
    int64_t s = 0;
    for (int t = 0; t < taps; ++t) { toff[t] = s; s += tap_counts[t]; }
  }
  const int nr = pairs_rows(nbr, M, taps, rb);
  for (int t = 0; t < taps; ++t) {
    const uint64_t b = __ballot(tid < nr && rb[tid * taps + t] >= 0);
    if (lane == 0) wc[w][t] = __popcll(b);
  }
  __syncthreads();
  const uint64_t lt = (1ull << lane) - 1ull;
  for (int t = 0; t < taps; ++t) {
    const int32_t n = tid < nr ? rb[tid * taps + t] : -1;
    const uint64_t b = __ballot(n >= 0);
    int32_t q = -1;
    if (n >= 0) {
      int64_t pos = toff[t] + pre[(int64_t)blockIdx.x * taps + t] + __popcll(b & lt);
      for (int i = 0; i < w; ++i) pos += wc[i][t];
      q = (int32_t)pos;
      pin[pos] = n;
      pout[pos] = (int32_t)m;
    }
    if (tid < nr) rb[tid * taps + t] = q;   // (only this thread reads or writes its row)
  }
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * 256;
  for (int i = tid; i < nr * taps; i += 256) ppos[r0 * taps + i] = rb[i];
}

// The tile of the two pair GEMMs below: acc = W[wt] X[pair_in[p]] (gather_gemm_tile on one tap)
// for the 64 pairs [p0, pend) of tile blockIdx.x, which belongs to tap t (wt = taps - 1 - t under
// flip), and the 64 output channels from blockIdx.y * BN.
template <int KST, class XF>
PCS_DEV void pair_tile(const PairTaps &pt, const int32_t *__restrict__ pin, typename XF::Arg X, int Cin,
                       const bf16_t *__restrict__ W, int flip, f32x4 (&acc)[2][2], int64_t &p0, int64_t &pend) {
  constexpr int RPP = THREADS / (KST / 8), HA = 64 / RPP;   // gather_gemm_tile's staging passes
  const int taps = pt.taps, tile = blockIdx.x;
  int t = 0;
  while (t + 1 < taps && pt.tile_off[t + 1] <= tile) ++t;
  p0 = pt.tap_off[t] + (int64_t)(tile - pt.tile_off[t]) * 64;
  pend = pt.tap_off[t + 1];
  int iv[HA];
#pragma unroll
  for (int h = 0; h < HA; ++h) {
    const int64_t p = p0 + threadIdx.x / (KST / 8) + RPP * h;
    iv[h] = p < pend ? pin[p] : -1;
  }
  const int wt = flip ? taps - 1 - t : t;
  gather_gemm_tile<64, KST, BN, XF>(X, Cin, W, taps, blockIdx.y * BN, 1, [&](int h, int, int) { return iv[h]; },
                                [&](int) { return wt; }, acc);
}

// Z[p][n0 ..] = W[tw(t)] X[pair_in[p]] for the 64 pairs of one tile of tap t (fp32 products).
// (Reducing in the centre tap's GEMM epilogue instead of a separate pass, the centre's products
// never stored, was slower: 26 dependent gathers per lane there against 8 threads per row here.)
template <int KST, class XF = Rows1>
__global__ __launch_bounds__(THREADS) void pair_gemm_kernel(PairTaps pt, const int32_t *__restrict__ pin,
                                                            typename XF::Arg X, int Cin,
                                                            const bf16_t *__restrict__ W, int Cout, int flip,
                                                            float *__restrict__ Z) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wr = wid >> 1, wc = wid & 1, lr = lane & 15, lg = lane >> 4;
  const int n0 = blockIdx.y * BN;
  f32x4 acc[2][2];
  int64_t p0, pend;
  pair_tile<KST, XF>(pt, pin, X, Cin, W, flip, acc, p0, pend);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t p = p0 + wr * 32 + i * 16 + lr;
    if (p >= pend) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int co = n0 + wc * 32 + j * 16 + 4 * lg;
      *reinterpret_cast<f32x4 *>(Z + p * Cout + co) = acc[i][j];
    }
  }
}

// Y[m][c .. c + 7] = b + sum over taps in order of Z[pair_pos[m][t]] (one thread per 8 channels)
template <bool OUT_BF16, class YF = Out1, class... EP>
__global__ __launch_bounds__(256) void pair_reduce_kernel(const int32_t *__restrict__ ppos, int64_t M, int taps,
                                                          const float *__restrict__ Z, int Cout,
                                                          const float *__restrict__ bias, typename YF::Arg Y, EP... epp) {
  static_assert(sizeof...(EP) == 0 || !YF::SPLIT, "the affine epilogue writes one array");
  const int cpr = Cout / 8;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * cpr) return;
  const int64_t m = i / cpr;
  const int c = (int)(i - m * cpr) * 8;
  f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f}, b = f32x4{0.f, 0.f, 0.f, 0.f};
  if (bias) {
    a = *reinterpret_cast<const f32x4 *>(bias + c);
    b = *reinterpret_cast<const f32x4 *>(bias + c + 4);
  }
  for (int t = 0; t < taps; ++t) {
    const int32_t q = ppos[m * taps + t];
    if (q < 0) continue;
    a += *reinterpret_cast<const f32x4 *>(Z + (int64_t)q * Cout + c);
    b += *reinterpret_cast<const f32x4 *>(Z + (int64_t)q * Cout + c + 4);
  }
  int cy = c, ld = Cout;
  void *y = YF::pick(Y, cy, ld);
  if constexpr (sizeof...(EP) != 0) {
    const auto ep = epi_of(epp...);
    float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    epi_apply<OUT_BF16>(ep, epi_coef<8>(ep, c), m * ld + cy, v);
    a = f32x4{v[0], v[1], v[2], v[3]};
    b = f32x4{v[4], v[5], v[6], v[7]};
  }
  if constexpr (OUT_BF16) {
    *reinterpret_cast<u32x4 *>(reinterpret_cast<bf16_t *>(y) + m * ld + cy) =
        mk_u32x4(pack2bf(a[0], a[1]), pack2bf(a[2], a[3]), pack2bf(b[0], b[1]), pack2bf(b[2], b[3]));
  } else {
    *reinterpret_cast<f32x4 *>(reinterpret_cast<float *>(y) + m * ld + cy) = a;
    *reinterpret_cast<f32x4 *>(reinterpret_cast<float *>(y) + m * ld + cy + 4) = b;
  }
}

// Y[pair_out[p]] = b + W[t] X[pair_in[p]] for the 64 pairs of one tile of tap t, where every output
// row has exactly one pair (the up-convolution of a k = 2, s = 2 level, and the down-convolution's
// input gradient: a fine voxel has one parent and sits at one tap of it).  pair_gemm_kernel's
// tile with the forward epilogue scattered through pair_out: no Z, no reduce pass.
template <int KST, bool OUT_BF16, class... EP>
__global__ __launch_bounds__(THREADS) void pair_rows_kernel(PairTaps pt, const int32_t *__restrict__ pin,
                                                            const int32_t *__restrict__ pout,
                                                            const bf16_t *__restrict__ X, int Cin,
                                                            const bf16_t *__restrict__ W, int Cout,
                                                            const float *__restrict__ bias, int64_t M,
                                                            void *__restrict__ Y, EP... ep) {
  f32x4 acc[2][2];
  int64_t p0, pend;
  pair_tile<KST, Rows1>(pt, pin, X, Cin, W, 0, acc, p0, pend);
  auto out_row = [&](int r) -> int64_t {
    if (p0 + r >= pend) return -1;
    const int64_t uo = pout[p0 + r];
    return uo < M ? uo : -1;   // (negative or >= M: not a row of Y, a list that breaks the precondition)
  };
  store_tile<64, BN, OUT_BF16>(acc, out_row, blockIdx.y * BN, Cout, bias, Y, ep...);
}

// dW_t partial of one pair slice g of tap t: sum over its pairs of dY[pair_out] (x) X[pair_in] into
// ws[g][co][ci] (wgrad_tile with one X image, gathered through the pair list).  Slices are a fixed
// number of pairs, so a tap's slice count follows its pair count (the centre tap has every row)
// and every workgroup has about the same work.
template <class XF = Rows1>
__global__ __launch_bounds__(THREADS) void pair_wgrad_kernel(PairTaps pt, const int32_t *__restrict__ pin,
                                                             const int32_t *__restrict__ pout,
                                                             typename XF::Arg X, int Cin,
                                                             const bf16_t *__restrict__ dY, int Cout,
                                                             float *__restrict__ ws) {
  const int nco = Cout / 64, taps = pt.taps;
  const int co0 = (blockIdx.x % nco) * 64, ci0 = (blockIdx.x / nco) * 64;
  const int g = blockIdx.y;
  int t = 0;
  while (t + 1 < taps && pt.slice_off[t + 1] <= g) ++t;
  const int64_t cnt = pt.tap_off[t + 1] - pt.tap_off[t], s0 = (int64_t)(g - pt.slice_off[t]) * pt.slice_len;
  const int64_t lo = pt.tap_off[t] + pcs_min64(s0, cnt), hi = pt.tap_off[t] + pcs_min64(s0 + pt.slice_len, cnt);
  const int sv = threadIdx.x >> 3, q8 = threadIdx.x & 7;
  auto load_rows = [&](int ks, u32x4 &rd, u32x4 (&rx)[1]) {
    const int64_t p = lo + (int64_t)ks * WV + sv;
    if (p >= hi) return;
    rd = *reinterpret_cast<const u32x4 *>(dY + (int64_t)pout[p] * Cout + co0 + q8 * 8);
    rx[0] = *reinterpret_cast<const u32x4 *>(XF::at(X, pin[p], Cin, ci0) + q8 * 8);
  };
  f32x4 acc[1][2][2];
  wgrad_tile<64, 64, 1>(load_rows, (int)((hi - lo + WV - 1) / WV), 1, acc);   // (uniform; 0 k-steps for an empty slice)
  store_wgrad_tile<64, 64>(acc[0], ws + (int64_t)g * Cout * Cin, co0, 1, 0, ci0, Cin);
}

// dW[co][t][ci] = sum over tap t's slices in order of ws[g][co][ci]
__global__ __launch_bounds__(256) void pair_wgrad_reduce_kernel(PairTaps pt, const float *__restrict__ ws, int Cin,
                                                                int Cout, float *__restrict__ dW) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // index into dW [Cout][taps][Cin]
  const int taps = pt.taps;
  if (i >= (int64_t)Cout * taps * Cin) return;
  const int ci = (int)(i % Cin);
  const int64_t r = i / Cin;
  const int t = (int)(r % taps), co = (int)(r / taps);
  float s = 0.f;
  for (int g = pt.slice_off[t]; g < pt.slice_off[t + 1]; ++g) s += ws[((int64_t)g * Cout + co) * Cin + ci];
  dW[i] = s;
}

// LAUNCH(KST, OUT_BF16) of a forward gather kernel: 64-channel k-steps where Cin allows, Y's dtype
#define PCS_KST_OB(K64, OB, LAUNCH)                                     \
  do {                                                                  \
    if (K64) { if (OB) LAUNCH(64, true); else LAUNCH(64, false); }      \
    else { if (OB) LAUNCH(32, true); else LAUNCH(32, false); }          \
  } while (0)

// db = column sums of dY [M, Cout] through the sp slice partials wsb (vps rows per slice), the tail
// of every weight-gradient entry point (who: its name, for the error text)
int bias_grad(const void *dY, int Cout, int64_t M, int64_t sp, int64_t vps, float *wsb, float *db, hipStream_t s,
              const char *who) {
  hipError_t e = hipSuccess;
  if (M > 0)
    hipLaunchKernelGGL(conv3d_bgrad_kernel, dim3((unsigned)((Cout + 63) / 64), (unsigned)sp), dim3(THREADS), 0, s,
                       static_cast<const bf16_t *>(dY), Cout, M, vps, wsb);
  else
    e = hipMemsetAsync(wsb, 0, sp * Cout * 4, s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return pcs_set_error(e, who);
  hipLaunchKernelGGL(conv3d_reduce_kernel, dim3((unsigned)((Cout + 255) / 256)), dim3(256), 0, s, wsb, sp, (int64_t)Cout, db);
  e = hipGetLastError();
  return e != hipSuccess ? pcs_set_error(e, who) : 0;
}

int launched(const char *who) {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? pcs_set_error(e, who) : 0;
}

// The launches behind the sparse entry points, after their argument checks: XF is Rows1 or Rows2, YF
// Out1 or Out2 (the two-source layer's blocks are multiples of 64 channels: 64-deep k-steps), ep the
// forward epilogue (EpiNone, or EpiAffine behind the pcs_*_affine entry points of pcs_fold.h).

// sparse_conv_kernel over M > 0 rows
template <class XF, class YF, class... EP>
int launch_sparse_conv(const char *who, const int32_t *nbr, int64_t M, int taps, typename XF::Arg X, int Cin, const void *W,
                       int Cout, const float *bias, typename YF::Arg Y, int ydtype, int flip, hipStream_t s, EP... ep) {
  const int64_t tiles = (M + 63) / 64;
  if (tiles > 0x7fffffff) return pcs_set_einval(who, "too many rows");
  const dim3 grid((unsigned)tiles, (unsigned)(Cout / BN));
  const bf16_t *Wb = static_cast<const bf16_t *>(W);
#define PCS_SC(KST, OB) \
  hipLaunchKernelGGL((sparse_conv_kernel<64, KST, OB, XF, YF, EP...>), grid, dim3(THREADS), 0, s, nbr, M, taps, X, Cin, Wb, \
                     Cout, bias, Y, flip, ep...)
  if constexpr (XF::SPLIT || YF::SPLIT) {
    if (ydtype == PCS_BF16) PCS_SC(64, true); else PCS_SC(64, false);
  } else {
    PCS_KST_OB(Cin % 64 == 0, ydtype == PCS_BF16, PCS_SC);
  }
#undef PCS_SC
  return launched(who);
}

// pair_gemm_kernel over the pair tiles into Z, then pair_reduce_kernel over the M rows
template <class XF, class YF, class... EP>
int launch_pair_conv(const char *who, const PairTaps &pt, const int32_t *pair_in, const int32_t *pair_pos, int64_t M,
                     typename XF::Arg X, int Cin, const void *W, int Cout, const float *bias, float *Z,
                     typename YF::Arg Y, int ydtype, int flip, hipStream_t s, EP... ep) {
  const int taps = pt.taps, tiles = pt.tile_off[taps];
  const bf16_t *Wb = static_cast<const bf16_t *>(W);
  if (tiles > 0) {
    const dim3 grid((unsigned)tiles, (unsigned)(Cout / BN));
    if (XF::SPLIT || Cin % 64 == 0)
      hipLaunchKernelGGL((pair_gemm_kernel<64, XF>), grid, dim3(THREADS), 0, s, pt, pair_in, X, Cin, Wb, Cout,
                         flip, Z);
    else if constexpr (!XF::SPLIT)
      hipLaunchKernelGGL((pair_gemm_kernel<32, XF>), grid, dim3(THREADS), 0, s, pt, pair_in, X, Cin, Wb, Cout,
                         flip, Z);
    if (const int rc = launched(who)) return rc;
  }
  const int64_t n = M * (Cout / 8);
  if (n > 0) {
    const dim3 g((unsigned)((n + 255) / 256));
    if (ydtype == PCS_BF16)
      hipLaunchKernelGGL((pair_reduce_kernel<true, YF, EP...>), g, dim3(256), 0, s, pair_pos, M, taps, Z, Cout, bias,
                         Y, ep...);
    else
      hipLaunchKernelGGL((pair_reduce_kernel<false, YF, EP...>), g, dim3(256), 0, s, pair_pos, M, taps, Z, Cout, bias,
                         Y, ep...);
    return launched(who);
  }
  return 0;
}

// sparse_wgrad_kernel's slice partials (zeros when M == 0), their sum into dW, and db
template <class XF>
int launch_sparse_wgrad(const char *who, const int32_t *nbr, int64_t M, int taps, typename XF::Arg X, int Cin, const void *dY,
                        int Cout, void *workspace, float *dW, float *db, hipStream_t s) {
  const int64_t sp = sparse_wgrad_splits(M, taps, Cin, Cout);
  const int64_t vps = ((M + sp - 1) / sp + WV - 1) / WV * WV;
  const int64_t wlen = (int64_t)Cout * taps * Cin;
  float *ws = static_cast<float *>(workspace), *wsb = ws + sp * wlen;
  if (M > 0) {
    hipLaunchKernelGGL(sparse_wgrad_kernel<XF>, dim3((unsigned)((Cout / 64) * (Cin / 64)), (unsigned)((taps + TG - 1) / TG), (unsigned)sp),
                       dim3(THREADS), 0, s, nbr, M, taps, X, Cin, static_cast<const bf16_t *>(dY), Cout, ws, vps);
  } else {
    const hipError_t e = hipMemsetAsync(ws, 0, sp * wlen * 4, s);
    if (e != hipSuccess) return pcs_set_error(e, who);
  }
  if (const int rc = launched(who)) return rc;
  hipLaunchKernelGGL(conv3d_reduce_kernel, dim3((unsigned)((wlen + 255) / 256)), dim3(256), 0, s, ws, sp, wlen, dW);
  if (const int rc = launched(who)) return rc;
  return db ? bias_grad(dY, Cout, M, sp, vps, wsb, db, s, who) : 0;
}

// The launches behind the dense stencil entry points (g: a stencil3 geometry, checked): XF is Rows1
// or Rows2, YF Out1 or Out2; the tiles are ctile(g.Cin) x ctile(g.Cout) whatever the source, so the
// two-source layer runs the split geometry of the layer on the concatenated array.

// stencil3_kernel over the 4 x 4 x 8 output blocks
template <class XF, class YF, class... EP>
int launch_stencil3(const char *who, const pcs_conv3d_geom &g, typename XF::Arg X, const void *W, const float *bias,
                    typename YF::Arg Y, int ydtype, hipStream_t s, EP... ep) {
  const int cs = ctile(g.Cin), nt = ctile(g.Cout);
  const int64_t nblk = stencil_blocks(g);
  if (nblk > 0x7fffffff) return pcs_set_einval(who, "grid too large");
  const dim3 sg((unsigned)nblk, (unsigned)(g.Cout / nt));
  const bf16_t *Ws = static_cast<const bf16_t *>(W);
#define PCS_S3(CS, NT)                                                                                          \
  do {                                                                                                          \
    if (ydtype == PCS_BF16) hipLaunchKernelGGL((stencil3_kernel<CS, NT, true, XF, YF, EP...>), sg, dim3(THREADS), 0, s, g, X, Ws, bias, Y, ep...); \
    else hipLaunchKernelGGL((stencil3_kernel<CS, NT, false, XF, YF, EP...>), sg, dim3(THREADS), 0, s, g, X, Ws, bias, Y, ep...);   \
  } while (0)
  if (cs == 64) { if (nt == 64) PCS_S3(64, 64); else PCS_S3(64, 32); }
  else { if (nt == 64) PCS_S3(32, 64); else PCS_S3(32, 32); }
#undef PCS_S3
  return launched(who);
}

// stencil3_wgrad_kernel's sp block-range partials into ws (the caller checks the launch and sums them)
template <class XF>
void launch_stencil3_wgrad(const pcs_conv3d_geom &g, typename XF::Arg X, const bf16_t *dY, float *ws, int64_t sp,
                           hipStream_t s) {
  const int cot = ctile(g.Cout), cit = ctile(g.Cin);
  const int64_t nb = stencil_blocks(g), bps = (nb + sp - 1) / sp;
  const dim3 grid((unsigned)((g.Cout / cot) * (g.Cin / cit)), 3u, (unsigned)sp);
#define PCS_SW(CO, CI) hipLaunchKernelGGL((stencil3_wgrad_kernel<CO, CI, XF>), grid, dim3(THREADS), 0, s, g, X, dY, ws, nb, bps)
  if (cot == 64) { if (cit == 64) PCS_SW(64, 64); else PCS_SW(64, 32); }
  else { if (cit == 64) PCS_SW(32, 64); else PCS_SW(32, 32); }
#undef PCS_SW
}

// what the pcs_*_affine entry points (include/pcs_fold.h) check beyond their twins, or nullptr
const char *affine_bad(const float *scale, const float *shift, const void *R) {
  if (!scale || !shift) return "NULL scale or shift";
  if (reinterpret_cast<uintptr_t>(R) % 16 != 0) return "R must be rows in Y's dtype, 16-byte aligned (or NULL)";
  return nullptr;
}
EpiAffine affine(const float *scale, const float *shift, const void *R, int relu) {
  return EpiAffine{scale, shift, R, relu != 0};
}

// pcs_conv3d and pcs_conv3d_affine (who: the entry point, for the error text)
template <class... EP>
int conv3d_forward(const char *who, const pcs_conv3d_geom *g, const void *X, const void *W, const float *bias, void *Y,
                   int32_t ydtype, pcs_stream_t stream, EP... ep) {
  const char *why = nullptr;
  if (!geom_ok(g, &why)) return pcs_set_einval(who, why);
  if (!X || !W || !Y) return pcs_set_einval(who, "X, W and Y are required");
  if (g->Cin % 32 != 0 || g->Cout % 32 != 0 || g->Cin <= 0 || g->Cout <= 0)
    return pcs_set_einval(who, "Cin and Cout must be multiples of 32");
  if (ydtype != PCS_F32 && ydtype != PCS_BF16) return pcs_set_einval(who, "Y dtype: PCS_F32 or PCS_BF16");
  const int64_t M = out_voxels(*g);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int cs = ctile(g->Cin), nt = ctile(g->Cout);
  if (stencil3(*g))   // halo-staged stencil (both forms)
    return launch_stencil3<Rows1, Out1>(who, *g, static_cast<const bf16_t *>(X), W, bias, Y, ydtype, s, ep...);
  // transposed stride 2: 8 parity classes, tiles of the largest class's sub-grid each.  128-voxel
  // tiles (8 MFMAs per wave per barrier) once there are enough of them to fill the chip
  const int64_t rows_cls = g->transposed && g->s == 2 ? g->B * ((g->Do + 1) / 2) * ((g->Ho + 1) / 2) * ((g->Wo + 1) / 2) : M;
  const int64_t ncb = g->Cout / nt;
  const int bmt = (rows_cls / 128) * ncb * (g->transposed && g->s == 2 ? 8 : 1) >= 2048 ? 128 : 64;
  const int64_t tiles = (rows_cls + bmt - 1) / bmt * (g->transposed && g->s == 2 ? 8 : 1);
  if (tiles <= 0 || tiles > 0x7fffffff) return pcs_set_einval(who, "grid too large");
  const dim3 grid((unsigned)tiles, (unsigned)ncb);
  const bf16_t *Xb = static_cast<const bf16_t *>(X), *Wb = static_cast<const bf16_t *>(W);
#define PCS_C3(BMT, KST, OB, NT) \
  hipLaunchKernelGGL((conv3d_kernel<BMT, KST, OB, NT, EP...>), grid, dim3(THREADS), 0, s, *g, Xb, Wb, bias, Y, M, ep...)
#define PCS_C3T(KST, OB)                                                                  \
  do {                                                                                    \
    if (bmt == 128) { if (nt == 64) PCS_C3(128, KST, OB, 64); else PCS_C3(128, KST, OB, 32); } \
    else { if (nt == 64) PCS_C3(64, KST, OB, 64); else PCS_C3(64, KST, OB, 32); }         \
  } while (0)
  PCS_KST_OB(cs == 64, ydtype == PCS_BF16, PCS_C3T);
#undef PCS_C3T
#undef PCS_C3
  return launched(who);
}

}  // namespace

extern "C" int pcs_conv3d(const pcs_conv3d_geom *g, const void *X, const void *W, const float *bias, void *Y,
                          int32_t ydtype, pcs_stream_t stream) {
  return conv3d_forward(__func__, g, X, W, bias, Y, ydtype, stream);
}

extern "C" int pcs_conv3d_affine(const pcs_conv3d_geom *g, const void *X, const void *W, const float *bias, void *Y,
                                 int32_t ydtype, const float *scale, const float *shift, const void *R, int32_t relu,
                                 pcs_stream_t stream) {
  if (const char *why = affine_bad(scale, shift, R)) return pcs_set_einval(__func__, why);
  return conv3d_forward(__func__, g, X, W, bias, Y, ydtype, stream, affine(scale, shift, R, relu));
}

extern "C" int64_t pcs_conv3d_wgrad_workspace(const pcs_conv3d_geom *g) {
  const char *why = nullptr;
  if (!geom_ok(g, &why)) return pcs_set_einval("pcs_conv3d_wgrad_workspace", why);
  if (g->Cin % 32 != 0 || g->Cout % 32 != 0 || g->Cin <= 0 || g->Cout <= 0)
    return pcs_set_einval("pcs_conv3d_wgrad_workspace", "Cin and Cout must be multiples of 32");
  const int64_t sp = wgrad_splits(*g);
  return sp * ((int64_t)g->Cout * g->k * g->k * g->k * g->Cin + g->Cout) * 4;
}

extern "C" int pcs_conv3d_wgrad(const pcs_conv3d_geom *g, const void *X, const void *dY, void *workspace,
                                int64_t workspace_bytes, float *dW, float *db, pcs_stream_t stream) {
  const int64_t need = pcs_conv3d_wgrad_workspace(g);
  if (need < 0) return (int)need;
  if (!X || !dY || !dW || !workspace || workspace_bytes < need)
    return pcs_set_einval("pcs_conv3d_wgrad", "X, dY, dW and a pcs_conv3d_wgrad_workspace-sized workspace are required");
  const int64_t M = out_voxels(*g), sp = wgrad_splits(*g), vps = wgrad_vps(*g, sp);
  const int taps = g->k * g->k * g->k;
  const int64_t wlen = (int64_t)g->Cout * taps * g->Cin;
  float *ws = static_cast<float *>(workspace), *wsb = ws + sp * wlen;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int cot = ctile(g->Cout), cit = ctile(g->Cin);
  const unsigned ntile = (unsigned)((g->Cout / cot) * (g->Cin / cit));
  const bf16_t *Xb = static_cast<const bf16_t *>(X), *dYb = static_cast<const bf16_t *>(dY);
  if (stencil3(*g)) {
    launch_stencil3_wgrad<Rows1>(*g, Xb, dYb, ws, sp, s);
  } else {
    const int groups = g->transposed && g->s == 2 ? taps : g->k * g->k;   // workgroups per (co, ci) tile and slice
    const dim3 grid(ntile, (unsigned)groups, (unsigned)sp);
#define PCS_GW(CO, CI) hipLaunchKernelGGL((conv3d_wgrad_kernel<CO, CI>), grid, dim3(THREADS), 0, s, *g, Xb, dYb, ws, M, vps)
    if (cot == 64) { if (cit == 64) PCS_GW(64, 64); else PCS_GW(64, 32); }
    else { if (cit == 64) PCS_GW(32, 64); else PCS_GW(32, 32); }
#undef PCS_GW
  }
  PCS_CHECK_LAUNCH();
  hipLaunchKernelGGL(conv3d_reduce_kernel, dim3((unsigned)((wlen + 255) / 256)), dim3(256), 0, s, ws, sp, wlen, dW);
  PCS_CHECK_LAUNCH();
  return db ? bias_grad(dY, g->Cout, M, sp, vps, wsb, db, s, __func__) : 0;
}

extern "C" int pcs_conv3d_weight_t(const void *W, int32_t Cout, int32_t taps, int32_t Cin, void *Wt, pcs_stream_t stream) {
  if (!W || !Wt || Cout <= 0 || taps <= 0 || taps > 27 || Cin <= 0)
    return pcs_set_einval("pcs_conv3d_weight_t", "bad arguments (0 < taps <= 27)");
  const int64_t n = (int64_t)Cout * taps * Cin;
  hipLaunchKernelGGL(conv3d_weight_t_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), static_cast<const bf16_t *>(W), Cout, taps, Cin,
                     static_cast<bf16_t *>(Wt));
  PCS_CHECK_LAUNCH();
  return 0;
}

// ---- submanifold sparse convolution (hash-indexed gather; see sparse_conv_kernel)
namespace {
// pcs_sparse_conv and pcs_sparse_conv_affine
template <class... EP>
int sparse_conv_forward(const char *who, const int32_t *nbr, int64_t M, int32_t taps, const void *X, int32_t Cin,
                        const void *W, int32_t Cout, const float *bias, void *Y, int32_t ydtype, int32_t flip,
                        pcs_stream_t stream, EP... ep) {
  if (!nbr || !X || !W || !Y || M < 0 || taps < 1 || taps > 27 || Cin <= 0 || Cout <= 0 || Cin % KS != 0 ||
      Cout % BN != 0 || (ydtype != PCS_F32 && ydtype != PCS_BF16))
    return pcs_set_einval(who, "bad arguments (1 <= taps <= 27, Cin % 32 == 0, Cout % 64 == 0, Y f32 | bf16)");
  // flip = 1 reads tap taps - 1 - t for tap t: the input gradient's offset(taps - 1 - t) = -offset(t)
  // holds only for the full centred 27-tap map (or the single centre tap)
  if (flip != 0 && taps != 27 && taps != 1)
    return pcs_set_einval(who, "flip needs the centred 27-tap neighbour map (or taps == 1)");
  if (M == 0) return 0;
  return launch_sparse_conv<Rows1, Out1>(who, nbr, M, taps, static_cast<const bf16_t *>(X), Cin, W, Cout, bias, Y, ydtype,
                                         flip, reinterpret_cast<hipStream_t>(stream), ep...);
}
}  // namespace

extern "C" int pcs_sparse_conv(const int32_t *nbr, int64_t M, int32_t taps, const void *X, int32_t Cin, const void *W,
                               int32_t Cout, const float *bias, void *Y, int32_t ydtype, int32_t flip,
                               pcs_stream_t stream) {
  return sparse_conv_forward(__func__, nbr, M, taps, X, Cin, W, Cout, bias, Y, ydtype, flip, stream);
}

extern "C" int pcs_sparse_conv_affine(const int32_t *nbr, int64_t M, int32_t taps, const void *X, int32_t Cin,
                                      const void *W, int32_t Cout, const float *bias, void *Y, int32_t ydtype,
                                      int32_t flip, const float *scale, const float *shift, const void *R,
                                      int32_t relu, pcs_stream_t stream) {
  if (const char *why = affine_bad(scale, shift, R)) return pcs_set_einval(__func__, why);
  return sparse_conv_forward(__func__, nbr, M, taps, X, Cin, W, Cout, bias, Y, ydtype, flip, stream,
                             affine(scale, shift, R, relu));
}

extern "C" int64_t pcs_sparse_conv_wgrad_workspace(int64_t M, int32_t taps, int32_t Cin, int32_t Cout) {
  if (M < 0 || taps < 1 || taps > 27 || Cin <= 0 || Cout <= 0 || Cin % 64 != 0 || Cout % 64 != 0)
    return pcs_set_einval("pcs_sparse_conv_wgrad_workspace", "bad arguments (Cin, Cout multiples of 64)");
  const int64_t sp = sparse_wgrad_splits(M, taps, Cin, Cout);
  return sp * ((int64_t)Cout * taps * Cin + Cout) * 4;
}

extern "C" int pcs_sparse_conv_wgrad(const int32_t *nbr, int64_t M, int32_t taps, const void *X, int32_t Cin,
                                     const void *dY, int32_t Cout, void *workspace, int64_t workspace_bytes, float *dW,
                                     float *db, pcs_stream_t stream) {
  const int64_t need = pcs_sparse_conv_wgrad_workspace(M, taps, Cin, Cout);
  if (need < 0) return (int)need;
  if (!nbr || !X || !dY || !dW || !workspace || workspace_bytes < need)
    return pcs_set_einval("pcs_sparse_conv_wgrad", "nbr, X, dY, dW and a workspace of pcs_sparse_conv_wgrad_workspace bytes");
  return launch_sparse_wgrad<Rows1>(__func__, nbr, M, taps, static_cast<const bf16_t *>(X), Cin, dY, Cout, workspace, dW, db,
                             reinterpret_cast<hipStream_t>(stream));
}

// ---- per-tap pair lists (see pairs_count_kernel)
extern "C" int64_t pcs_sparse_pairs_workspace(int64_t M, int32_t taps) {
  if (M < 0 || taps < 1 || taps > PT_MAX) return pcs_set_einval("pcs_sparse_pairs_workspace", "bad arguments (1 <= taps <= 27)");
  return ((M + 255) / 256 * taps + 1) * 4;
}

extern "C" int pcs_sparse_pairs_count(const int32_t *nbr, int64_t M, int32_t taps, void *workspace, int64_t *tap_counts,
                                      pcs_stream_t stream) {
  const int64_t need = pcs_sparse_pairs_workspace(M, taps);
  if (need < 0) return (int)need;
  if (!nbr || !workspace || !tap_counts) return pcs_set_einval("pcs_sparse_pairs_count", "nbr, workspace and tap_counts are required");
  if (M * taps >= ((int64_t)1 << 31)) return pcs_set_einval("pcs_sparse_pairs_count", "M * taps must be < 2^31");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t nblk = (M + 255) / 256;
  int32_t *cnt = static_cast<int32_t *>(workspace);
  if (nblk > 0)
    hipLaunchKernelGGL(pairs_count_kernel, dim3((unsigned)nblk), dim3(256), 0, s, nbr, M, (int)taps, cnt);
  hipLaunchKernelGGL(pairs_scan_kernel, dim3((unsigned)taps), dim3(256), 0, s, cnt, nblk, (int)taps, tap_counts);
  PCS_CHECK_LAUNCH();
  return 0;
}

extern "C" int pcs_sparse_pairs_build(const int32_t *nbr, int64_t M, int32_t taps, const void *workspace,
                                      const int64_t *tap_counts, int32_t *pair_in, int32_t *pair_out, int32_t *pair_pos,
                                      pcs_stream_t stream) {
  if (pcs_sparse_pairs_workspace(M, taps) < 0) return PCS_EINVAL;
  if (!nbr || !workspace || !tap_counts || !pair_pos || ((!pair_in || !pair_out) && M > 0))
    return pcs_set_einval("pcs_sparse_pairs_build", "nbr, workspace, tap_counts, pair_in, pair_out and pair_pos are required");
  if (M * taps >= ((int64_t)1 << 31)) return pcs_set_einval("pcs_sparse_pairs_build", "M * taps must be < 2^31");
  const int64_t nblk = (M + 255) / 256;
  if (nblk > 0)
    hipLaunchKernelGGL(pairs_build_kernel, dim3((unsigned)nblk), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), nbr, M,
                       (int)taps, static_cast<const int32_t *>(workspace), tap_counts, pair_in, pair_out, pair_pos);
  PCS_CHECK_LAUNCH();
  return 0;
}

namespace {
// the tap and tile offsets of a pair list from the host copy of its tap offsets
const char *pair_taps(const int64_t *tap_off, int32_t taps, PairTaps *pt) {
  if (!tap_off || taps < 1 || taps > PT_MAX) return "tap_off (host, taps + 1 entries) and 1 <= taps <= 27";
  pt->taps = taps;
  int64_t tiles = 0;
  for (int t = 0; t <= taps; ++t) {
    if (tap_off[t] < (t ? tap_off[t - 1] : 0) || (t == 0 && tap_off[0] != 0)) return "tap_off must start at 0 and not decrease";
    pt->tap_off[t] = tap_off[t];
    pt->tile_off[t] = (int32_t)tiles;
    if (t < taps) tiles += (tap_off[t + 1] - tap_off[t] + 63) / 64;
  }
  if (tiles > 0x7fffffff || tap_off[taps] >= ((int64_t)1 << 31)) return "too many pairs";
  return nullptr;
}

// pcs_sparse_conv_pairs and pcs_sparse_conv_pairs_affine
template <class... EP>
int pairs_forward(const char *who, const int32_t *pair_in, const int32_t *pair_pos, const int64_t *tap_off, int32_t taps,
                  int64_t M, const void *X, int32_t Cin, const void *W, int32_t Cout, const float *bias, float *Z, void *Y,
                  int32_t ydtype, int32_t flip, pcs_stream_t stream, EP... ep) {
  PairTaps pt;
  const char *why = pair_taps(tap_off, taps, &pt);
  if (why) return pcs_set_einval(who, why);
  if (!pair_pos || !X || !W || !Y || M < 0 || Cin <= 0 || Cout <= 0 || Cin % KS != 0 || Cout % BN != 0 ||
      (ydtype != PCS_F32 && ydtype != PCS_BF16) || (tap_off[taps] > 0 && (!pair_in || !Z)))
    return pcs_set_einval(who, "bad arguments (Cin % 32 == 0, Cout % 64 == 0, Y f32 | bf16, Z [P, Cout] f32)");
  if (flip && taps != 27 && taps != 1) return pcs_set_einval(who, "flip needs the centred 27-tap neighbour map (or taps == 1)");
  return launch_pair_conv<Rows1, Out1>(who, pt, pair_in, pair_pos, M, static_cast<const bf16_t *>(X), Cin, W, Cout, bias,
                                       Z, Y, ydtype, flip, reinterpret_cast<hipStream_t>(stream), ep...);
}

// pcs_sparse_conv_rows and pcs_sparse_conv_rows_affine
template <class... EP>
int rows_forward(const char *who, const int32_t *pair_in, const int32_t *pair_out, const int64_t *tap_off, int32_t taps,
                 int64_t M, const void *X, int32_t Cin, const void *W, int32_t Cout, const float *bias, void *Y,
                 int32_t ydtype, pcs_stream_t stream, EP... ep) {
  PairTaps pt;
  const char *why = pair_taps(tap_off, taps, &pt);
  if (why) return pcs_set_einval(who, why);
  if (!X || !W || !Y || M < 0 || Cin <= 0 || Cout <= 0 || Cin % KS != 0 || Cout % BN != 0 ||
      (ydtype != PCS_F32 && ydtype != PCS_BF16) || (tap_off[taps] > 0 && (!pair_in || !pair_out)))
    return pcs_set_einval(who, "bad arguments (Cin % 32 == 0, Cout % 64 == 0, Y f32 | bf16)");
  if (tap_off[taps] != M) return pcs_set_einval(who, "every output row needs exactly one pair (tap_off[taps] == M)");
  const int tiles = pt.tile_off[taps];
  if (tiles == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)tiles, (unsigned)(Cout / BN));
  const bf16_t *Xb = static_cast<const bf16_t *>(X), *Wb = static_cast<const bf16_t *>(W);
#define PCS_PR(KST, OB) \
  hipLaunchKernelGGL((pair_rows_kernel<KST, OB, EP...>), grid, dim3(THREADS), 0, s, pt, pair_in, pair_out, Xb, (int)Cin, Wb, \
                     (int)Cout, bias, M, Y, ep...)
  PCS_KST_OB(Cin % 64 == 0, ydtype == PCS_BF16, PCS_PR);
#undef PCS_PR
  return launched(who);
}
}  // namespace

extern "C" int pcs_sparse_conv_pairs(const int32_t *pair_in, const int32_t *pair_pos, const int64_t *tap_off, int32_t taps,
                                     int64_t M, const void *X, int32_t Cin, const void *W, int32_t Cout,
                                     const float *bias, float *Z, void *Y, int32_t ydtype, int32_t flip,
                                     pcs_stream_t stream) {
  return pairs_forward(__func__, pair_in, pair_pos, tap_off, taps, M, X, Cin, W, Cout, bias, Z, Y, ydtype, flip, stream);
}

extern "C" int pcs_sparse_conv_pairs_affine(const int32_t *pair_in, const int32_t *pair_pos, const int64_t *tap_off,
                                            int32_t taps, int64_t M, const void *X, int32_t Cin, const void *W,
                                            int32_t Cout, const float *bias, float *Z, void *Y, int32_t ydtype,
                                            int32_t flip, const float *scale, const float *shift, const void *R,
                                            int32_t relu, pcs_stream_t stream) {
  if (const char *why = affine_bad(scale, shift, R)) return pcs_set_einval(__func__, why);
  return pairs_forward(__func__, pair_in, pair_pos, tap_off, taps, M, X, Cin, W, Cout, bias, Z, Y, ydtype, flip, stream,
                       affine(scale, shift, R, relu));
}

extern "C" int pcs_sparse_conv_rows(const int32_t *pair_in, const int32_t *pair_out, const int64_t *tap_off, int32_t taps,
                                    int64_t M, const void *X, int32_t Cin, const void *W, int32_t Cout,
                                    const float *bias, void *Y, int32_t ydtype, pcs_stream_t stream) {
  return rows_forward(__func__, pair_in, pair_out, tap_off, taps, M, X, Cin, W, Cout, bias, Y, ydtype, stream);
}

extern "C" int pcs_sparse_conv_rows_affine(const int32_t *pair_in, const int32_t *pair_out, const int64_t *tap_off,
                                           int32_t taps, int64_t M, const void *X, int32_t Cin, const void *W,
                                           int32_t Cout, const float *bias, void *Y, int32_t ydtype, const float *scale,
                                           const float *shift, const void *R, int32_t relu, pcs_stream_t stream) {
  if (const char *why = affine_bad(scale, shift, R)) return pcs_set_einval(__func__, why);
  return rows_forward(__func__, pair_in, pair_out, tap_off, taps, M, X, Cin, W, Cout, bias, Y, ydtype, stream,
                      affine(scale, shift, R, relu));
}

namespace {
// weight-gradient slices: slice_len pairs each (at least 4 k-steps), ceil(count / slice_len) per
// tap (at least one, so every tap's partial is written), about 2048 workgroups over the slices
// and the 64 x 64 channel tiles together (as sparse_wgrad_splits): each slice holds a full
// Cout x Cin fp32 partial, so the workspace stays near 2048 tiles' worth (34 MB at 64 -> 64, 40 MB
// at 256 -> 256, where a fixed 2048 slices took 544 MB) instead of growing with the channel product
void pair_wgrad_slices(PairTaps *pt, int Cin, int Cout) {
  const int64_t P = pt->tap_off[pt->taps];
  const int64_t tiles = (int64_t)(Cout / 64) * (Cin / 64);
  const int64_t target = (2048 + tiles - 1) / tiles;
  int64_t len = (P + target - 1) / target;
  len = (len < 4 * WV ? 4 * WV : len + WV - 1) / WV * WV;
  pt->slice_len = len;
  int64_t g = 0;
  for (int t = 0; t <= pt->taps; ++t) {
    pt->slice_off[t] = (int32_t)g;
    if (t < pt->taps) {
      const int64_t c = pt->tap_off[t + 1] - pt->tap_off[t];
      g += c > 0 ? (c + len - 1) / len : 1;
    }
  }
}

// pair_wgrad_kernel's slice partials (pt with its slices), their sum into dW, and db
template <class XF>
int launch_pair_wgrad(const char *who, const PairTaps &pt, const int32_t *pair_in, const int32_t *pair_out, int64_t M,
                      typename XF::Arg X, int Cin, const void *dY, int Cout, void *workspace, float *dW, float *db, hipStream_t s) {
  const int taps = pt.taps;
  const int64_t ns = pt.slice_off[taps], wlen = (int64_t)Cout * taps * Cin;
  float *ws = static_cast<float *>(workspace), *wsb = ws + ns * Cout * Cin;
  hipLaunchKernelGGL(pair_wgrad_kernel<XF>, dim3((unsigned)((Cout / 64) * (Cin / 64)), (unsigned)ns), dim3(THREADS), 0, s, pt,
                     pair_in, pair_out, X, Cin, static_cast<const bf16_t *>(dY), Cout, ws);
  if (const int rc = launched(who)) return rc;
  hipLaunchKernelGGL(pair_wgrad_reduce_kernel, dim3((unsigned)((wlen + 255) / 256)), dim3(256), 0, s, pt, ws, Cin, Cout, dW);
  if (const int rc = launched(who)) return rc;
  if (!db) return 0;
  const int64_t spb = sparse_wgrad_splits(M, 1, 64, Cout);
  return bias_grad(dY, Cout, M, spb, ((M + spb - 1) / spb + WV - 1) / WV * WV, wsb, db, s, who);
}
}  // namespace

extern "C" int64_t pcs_sparse_conv_wgrad_pairs_workspace(const int64_t *tap_off, int32_t taps, int64_t M, int32_t Cin,
                                                         int32_t Cout) {
  PairTaps pt;
  const char *why = pair_taps(tap_off, taps, &pt);
  if (why) return pcs_set_einval("pcs_sparse_conv_wgrad_pairs_workspace", why);
  if (M < 0 || Cin <= 0 || Cout <= 0 || Cin % 64 != 0 || Cout % 64 != 0)
    return pcs_set_einval("pcs_sparse_conv_wgrad_pairs_workspace", "bad arguments (Cin, Cout multiples of 64)");
  pair_wgrad_slices(&pt, Cin, Cout);
  const int64_t spb = sparse_wgrad_splits(M, 1, 64, Cout);
  return ((int64_t)pt.slice_off[taps] * Cout * Cin + spb * Cout) * 4;
}

extern "C" int pcs_sparse_conv_wgrad_pairs(const int32_t *pair_in, const int32_t *pair_out, const int64_t *tap_off,
                                           int32_t taps, int64_t M, const void *X, int32_t Cin, const void *dY,
                                           int32_t Cout, void *workspace, int64_t workspace_bytes, float *dW, float *db,
                                           pcs_stream_t stream) {
  const int64_t need = pcs_sparse_conv_wgrad_pairs_workspace(tap_off, taps, M, Cin, Cout);
  if (need < 0) return (int)need;
  if (!X || !dY || !dW || !workspace || workspace_bytes < need || (tap_off[taps] > 0 && (!pair_in || !pair_out)))
    return pcs_set_einval("pcs_sparse_conv_wgrad_pairs", "pairs, X, dY, dW and a workspace of pcs_sparse_conv_wgrad_pairs_workspace bytes");
  PairTaps pt;
  pair_taps(tap_off, taps, &pt);
  pair_wgrad_slices(&pt, Cin, Cout);
  return launch_pair_wgrad<Rows1>(__func__, pt, pair_in, pair_out, M, static_cast<const bf16_t *>(X), Cin, dY, Cout, workspace,
                           dW, db, reinterpret_cast<hipStream_t>(stream));
}

// ---- the two-source layer: the kernels above on X = [XA | XB] along channels, never materialised
// (Rows2 / Out2).  Same k-step order, split geometry and workspaces as the layer on the
// concatenated array (Cin = CA + CB), so every result is bit-identical to it.
namespace {
// the rules the six entry points share, or nullptr
const char *cat_args_bad(int64_t M, int taps, int CA, int CB, int Cout, int ydtype, int flip) {
  if (M < 0) return "M must be >= 0";
  if (taps < 1 || taps > PT_MAX) return "1 <= taps <= 27";
  if (CA <= 0 || CB <= 0 || Cout <= 0 || CA % 64 != 0 || CB % 64 != 0 || Cout % 64 != 0 || (int64_t)CA + CB > (1 << 20) ||
      Cout > (1 << 20))
    return "CA, CB and Cout must be positive multiples of 64";
  if (ydtype != PCS_F32 && ydtype != PCS_BF16) return "output dtype: PCS_F32 or PCS_BF16";
  if (flip != 0 && flip != 1) return "flip must be 0 or 1";
  if (flip && taps != 27 && taps != 1) return "flip needs the centred 27-tap neighbour map (or taps == 1)";
  return nullptr;
}
Rows2 rows2(const void *XA, int CA, const void *XB) {
  return Rows2{static_cast<const bf16_t *>(XA), static_cast<const bf16_t *>(XB), CA};
}

// pcs_sparse_conv_cat and pcs_sparse_conv_cat_affine
template <class... EP>
int cat_forward(const char *who, const int32_t *nbr, int64_t M, int32_t taps, const void *XA, int32_t CA, const void *XB,
                int32_t CB, const void *W, int32_t Cout, const float *bias, void *Y, int32_t ydtype, int32_t flip,
                pcs_stream_t stream, EP... ep) {
  if (const char *why = cat_args_bad(M, taps, CA, CB, Cout, ydtype, flip)) return pcs_set_einval(who, why);
  if (!nbr || !XA || !XB || !W || !Y) return pcs_set_einval(who, "NULL nbr, XA, XB, W or Y");
  if (M == 0) return 0;
  return launch_sparse_conv<Rows2, Out1>(who, nbr, M, taps, rows2(XA, CA, XB), CA + CB, W, Cout, bias, Y, ydtype, flip,
                                         reinterpret_cast<hipStream_t>(stream), ep...);
}

// pcs_sparse_conv_cat_pairs and pcs_sparse_conv_cat_pairs_affine
template <class... EP>
int cat_pairs_forward(const char *who, const int32_t *pair_in, const int32_t *pair_pos, const int64_t *tap_off, int32_t taps,
                      int64_t M, const void *XA, int32_t CA, const void *XB, int32_t CB, const void *W, int32_t Cout,
                      const float *bias, float *Z, void *Y, int32_t ydtype, int32_t flip, pcs_stream_t stream, EP... ep) {
  if (const char *why = cat_args_bad(M, taps, CA, CB, Cout, ydtype, flip)) return pcs_set_einval(who, why);
  PairTaps pt;
  if (const char *why = pair_taps(tap_off, taps, &pt)) return pcs_set_einval(who, why);
  if (!pair_pos || !XA || !XB || !W || !Y || (tap_off[taps] > 0 && (!pair_in || !Z)))
    return pcs_set_einval(who, "NULL pair_pos, XA, XB, W or Y (or pair_in, Z with pairs)");
  if (M == 0) return 0;
  return launch_pair_conv<Rows2, Out1>(who, pt, pair_in, pair_pos, M, rows2(XA, CA, XB), CA + CB, W, Cout, bias, Z, Y, ydtype,
                                       flip, reinterpret_cast<hipStream_t>(stream), ep...);
}
}  // namespace

extern "C" int pcs_sparse_conv_cat(const int32_t *nbr, int64_t M, int32_t taps, const void *XA, int32_t CA, const void *XB,
                                   int32_t CB, const void *W, int32_t Cout, const float *bias, void *Y, int32_t ydtype,
                                   int32_t flip, pcs_stream_t stream) {
  return cat_forward(__func__, nbr, M, taps, XA, CA, XB, CB, W, Cout, bias, Y, ydtype, flip, stream);
}

extern "C" int pcs_sparse_conv_cat_affine(const int32_t *nbr, int64_t M, int32_t taps, const void *XA, int32_t CA,
                                          const void *XB, int32_t CB, const void *W, int32_t Cout, const float *bias,
                                          void *Y, int32_t ydtype, int32_t flip, const float *scale, const float *shift,
                                          const void *R, int32_t relu, pcs_stream_t stream) {
  if (const char *why = affine_bad(scale, shift, R)) return pcs_set_einval(__func__, why);
  return cat_forward(__func__, nbr, M, taps, XA, CA, XB, CB, W, Cout, bias, Y, ydtype, flip, stream,
                     affine(scale, shift, R, relu));
}

extern "C" int pcs_sparse_conv_cat_pairs_affine(const int32_t *pair_in, const int32_t *pair_pos, const int64_t *tap_off,
                                                int32_t taps, int64_t M, const void *XA, int32_t CA, const void *XB,
                                                int32_t CB, const void *W, int32_t Cout, const float *bias, float *Z,
                                                void *Y, int32_t ydtype, int32_t flip, const float *scale,
                                                const float *shift, const void *R, int32_t relu, pcs_stream_t stream) {
  if (const char *why = affine_bad(scale, shift, R)) return pcs_set_einval(__func__, why);
  return cat_pairs_forward(__func__, pair_in, pair_pos, tap_off, taps, M, XA, CA, XB, CB, W, Cout, bias, Z, Y, ydtype, flip,
                           stream, affine(scale, shift, R, relu));
}

extern "C" int pcs_sparse_conv_cat_dgrad(const int32_t *nbr, int64_t M, int32_t taps, const void *dY, int32_t Cout,
                                         const void *Wt, void *dXA, int32_t CA, void *dXB, int32_t CB, int32_t xdtype,
                                         int32_t flip, pcs_stream_t stream) {
  if (const char *why = cat_args_bad(M, taps, CA, CB, Cout, xdtype, flip)) return pcs_set_einval(__func__, why);
  if (!nbr || !dY || !Wt || !dXA || !dXB) return pcs_set_einval(__func__, "NULL nbr, dY, Wt, dXA or dXB");
  if (M == 0) return 0;
  return launch_sparse_conv<Rows1, Out2>(__func__, nbr, M, taps, static_cast<const bf16_t *>(dY), Cout, Wt, CA + CB, nullptr,
                            Out2{dXA, dXB, CA}, xdtype, flip, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pcs_sparse_conv_cat_wgrad(const int32_t *nbr, int64_t M, int32_t taps, const void *XA, int32_t CA,
                                         const void *XB, int32_t CB, const void *dY, int32_t Cout, void *workspace,
                                         int64_t workspace_bytes, float *dW, float *db, pcs_stream_t stream) {
  if (const char *why = cat_args_bad(M, taps, CA, CB, Cout, PCS_BF16, 0)) return pcs_set_einval(__func__, why);
  if (!nbr || !XA || !XB || !dY || !dW || !workspace) return pcs_set_einval(__func__, "NULL nbr, XA, XB, dY, dW or workspace");
  if (workspace_bytes < pcs_sparse_conv_wgrad_workspace(M, taps, CA + CB, Cout))
    return pcs_set_einval(__func__, "the workspace is shorter than pcs_sparse_conv_wgrad_workspace(M, taps, CA + CB, Cout)");
  if (M == 0) return 0;
  return launch_sparse_wgrad<Rows2>(__func__, nbr, M, taps, rows2(XA, CA, XB), CA + CB, dY, Cout, workspace, dW, db,
                             reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pcs_sparse_conv_cat_pairs(const int32_t *pair_in, const int32_t *pair_pos, const int64_t *tap_off,
                                         int32_t taps, int64_t M, const void *XA, int32_t CA, const void *XB, int32_t CB,
                                         const void *W, int32_t Cout, const float *bias, float *Z, void *Y, int32_t ydtype,
                                         int32_t flip, pcs_stream_t stream) {
  return cat_pairs_forward(__func__, pair_in, pair_pos, tap_off, taps, M, XA, CA, XB, CB, W, Cout, bias, Z, Y, ydtype, flip,
                           stream);
}

extern "C" int pcs_sparse_conv_cat_dgrad_pairs(const int32_t *pair_in, const int32_t *pair_pos, const int64_t *tap_off,
                                               int32_t taps, int64_t M, const void *dY, int32_t Cout, const void *Wt,
                                               float *Z, void *dXA, int32_t CA, void *dXB, int32_t CB, int32_t xdtype,
                                               int32_t flip, pcs_stream_t stream) {
  if (const char *why = cat_args_bad(M, taps, CA, CB, Cout, xdtype, flip)) return pcs_set_einval(__func__, why);
  PairTaps pt;
  if (const char *why = pair_taps(tap_off, taps, &pt)) return pcs_set_einval(__func__, why);
  if (!pair_pos || !dY || !Wt || !dXA || !dXB || (tap_off[taps] > 0 && (!pair_in || !Z)))
    return pcs_set_einval(__func__, "NULL pair_pos, dY, Wt, dXA or dXB (or pair_in, Z with pairs)");
  if (M == 0) return 0;
  return launch_pair_conv<Rows1, Out2>(__func__, pt, pair_in, pair_pos, M, static_cast<const bf16_t *>(dY), Cout, Wt, CA + CB,
                          nullptr, Z, Out2{dXA, dXB, CA}, xdtype, flip, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pcs_sparse_conv_cat_wgrad_pairs(const int32_t *pair_in, const int32_t *pair_out, const int64_t *tap_off,
                                               int32_t taps, int64_t M, const void *XA, int32_t CA, const void *XB,
                                               int32_t CB, const void *dY, int32_t Cout, void *workspace,
                                               int64_t workspace_bytes, float *dW, float *db, pcs_stream_t stream) {
  if (const char *why = cat_args_bad(M, taps, CA, CB, Cout, PCS_BF16, 0)) return pcs_set_einval(__func__, why);
  PairTaps pt;
  if (const char *why = pair_taps(tap_off, taps, &pt)) return pcs_set_einval(__func__, why);
  if (!XA || !XB || !dY || !dW || !workspace || (tap_off[taps] > 0 && (!pair_in || !pair_out)))
    return pcs_set_einval(__func__, "NULL XA, XB, dY, dW or workspace (or pair_in, pair_out with pairs)");
  if (workspace_bytes < pcs_sparse_conv_wgrad_pairs_workspace(tap_off, taps, M, CA + CB, Cout))
    return pcs_set_einval(__func__,
                          "the workspace is shorter than pcs_sparse_conv_wgrad_pairs_workspace(tap_off, taps, M, CA + CB, Cout)");
  if (M == 0) return 0;
  pair_wgrad_slices(&pt, CA + CB, Cout);
  return launch_pair_wgrad<Rows2>(__func__, pt, pair_in, pair_out, M, rows2(XA, CA, XB), CA + CB, dY, Cout, workspace, dW, db,
                           reinterpret_cast<hipStream_t>(stream));
}

// ---- the two-source dense stencil (include/pcs_dense.h): stencil3_kernel / stencil3_wgrad_kernel on
// X = [XA | XB] along channels (Rows2), the input gradient written as dXA | dXB (Out2).  The tiles,
// the k-step order, the block ranges and the workspace are those of pcs_conv3d / pcs_conv3d_wgrad at
// Cin = CA + CB, so every result is bit-identical to the layer on the concatenated array.
namespace {
// the rules the three entry points share, or nullptr; cat = the geometry's channel count that is split
// into CA | CB, other = the one that is not
const char *dense_cat_bad(const pcs_conv3d_geom *g, int cat, int other, int CA, int CB, int dtype) {
  const char *why = nullptr;
  if (!geom_ok(g, &why)) return why;
  if (!stencil3(*g)) return "the two-source layer is the 3x3x3 stride-1 stencil (k == 3, s == 1)";
  if (CA <= 0 || CB <= 0 || other <= 0 || CA % 32 != 0 || CB % 32 != 0 || other % 32 != 0 || CA > (1 << 20) ||
      CB > (1 << 20))
    return "CA, CB and Cout must be positive multiples of 32";
  if (cat != CA + CB) return "the geometry's channel count must be CA + CB";
  if (dtype != PCS_F32 && dtype != PCS_BF16) return "output dtype: PCS_F32 or PCS_BF16";
  if (stencil_blocks(*g) > 0x7fffffff) return "grid too large";
  return nullptr;
}

// pcs_conv3d_cat and pcs_conv3d_cat_affine
template <class... EP>
int dense_cat_forward(const char *who, const pcs_conv3d_geom *g, const void *XA, int32_t CA, const void *XB, int32_t CB,
                      const void *W, const float *bias, void *Y, int32_t ydtype, pcs_stream_t stream, EP... ep) {
  if (const char *why = dense_cat_bad(g, g ? g->Cin : 0, g ? g->Cout : 0, CA, CB, ydtype)) return pcs_set_einval(who, why);
  if (!XA || !XB || !W || !Y) return pcs_set_einval(who, "NULL XA, XB, W or Y");
  return launch_stencil3<Rows2, Out1>(who, *g, rows2(XA, CA, XB), W, bias, Y, ydtype, reinterpret_cast<hipStream_t>(stream), ep...);
}
}  // namespace

extern "C" int pcs_conv3d_cat(const pcs_conv3d_geom *g, const void *XA, int32_t CA, const void *XB, int32_t CB,
                              const void *W, const float *bias, void *Y, int32_t ydtype, pcs_stream_t stream) {
  return dense_cat_forward(__func__, g, XA, CA, XB, CB, W, bias, Y, ydtype, stream);
}

extern "C" int pcs_conv3d_cat_affine(const pcs_conv3d_geom *g, const void *XA, int32_t CA, const void *XB, int32_t CB,
                                     const void *W, const float *bias, void *Y, int32_t ydtype, const float *scale,
                                     const float *shift, const void *R, int32_t relu, pcs_stream_t stream) {
  if (const char *why = affine_bad(scale, shift, R)) return pcs_set_einval(__func__, why);
  return dense_cat_forward(__func__, g, XA, CA, XB, CB, W, bias, Y, ydtype, stream, affine(scale, shift, R, relu));
}

extern "C" int pcs_conv3d_cat_dgrad(const pcs_conv3d_geom *g, const void *dY, const void *Wt, void *dXA, int32_t CA,
                                    void *dXB, int32_t CB, int32_t xdtype, pcs_stream_t stream) {
  if (const char *why = dense_cat_bad(g, g ? g->Cout : 0, g ? g->Cin : 0, CA, CB, xdtype)) return pcs_set_einval(__func__, why);
  if (!dY || !Wt || !dXA || !dXB) return pcs_set_einval(__func__, "NULL dY, Wt, dXA or dXB");
  return launch_stencil3<Rows1, Out2>(__func__, *g, static_cast<const bf16_t *>(dY), Wt, nullptr, Out2{dXA, dXB, CA}, xdtype,
                                      reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pcs_conv3d_cat_wgrad(const pcs_conv3d_geom *g, const void *XA, int32_t CA, const void *XB, int32_t CB,
                                    const void *dY, void *workspace, int64_t workspace_bytes, float *dW, float *db,
                                    pcs_stream_t stream) {
  if (const char *why = dense_cat_bad(g, g ? g->Cin : 0, g ? g->Cout : 0, CA, CB, PCS_BF16)) return pcs_set_einval(__func__, why);
  if (!XA || !XB || !dY || !dW || !workspace) return pcs_set_einval(__func__, "NULL XA, XB, dY, dW or workspace");
  if (workspace_bytes < pcs_conv3d_wgrad_workspace(g))
    return pcs_set_einval(__func__, "the workspace is shorter than pcs_conv3d_wgrad_workspace(g) at Cin = CA + CB");
  const int64_t M = out_voxels(*g), sp = wgrad_splits(*g), vps = wgrad_vps(*g, sp);
  const int64_t wlen = (int64_t)g->Cout * 27 * g->Cin;
  float *ws = static_cast<float *>(workspace), *wsb = ws + sp * wlen;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  launch_stencil3_wgrad<Rows2>(*g, rows2(XA, CA, XB), static_cast<const bf16_t *>(dY), ws, sp, s);
  if (const int rc = launched(__func__)) return rc;
  hipLaunchKernelGGL(conv3d_reduce_kernel, dim3((unsigned)((wlen + 255) / 256)), dim3(256), 0, s, ws, sp, wlen, dW);
  if (const int rc = launched(__func__)) return rc;
  return db ? bias_grad(dY, g->Cout, M, sp, vps, wsb, db, s, __func__) : 0;
}
