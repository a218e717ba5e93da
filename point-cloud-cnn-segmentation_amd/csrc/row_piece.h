// The row scheme of the bandwidth-bound kernels on the occupied-voxel path (sparse_bn.hip,
// pointhead.hip, pointvoxel.hip): a row of C channels is C / E lanes of E elements (E = 8 when either
// side of the kernel is bf16, else 4: 16 bytes of the narrower type), a workgroup of 256 threads
// holds 256 / (C / E) rows per pass (the lanes left over when C / E does not divide 256 idle), and a
// lane keeps its pieces as raw 16-byte registers between the load and the use, so that it issues all
// its loads before it waits for the first.  With them the host-side parts these files share: the
// dtype and width checks, the block geometry of a reduction and the (xdtype, ydtype) dispatch.
// One definition each: no .hip file defines a function or struct of these names
// (tests/test_csrc_helpers.py), and a change here has to leave every file's device code as
// intended (tools/asm_equal.py compares it against a revision).
#pragma once
#include "common.h"

namespace pcs_rows {

constexpr int THREADS = 256;
constexpr int MAX_C = 1024;        // of the kernels that bound C
constexpr int ROW_TILE = 64;       // rows per block of a reduction are a multiple of this
constexpr int MAX_BLOCKS = 2048;   // of a reduction (~8 per CU)

template <typename A, typename B>
struct Piece {
  static constexpr int E = (Elem<A>::EPC == 8 || Elem<B>::EPC == 8) ? 8 : 4;
};

// a lane's E elements of a row as raw 16-byte registers: loads first, conversion at the use
template <typename T, int E>
struct Raw {
  static constexpr int NQ = E * Elem<T>::SIZE / 16;
  u32x4 q[NQ];
};

template <typename T, int E>
PCS_DEV void raw_load(Raw<T, E> &r, const T *__restrict__ p, bool present) {
#pragma unroll
  for (int i = 0; i < Raw<T, E>::NQ; ++i)
    r.q[i] = present ? reinterpret_cast<const u32x4 *>(p)[i] : mk_u32x4(0u, 0u, 0u, 0u);
}

template <typename T, int E>
PCS_DEV void raw_unpack(const Raw<T, E> &r, float (&v)[E]) {
  constexpr int EPC = Elem<T>::EPC;
#pragma unroll
  for (int i = 0; i < Raw<T, E>::NQ; ++i) {
    float t[EPC];
    unpack_chunk(r.q[i], t);
#pragma unroll
    for (int e = 0; e < EPC; ++e) v[i * EPC + e] = t[e];
  }
}

// acc += w * the piece
template <typename T, int E>
PCS_DEV void raw_fma(const Raw<T, E> &r, float w, float (&acc)[E]) {
  constexpr int EPC = Elem<T>::EPC;
#pragma unroll
  for (int i = 0; i < Raw<T, E>::NQ; ++i) {
    float v[EPC];
    unpack_chunk(r.q[i], v);
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[i * EPC + e] += w * v[e];
  }
}

// NT: through st16 (non-temporal), for rows that only a later kernel reads back
template <typename T, int E, bool NT = false>
PCS_DEV void store_piece(T *__restrict__ p, const float (&v)[E]) {
  constexpr int EPC = Elem<T>::EPC;
#pragma unroll
  for (int i = 0; i < E / EPC; ++i) {
    float t[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) t[e] = v[i * EPC + e];
    if constexpr (NT) st16(reinterpret_cast<u32x4 *>(p) + i, pack_chunk(t));
    else reinterpret_cast<u32x4 *>(p)[i] = pack_chunk(t);
  }
}

// This thread's (row slot r0, piece cc) in a workgroup of rpp = 256 / lpr rows; false: a lane left
// over.  Two forms, because the kernels that bound C (lpr <= 256) must not pay for the case they
// never meet: written in the wide form they gain a compare and a branch in their prologue.
PCS_DEV bool lane_slot(int lpr, int &rpp, int &r0, int &cc) {
  rpp = THREADS / lpr;
  r0 = (int)threadIdx.x / lpr;
  cc = (int)threadIdx.x - r0 * lpr;
  return r0 < rpp;
}

// any C: one row, pieces strided by 256, when a row has 256 pieces or more (cc is then the first)
PCS_DEV bool lane_slot_wide(int lpr, int &rpp, int &r0, int &cc) {
  rpp = lpr >= THREADS ? 1 : THREADS / lpr;
  r0 = (int)threadIdx.x / lpr;
  cc = (int)threadIdx.x - r0 * lpr;
  return r0 < rpp;
}

// ---- host side
inline bool known(int32_t dtype) { return dtype == PCS_F32 || dtype == PCS_BF16; }

// C a multiple of the piece (8 when either side is bf16, else 4) and, if bounded, at most MAX_C
inline const char *check_width(int32_t xdtype, int32_t ydtype, int32_t C, bool bounded = false) {
  if (!known(xdtype) || !known(ydtype)) return "unknown dtype (PCS_F32 | PCS_BF16)";
  const int e = (xdtype == PCS_BF16 || ydtype == PCS_BF16) ? 8 : 4;
  if (C < e || C % e != 0 || (bounded && C > MAX_C))
    return bounded ? "C % 8 == 0 (bf16 on either side) or C % 4 == 0 (fp32), C <= 1024 required"
                   : "C % 8 == 0 (bf16 on either side) or C % 4 == 0 (fp32) required";
  return nullptr;
}

struct Blocks {
  int64_t per;   // rows (points) of a block, a multiple of tile
  int32_t n;     // blocks: they tile [0, total) and none is empty (0 for total = 0)
};

inline Blocks reduction_blocks(int64_t total, int64_t tile) {
  const int64_t span = tile * MAX_BLOCKS;
  Blocks b;
  b.per = tile * pcs_max64((total + span - 1) / span, 1);
  b.n = (int32_t)((total + b.per - 1) / b.per);
  return b;
}

// f(XT{}, YT{}) with the element types of the dtype pair: the template arguments of a launch
template <typename F>
void for_dtype_pair(int32_t xdtype, int32_t ydtype, F &&f) {
  if (xdtype == PCS_BF16 && ydtype == PCS_BF16) f(bf16_t{}, bf16_t{});
  else if (xdtype == PCS_BF16) f(bf16_t{}, float{});
  else if (ydtype == PCS_BF16) f(float{}, bf16_t{});
  else f(float{}, float{});
}

}  // namespace pcs_rows
