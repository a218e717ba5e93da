// Device primitives of the hand-scheduled kernels: the XCD block remap, LDS-DMA (global_load_lds)
// statements with their M0 handling, counted waits and raw barriers fenced against the
// scheduler, transposed LDS fragment reads, and the few layout / unpack helpers several kernels
// share.  Included only by the kernel files that use them -- not from common.h: an M0-clobbering
// DMA statement must not be reachable by accident.  One definition each: no .hip file defines a
// function of these names (tests/test_csrc_helpers.py), and a change here has to leave every
// file's device code as intended (tools/asm_equal.py compares it against a revision).
#pragma once
#include "common.h"

typedef __attribute__((address_space(3))) void lds_void_t;
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) v2i lds_v2i;

// bijective XCD-grouping remap of the linear block id: workgroups bid, bid + 8, ... (one XCD's,
// sharing its L2) get consecutive logical ids
PCS_DEV int xcd_remap(int bid, int nb) {
  const int q = nb >> 3, r = nb & 7, x = bid & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

// ---- scheduling fences, counted waits, barriers ---------------------------------------------
// hipcc moves nothing across sbar(); each wait / barrier below sits between two of them so that
// the MFMAs and LDS reads around it stay on the side the kernel's pipeline put them (the "memory"
// clobber alone orders only memory accesses).
PCS_DEV void sbar() { __builtin_amdgcn_sched_barrier(0); }
// wait until at most N of this wave's vector-memory operations (DMA pieces, loads, stores: they
// retire in issue order) are outstanding
template <int N> PCS_DEV void wait_vm() {
  sbar();
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
  sbar();
}
PCS_DEV void wait_lgkm0() {
  sbar();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  sbar();
}
// s_barrier alone: the caller has already waited (wait_vm / wait_lgkm0) for what it hands over
PCS_DEV void barrier_raw() {
  sbar();
  asm volatile("s_barrier" ::: "memory");
  sbar();
}
// common.h's lds_barrier() between two scheduling fences: for the pipelined kernels, where the
// barrier also separates MFMA phases.  A kernel without a hand-placed instruction order uses
// lds_barrier().
PCS_DEV void barrier_lds() {
  sbar();
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  sbar();
}

// ---- LDS-DMA: one piece = 64 lanes x 16 B (glds16*) or 4 B (glds4o) from sbase + voff (per
// lane) to consecutive LDS bytes from the address in M0.  Inline asm so that the compiler's own
// wait insertion neither drains these loads before unrelated LDS reads nor spills their 64-bit
// addresses: the kernel counts them itself (wait_vm).
// glds16, glds16o and glds4o set M0 and do NOT restore it, and hipcc does not know (M0 is no
// clobber it tracks).  So the caller either brackets a run of them with m0_save() /
// m0_restore(), or its file is listed in M0_FILES of tests/test_asm_audit.py, which checks that
// no compiler-generated instruction of that file touches M0.  glds16_keep_m0 needs neither.
PCS_DEV uint32_t m0_save() {
  uint32_t k;
  asm volatile("s_mov_b32 %0, m0" : "=s"(k));
  return k;
}
PCS_DEV void m0_restore(uint32_t k) { asm volatile("s_mov_b32 m0, %0" ::"s"(k)); }
// LDS destination m0base + OFF (OFF a compile-time byte offset): clobbers M0
template <int OFF> PCS_DEV void glds16o(const char *sbase, uint32_t voff, uint32_t m0base) {
  asm volatile("s_add_u32 m0, %2, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
               :: "v"(voff), "s"(sbase), "s"(m0base), "n"(OFF) : "memory", "scc");
}
template <int OFF> PCS_DEV void glds4o(const char *sbase, uint32_t voff, uint32_t m0base) {
  asm volatile("s_add_u32 m0, %2, %3\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1"
               :: "v"(voff), "s"(sbase), "s"(m0base), "n"(OFF) : "memory", "scc");
}
// LDS destination lds_dst + 16 * lane: clobbers M0
PCS_DEV void glds16(const char *sbase, uint32_t voff, char *lds_dst) {
  const uint32_t m0v = (uint32_t)(uintptr_t)(lds_void_t *)lds_dst;
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
               :: "v"(voff), "s"(sbase), "s"(m0v)
               : "memory");
}
// the same piece with M0 saved and restored inside the statement (two more scalar moves per piece)
PCS_DEV void glds16_keep_m0(const char *sbase, uint32_t voff, char *lds_dst) {
  const uint32_t m0v = (uint32_t)(uintptr_t)(lds_void_t *)lds_dst;
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(sbase), "s"(m0v)
               : "memory");
}

// ---- LDS layouts and fragment reads ------------------------------------------------------------
// row permutation (bits 2 <-> 3 swapped) of the padded row-major tiles read by ds_read_b64_tr_b16:
// the eight rows one transposed read touches land on eight distinct bank groups
PCS_DEV int prow(int r) { return (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1); }
// 16-B slot permutation of the streamed dz5 rows: chunk c of row r sits at slot c ^ ftr(r)
PCS_DEV int ftr(int row) { return ((row & 3) << 1) | (row & 8); }
// one bf16 MFMA operand (k = 8 rows of one column per lane) from two transposed reads of 4 rows
PCS_DEV bf16x8 tr_frag2(const char *p0, const char *p1) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)p0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)p1);
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}
// split coefficient layout: elements 0-3 of every chunk first, then elements 4-7
PCS_DEV int split_idx(int i, int n) { return ((i & 7) >> 2) * (n / 2) + (i >> 3) * 4 + (i & 3); }
// the two bf16 halves of a packed pair as floats
PCS_DEV float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
PCS_DEV float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
// 8 consecutive per-channel floats from LDS (two 16-B reads)
PCS_DEV void lds_vec8(const float *p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4 *>(p);
  const float4 b = *reinterpret_cast<const float4 *>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
