/*
 * Segmented max on the occupied-voxel path: an extension of the C ABI of pcs.h, declared in a header
 * of its own.  The entry points live in the same library (libpcs.so); PCS_ABI_VERSION is pcs.h's and
 * does not change with this header, which adds functions and touches no struct or existing signature.
 * The binding reads it after pcs.h (pcs_amd/_lib.py, EXT_SIGNATURES; tests/golden/abi_tables_segmax.json
 * records the result).
 *
 * csrc/segmax.hip, the fused lift in csrc/pointhead.hip; build-defined, the numpy statement is
 * tests/segmax_refs.py: the max over a segment of rows with torch.max's pick, its backward, and the max
 * form of the point lift.  No atomics; every output row is stored exactly once; results are bitwise
 * reproducible.  A NaN in a gradient path is unspecified.
 * pcs_rows_segmax: for segment m and channel c, over j in [seg_off[m], seg_off[m + 1]) ascending with
 *   source row s = src[j] (src NULL: s = j; s < 0 skipped): the pick of torch.max over a dim, compared
 *   in fp32: a NaN beats every number, and among equal values (or among NaNs) the earliest j wins; the
 *   first present row always makes a pick (all -inf gives -inf).  Y[m][c] = the picked value (an f32
 *   to bf16 store rounds it once, to nearest even), arg[m][c] (i32 [M, C], may be NULL) = the picked
 *   s.  A segment without a present row stores Y = 0, arg = -1.  Source rows are int32: every s, and
 *   with src NULL every j, so seg_off[M], must be below 2^31 (seg_off lives on the device, so the
 *   call cannot check it).  seg_off [M + 1] i64 on the DEVICE;
 *   X [*, C], Y [M, C], each PCS_F32 or PCS_BF16; C % 8 == 0 when either side is bf16, else C % 4 == 0.
 * pcs_rows_argselect: dX[r][c] = (seg_of[r] >= 0 && arg[seg_of[r]][c] == r) ? dY[seg_of[r]][c] : 0 for
 *   the R source rows (R < 2^31): the backward of pcs_rows_segmax when a source row belongs to at most
 *   one segment (seg_of i32 [R], -1 = none).  dY [M, C], dX [R, C], dtypes and C as above.
 * pcs_point_lift_max: Y[v][c] = relu(max_{j in [seg_off[v], seg_off[v + 1])} z[j][c]) with z as
 *   pcs_point_lift_mean's (the same fma chain), the arguments of pcs_point_lift_mean without
 *   inv_count.  An empty segment stores a zero row; order[j] < 0 is skipped.
 * pcs_point_lift_max_bwd: with j* the first j of the largest z[j][c] of the segment, recomputed, and
 *   g[v][c] = z[j*][c] > 0 ? dV[v][c] : 0: dW[c][i] = sum_v g[v][c] * P[order[j*]][i]; db[c] = sum_v
 *   g[v][c] (db NULL: skipped).  The points get no gradient.  workspace: 16-byte aligned, at least
 *   pcs_point_lift_max_bwd_workspace(V, C, Cin) bytes.  C % 8 == 0, 8 <= C <= 1024; 1 <= Cin <= 8.
 * M == 0 / R == 0 / V == 0 return 0 without a launch.
 */
#ifndef PCS_SEGMAX_H
#define PCS_SEGMAX_H
#include "pcs.h"

#ifdef __cplusplus
extern "C" {
#endif

int pcs_rows_segmax(const void *X, int32_t xdtype, const int32_t *src, const int64_t *seg_off, int64_t M, int32_t C,
                    void *Y, int32_t ydtype, int32_t *arg, pcs_stream_t stream);
int pcs_rows_argselect(const void *dY, int32_t dydtype, const int32_t *arg, const int32_t *seg_of, int64_t R, int32_t C,
                       void *dX, int32_t dxdtype, pcs_stream_t stream);
int pcs_point_lift_max(const float *P, int64_t ldp, int32_t Cin, const float *W, const float *bias,
                       const int32_t *order, const int64_t *seg_off, int64_t V, int32_t C, void *Y, int32_t ydtype,
                       pcs_stream_t stream);
int64_t pcs_point_lift_max_bwd_workspace(int64_t V, int32_t C, int32_t Cin);
int pcs_point_lift_max_bwd(const void *dV, int32_t dvdtype, const float *P, int64_t ldp, int32_t Cin, const float *W,
                           const float *bias, const int32_t *order, const int64_t *seg_off, int64_t V, int32_t C,
                           void *workspace, int64_t workspace_bytes, float *dW, float *db, pcs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PCS_SEGMAX_H */
