/*
 * The dense voxel U-Net's two kernels: an extension of the C ABI of pcs.h, declared in a header of its
 * own.  The entry points live in the same library (libpcs.so); PCS_ABI_VERSION is pcs.h's and does not
 * change with this header, which adds functions and touches no struct or existing signature.  The
 * binding reads it after pcs.h and pcs_segmax.h into a table of its own (pcs_amd/_lib.py,
 * DENSE_SIGNATURES; tests/golden/abi_tables_dense.json records the result).
 *
 * The two-source 3x3x3 stencil (csrc/conv3d.hip): pcs_conv3d / pcs_conv3d_wgrad on X = [XA | XB] along
 * channels, XA [B, D, H, W, CA] and XB [B, D, H, W, CB] bf16 channels-last, against the weight of the
 * layer on the concatenated array (W [Cout, 27, CA + CB] bf16); no [.., CA + CB] array is read, written
 * or kept.  Same k-step order, split geometry and workspace as the single-source layer at Cin = CA + CB,
 * so every result is bit-identical to it.  g is the geometry pcs_conv3d (pcs_conv3d_wgrad) would take on
 * the concatenated array and must be the stride-1 stencil: k == 3, s == 1 (either form).  CA, CB and the
 * other side's channel count are positive multiples of 32.
 * pcs_conv3d_cat: Y = conv(g; [XA | XB], W) + bias; g->Cin == CA + CB; Y [B, Do, Ho, Wo, g->Cout] in
 *   ydtype (PCS_F32 or PCS_BF16), bias f32 [g->Cout] or NULL.
 * pcs_conv3d_cat_dgrad: [dXA | dXB] = conv(g; dY, Wt), the input gradient of the layer: g is the other
 *   form of the forward's geometry with the grids and channel counts swapped (g->Cin = the forward's
 *   Cout, g->Cout == CA + CB), Wt = pcs_conv3d_weight_t of W, dY [.., g->Cin] bf16; dXA [.., CA] and
 *   dXB [.., CB] in xdtype.  An output tile may straddle the two arrays; a 4-channel store never does.
 * pcs_conv3d_cat_wgrad: dW f32 [g->Cout, 27, CA + CB] and db f32 [g->Cout] (NULL: skipped) of the
 *   forward geometry g (g->Cin == CA + CB) from dY bf16 [.., g->Cout]; workspace: at least
 *   pcs_conv3d_wgrad_workspace(g) bytes.
 *
 * pcs_dense_trilinear_index (csrc/pointvoxel.hip): pcs_trilinear_index for a dense num_scenes x grid^3
 * level, in which every in-grid cell is present and its row is (scene * grid + ix) * grid * grid +
 * iy * grid + iz: the same float32 expressions (u, the clamps, c, b, f), corner order and weights
 * renormalised over the present corners, without a hash table.  own [T] is therefore always >= 0 and a
 * corner is -1 only outside the grid.  num_scenes * grid^3 must be below 2^31 (rows are int32).
 * T == 0 returns 0 without a launch.
 *
 * Bad arguments return PCS_EINVAL (-1000) with a message naming the entry point, before any launch.
 */
#ifndef PCS_DENSE_H
#define PCS_DENSE_H
#include "pcs.h"

#ifdef __cplusplus
extern "C" {
#endif

int pcs_conv3d_cat(const pcs_conv3d_geom *g, const void *XA, int32_t CA, const void *XB, int32_t CB, const void *W,
                   const float *bias, void *Y, int32_t ydtype, pcs_stream_t stream);
int pcs_conv3d_cat_dgrad(const pcs_conv3d_geom *g, const void *dY, const void *Wt, void *dXA, int32_t CA, void *dXB,
                         int32_t CB, int32_t xdtype, pcs_stream_t stream);
int pcs_conv3d_cat_wgrad(const pcs_conv3d_geom *g, const void *XA, int32_t CA, const void *XB, int32_t CB,
                         const void *dY, void *workspace, int64_t workspace_bytes, float *dW, float *db,
                         pcs_stream_t stream);
int pcs_dense_trilinear_index(const float *points, const int64_t *offsets, int64_t num_scenes, int64_t T,
                              int32_t grid, float lo_x, float lo_y, float lo_z, float hi_x, float hi_y, float hi_z,
                              int32_t *own, int32_t *corner, float *weight, pcs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PCS_DENSE_H */
