/*
 * Inference entry points of the voxel U-Nets: the forward convolutions with an eval-mode BatchNorm
 * (+ residual) (+ ReLU) folded into their store.  An extension of the C ABI of pcs.h, declared in a header
 * of its own: the entry points live in the same library (libpcs.so); PCS_ABI_VERSION is pcs.h's and does
 * not change with this header, which adds functions and touches no struct or existing signature.  The
 * binding reads it after pcs.h, pcs_segmax.h and pcs_dense.h into a table of its own (pcs_amd/_lib.py,
 * FOLD_SIGNATURES; tests/golden/abi_tables_fold.json records the result).
 *
 * Each pcs_X_affine is pcs_X (pcs.h; pcs_conv3d_cat: pcs_dense.h) with one more step where the kernel
 * stores a row (csrc/conv3d.hip, EpiAffine): with acc the convolution's fp32 sum of channel c of row r,
 *
 *     v       = acc[r][c] (+ bias[c], as pcs_X)
 *     Y[r][c] = act( fmaf(v, scale[c], shift[c]) (+ R[r][c]) ),   act = relu != 0 ? max(., 0) : identity
 *
 * in fp32, rounded once to Y's dtype.  This is pcs_sparse_bn_apply's statement in its operation order (one
 * fused multiply-add, then the residual's own add; a NaN propagates through the ReLU), so the result is
 * bit-identical to pcs_X with an fp32 Y followed by pcs_sparse_bn_apply on that array, without the array:
 * no [rows, Cout] intermediate is written or read, and the sums are rounded once instead of twice.  With
 * scale / shift from pcs_bn_eval_coefs it is the layer convolution -> BatchNorm in eval mode (+ residual)
 * (+ ReLU) of pcs_amd.fold.
 *
 * The arguments before scale are pcs_X's, with pcs_X's meaning, checks and routes (the same kernels, tiles
 * and summation order: only the store differs); the stream stays last.  Then:
 *   scale, shift  f32 [Cout] on the device, required (Cout: the channel count of Y)
 *   R             NULL, or the residual: an array of Y's shape, dtype (ydtype) and row indexing, 16-byte
 *                 aligned; it is read in the vector width Y is written in and may not alias Y
 *   relu          0 or not 0
 * No entry point allocates; every launch is on the given stream; M == 0 (the sparse forms) returns 0
 * without a launch.  Bad arguments return PCS_EINVAL (-1000) with a message naming the entry point, before
 * any launch.  The forward only: there is no gradient of a folded layer.
 */
#ifndef PCS_FOLD_H
#define PCS_FOLD_H
#include "pcs.h"

#ifdef __cplusplus
extern "C" {
#endif

int pcs_sparse_conv_affine(const int32_t *nbr, int64_t M, int32_t taps, const void *X, int32_t Cin, const void *W,
                           int32_t Cout, const float *bias, void *Y, int32_t ydtype, int32_t flip, const float *scale,
                           const float *shift, const void *R, int32_t relu, pcs_stream_t stream);
int pcs_sparse_conv_pairs_affine(const int32_t *pair_in, const int32_t *pair_pos, const int64_t *tap_off, int32_t taps,
                                 int64_t M, const void *X, int32_t Cin, const void *W, int32_t Cout, const float *bias,
                                 float *Z, void *Y, int32_t ydtype, int32_t flip, const float *scale,
                                 const float *shift, const void *R, int32_t relu, pcs_stream_t stream);
int pcs_sparse_conv_rows_affine(const int32_t *pair_in, const int32_t *pair_out, const int64_t *tap_off, int32_t taps,
                                int64_t M, const void *X, int32_t Cin, const void *W, int32_t Cout, const float *bias,
                                void *Y, int32_t ydtype, const float *scale, const float *shift, const void *R,
                                int32_t relu, pcs_stream_t stream);
int pcs_sparse_conv_cat_affine(const int32_t *nbr, int64_t M, int32_t taps, const void *XA, int32_t CA, const void *XB,
                               int32_t CB, const void *W, int32_t Cout, const float *bias, void *Y, int32_t ydtype,
                               int32_t flip, const float *scale, const float *shift, const void *R, int32_t relu,
                               pcs_stream_t stream);
int pcs_sparse_conv_cat_pairs_affine(const int32_t *pair_in, const int32_t *pair_pos, const int64_t *tap_off,
                                     int32_t taps, int64_t M, const void *XA, int32_t CA, const void *XB, int32_t CB,
                                     const void *W, int32_t Cout, const float *bias, float *Z, void *Y, int32_t ydtype,
                                     int32_t flip, const float *scale, const float *shift, const void *R,
                                     int32_t relu, pcs_stream_t stream);
int pcs_conv3d_affine(const pcs_conv3d_geom *g, const void *X, const void *W, const float *bias, void *Y,
                      int32_t ydtype, const float *scale, const float *shift, const void *R, int32_t relu,
                      pcs_stream_t stream);
int pcs_conv3d_cat_affine(const pcs_conv3d_geom *g, const void *XA, int32_t CA, const void *XB, int32_t CB,
                          const void *W, const float *bias, void *Y, int32_t ydtype, const float *scale,
                          const float *shift, const void *R, int32_t relu, pcs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PCS_FOLD_H */
