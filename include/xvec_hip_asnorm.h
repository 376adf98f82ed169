/* xvec_hip_asnorm.h - the part of the C ABI that adaptive score normalisation (AS-norm) adds to
 * xvec_hip.h: the PLDA log-likelihood ratio of all pairs of two tables, the statistics of each row's N largest scores, the
 * two fused, and the plan of the fused path.  A header of its own beside xvec_hip.h, which it includes: the same library
 * (libxvec_hip.so), the same conventions (xv_status, xv_last_error(), host buffers in and out, device_ms optional).  It
 * continues the PLDA back-end section of xvec_hip.h, after xv_plda_score.
 *
 * Device kernels behind host buffers, fp64 arithmetic on fp32 vectors, deterministic (fixed reduction orders, no float
 * atomics).  Sizes and N out of range are XV_ERR_ARG; the device entries fail with XV_ERR_DEVICE when no gfx950 device is
 * usable.
 *   xv_plda_score_dense  the same ratio for EVERY pair: scores[i][j] (fp64, [n_u][n_v]) of enrolment row i against test
 *                      row j, as one fp64 matrix product on the matrix cores.  A score is a function of its pair and psi
 *                      alone: the same bits wherever the pair sits in whichever tables.  n_u == 0 or n_v == 0 writes
 *                      nothing.  dim <= 512.
 *   xv_topn_stats      per row of scores [rows][cols] (finite values): the n largest values - exactly; among values equal to
 *                      the n-th largest, the lowest columns - their mean[row] and population standard deviation std[row]
 *                      (two passes).  -0 counts as +0.  A row's result is the same bits alone and in any batch.
 *                      2 <= n <= cols <= 1048576 (kTopnMaxCols), else XV_ERR_ARG.
 *   xv_plda_cohort_stats  xv_topn_stats of xv_plda_score_dense without the matrix leaving the device, bit for bit:
 *                      by_column == 0: mean / std [n_u], per row of u over all rows of v; by_column != 0: [n_v], per row
 *                      of v over all rows of u.  The matrix exists one chunk of rows at a time (xv_plda_dense_plan).
 *   xv_plda_dense_plan host only, pure: how a rows x cols score matrix passes through a device workspace of at most
 *                      workspace_bytes (<= 0: the default, 256 MiB): rows_per_chunk rows at a time (the most that fit; a
 *                      multiple of the kernel's 64-row tile from 64 on), n_chunks = ceil(rows / rows_per_chunk) of them,
 *                      chunk c being rows [c rows_per_chunk, min(rows, (c + 1) rows_per_chunk)); chunk_bytes is what gets
 *                      allocated.  A workspace that does not hold one row is XV_ERR_ARG.  Outputs may be NULL. */
#ifndef XVEC_HIP_ASNORM_H_
#define XVEC_HIP_ASNORM_H_

#include "xvec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

xv_status xv_plda_score_dense(int device, const float* u, const double* num_u, int32_t n_u, const float* v, int32_t n_v, int32_t dim,
                              const double* psi, double* scores, float* device_ms);
xv_status xv_topn_stats(int device, const double* scores, int64_t rows, int32_t cols, int32_t n, double* mean, double* std,
                        float* device_ms);
xv_status xv_plda_cohort_stats(int device, const float* u, const double* num_u, int32_t n_u, const float* v, int32_t n_v, int32_t dim,
                               const double* psi, int32_t by_column, int32_t n, double* mean, double* std, float* device_ms);
xv_status xv_plda_dense_plan(int64_t rows, int64_t cols, int32_t dim, int64_t workspace_bytes, int64_t* rows_per_chunk,
                             int64_t* n_chunks, int64_t* chunk_bytes);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_HIP_ASNORM_H_ */
