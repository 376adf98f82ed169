/* xvec_hip_nnet2.h - the part of the C ABI that nnet-am-compute (the nnet2 senone posteriors of the DNN i-vector path, DESIGN.md
 * section 3.13) adds to xvec_hip.h.  A header of its own beside xvec_hip.h, which it includes: the same library
 * (libxvec_hip.so), the same conventions (xv_status, xv_last_error(), host buffers in and out, device_ms optional).
 *
 *   xv_nnet2_open      reads an nnet2 acoustic model (final.mdl, binary or text; any rxfilename) and lowers it to layers.  Host
 *                      only: no device is opened before the first xv_nnet2_compute.  A file the reader refuses is XV_ERR_IO, and
 *                      xv_last_error() names the component.
 *   xv_nnet2_close     frees the model's host and device memory.  NULL is allowed.
 *   xv_nnet2_get_info  the model's dimensions: what xv_nnet2_plan needs and what nnet-am-info prints.
 *   xv_nnet2_plan      host only, pure: how a packed sequence of `rows` rows (the utterances with their padding, back to back)
 *                      passes through a device workspace of at most workspace_bytes (<= 0: the default, 256 MiB):
 *                      rows_per_block rows at a time - block_rows if > 0, else the most that fit, at most 2^20 -, n_blocks =
 *                      ceil(rows / rows_per_block) of them, block b being rows [b rows_per_block, min(rows, (b + 1)
 *                      rows_per_block)); every block carries left_context + right_context further rows of overlap.  bytes is what
 *                      gets allocated.  A workspace that does not hold the block is XV_ERR_ARG.  Outputs may be NULL.
 *   xv_nnet2_compute   the forward pass.  feats: [row_off[n_utts]][input_dim] fp32, utterance u being rows [row_off[u],
 *                      row_off[u + 1]).  flags: XV_NNET2_APPLY_LOG | XV_NNET2_DIVIDE_BY_PRIORS | XV_NNET2_PAD_INPUT.  out: fp32
 *                      [sum of the utterances' output rows][output_dim], where an utterance of T > 0 rows gives T rows with
 *                      XV_NNET2_PAD_INPUT and max(0, T - left_context - right_context) without it.  block_rows: as in
 *                      xv_nnet2_plan (<= 0: the default).  A row of the output is the same bits alone, in any batch and for
 *                      every block_rows.  XV_NNET2_DIVIDE_BY_PRIORS on a model without priors of the output dimension is
 *                      XV_ERR_ARG; no usable gfx950 device is XV_ERR_DEVICE.
 *   xv_nnet2_compute_layers  the same, and layer_ms[num_layers + 1]: the device time of every layer (the kernel that prepares its
 *                      input and its affine) and, last, of the head.
 * One launch each on caller data, for the unit tests of the kernels (csrc/nnet2_kernels.h):
 *   xv_nnet2_kernel_affine  out[t][j] = bias[j] + sum_c sum_i w[j][c k + i] x[t + context[c]][i]; rows of x outside [0, rows)
 *                      read as zero.  x [rows][k], w [n][n_ctx k], out [rows][n].  (The input-preparation launch splits x first.)
 *   xv_nnet2_kernel_row     pre [rows][in_dim] -> nonlin (0 none, 1 p-norm, 2 ReLU) -> normalize (if non-zero) -> the two fp16
 *                      planes hi, lo [rows][ld], ld = out_dim rounded up to 32, columns from out_dim on zero; the value is
 *                      hi + lo / 2048.
 *   xv_nnet2_kernel_head    logits [rows][n], n <= 16384 -> softmax, group sums (sizes [n_groups] summing to n, or NULL), times
 *                      1 / priors (or NULL), log (if apply_log) -> out [rows][n_groups or n]. */
#ifndef XVEC_HIP_NNET2_H_
#define XVEC_HIP_NNET2_H_

#include "xvec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xv_nnet2 xv_nnet2;

#define XV_NNET2_APPLY_LOG 1
#define XV_NNET2_DIVIDE_BY_PRIORS 2
#define XV_NNET2_PAD_INPUT 4

typedef struct xv_nnet2_info_t {
  int32_t num_components, num_updatable_components, left_context, right_context;
  int32_t input_dim, output_dim, softmax_dim, prior_dim;
  int32_t num_layers, max_plane_cols, max_pre_cols, halo;
  int64_t parameter_dim;
} xv_nnet2_info_t;

xv_status xv_nnet2_open(const char* model_rxfilename, xv_nnet2** out);
void xv_nnet2_close(xv_nnet2* m);
xv_status xv_nnet2_get_info(const xv_nnet2* m, xv_nnet2_info_t* info);
xv_status xv_nnet2_plan(const xv_nnet2_info_t* info, int64_t rows, int64_t block_rows, int64_t workspace_bytes, int64_t* rows_per_block,
                        int64_t* n_blocks, int64_t* bytes);
xv_status xv_nnet2_compute(xv_nnet2* m, int device, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t flags,
                           int64_t block_rows, float* out, float* device_ms);
xv_status xv_nnet2_compute_layers(xv_nnet2* m, int device, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t flags,
                                  int64_t block_rows, float* out, float* layer_ms);
xv_status xv_nnet2_kernel_affine(int device, const float* x, int32_t rows, int32_t k, const int32_t* context, int32_t n_ctx, const float* w,
                                 const float* bias, int32_t n, float* out);
xv_status xv_nnet2_kernel_row(int device, const float* pre, int32_t rows, int32_t in_dim, int32_t out_dim, int32_t nonlin, int32_t normalize,
                              uint16_t* hi, uint16_t* lo);
xv_status xv_nnet2_kernel_head(int device, const float* logits, int32_t rows, int32_t n, const int32_t* sizes, int32_t n_groups,
                               const float* priors, int32_t apply_log, float* out);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_HIP_NNET2_H_ */
