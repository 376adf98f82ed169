// Device kernels of the GMM-UBM stage of the i-vector baseline (add-deltas, gmm-gselect, fgmm-global-gselect-to-post; semantics in
// ubm.h).  Kept out of kernels.hip for the reason cmvn_kernels.* are: KERNELS_SHA names the extraction kernels only.
//
// Everything is fp32 products with fp32 accumulation on the vector ALU; no matrix-core path is built (none has been measured).
// Every sum has an order that is a function of the frame and the model alone, and no floating-point value goes through an
// atomic: a frame's results are the same bits in whatever batch it lands.
//   add_deltas          one workgroup per (matrix, block of kDeltaRowBlock rows); compiled with contraction off: the product and the
//                       sum of every tap are rounded on their own.
//   ubm_diag_gselect    a workgroup owns kUbmFrameBlock frames, stages (x, x * x) of them in LDS once and walks the Gaussians in
//                       tiles of kUbmGaussTile: thread (Gaussian of the tile, half of the frames) adds gconst + sum_d (m x + v x^2)
//                       in ascending d.  The tile's scores go to LDS; per frame one wave keeps what beats the frame's current n-th
//                       best and ranks the survivors together with the running list (order: score descending, then index
//                       ascending; scores compared as order-preserving integer keys of score + 0, so the two zeros are equal and
//                       the order is total even with NaNs).  The frames x Gaussians score matrix never leaves the workgroup.
//                       n <= kUbmMaxSelect.
//   ubm_full_loglike    reads the rows * n (frame, slot) pairs bucketed by Gaussian, ascending pair inside a bucket (bucket_sort.h).
//                       Workgroup (g, s) expands Gaussian g's packed inverse covariance into LDS and takes tiles s, s + S, ... of
//                       kUbmFullFrameTile frames of g's bucket: thread (frame, column group) forms y_j = sum_i x_i A_ij in ascending
//                       i for its columns, then its share of b . x - x . y / 2; the 8 shares are added in ascending group order
//                       to gconst and scattered back to (frame, slot).
//   ubm_post            one thread per frame: softmax over the n log-likelihoods, the min-post rule, compaction.  A frame whose
//                       largest log-likelihood is not finite gets count 0, slot posteriors of 0 and that value as its log-sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace xv {

constexpr int kUbmThreads = 256;
constexpr int kUbmFrameBlock = 32;      // frames per workgroup of the selection kernel
constexpr int kUbmGaussTile = 128;      // Gaussians per pass of that workgroup
constexpr int kUbmMaxSelect = 64;       // the largest n
constexpr int kUbmMaxDim = 96;          // the largest feature dimension of a model on the device
constexpr int kUbmFullFrameTile = 32;   // frames per pass of the full-covariance kernel
constexpr int kUbmFullGroups = 8;       // column groups of that kernel (kUbmThreads / kUbmFullFrameTile)
constexpr int kDeltaRowBlock = 256;     // rows per work item of add_deltas
constexpr int kDeltaMaxOrder = 8;

struct DeltaArgs {
  const float* feats;        // [row_off[n]][in_stride]; the first dim columns are used (--truncate)
  int in_stride, dim;
  const int32_t* row_off;    // [n + 1]
  int n;
  int order, window;
  const float* scales;       // the scales of orders 0 .. order back to back; order i has 2 i window + 1 of them
  int scale_off[kDeltaMaxOrder + 2];
  const int32_t* item_mat;   // [n_items] work items: the matrix ...
  const int32_t* item_blk;   // ... and its row block
  int n_items;
  float* out;                // [row_off[n]][(order + 1) dim]
};

struct UbmDiagArgs {
  const float* feats;   // [rows][dim]
  int64_t rows;
  int dim;
  int num_gauss, gauss_pad;   // gauss_pad: num_gauss rounded up to kUbmGaussTile; the arrays below are padded with zeros
  const float* m_t;           // [dim][gauss_pad]  means * inverse variances
  const float* v_t;           // [dim][gauss_pad]  -0.5 * inverse variances
  const float* gconst;        // [gauss_pad]
  int n;                      // 1 <= n <= min(kUbmMaxSelect, num_gauss)
  int32_t* out_idx;           // [rows][n] descending log-likelihood
  float* out_ll;              // [rows][n] or null
};

struct UbmFullArgs {
  const float* feats;   // [rows][dim]
  int64_t rows;
  int dim;
  int num_gauss;
  const float* inv_covars;   // [num_gauss][dim (dim + 1) / 2] packed lower triangles
  const float* lin;          // [num_gauss][dim] inverse covariance times mean
  const float* gconst;       // [num_gauss]
  int n;                     // pairs per frame
  const int32_t* gselect;    // [rows * n] the Gaussian of every pair, each in [0, num_gauss) (the host checks)
  // the pairs sorted by Gaussian (bucket_sort.h, one segment)
  const int32_t* bucket_start;   // [num_gauss + 1]
  const int32_t* sorted;         // [rows * n] pair indices, bucket after bucket
  int split;                 // workgroups per Gaussian of the full-covariance kernel
  float* ll;                 // [rows * n]
  // posteriors
  float min_post;
  int32_t* out_count;        // [rows]
  int32_t* out_idx;          // [rows][n] the first out_count[t] are set
  float* out_post;           // [rows][n]
  float* out_logsum;         // [rows] or null
  float* out_slot_post;      // [rows][n] or null: the same posteriors where the selection has them, zeros kept (ubm_train.h)
};

hipError_t launch_add_deltas(const DeltaArgs& a, hipStream_t s);
hipError_t launch_ubm_diag_gselect(const UbmDiagArgs& a, hipStream_t s);
hipError_t launch_ubm_full_loglike(const UbmFullArgs& a, hipStream_t s);
hipError_t launch_ubm_post(const UbmFullArgs& a, hipStream_t s);

}  // namespace xv
