// Device kernels of diagonal UBM training: the E-steps of gmm-global-acc-stats (sparse, on a Gaussian selection) and of
// gmm-global-init-from-feats (dense, every frame against every Gaussian).  Semantics in dubm_train.h.  Kept out of kernels.hip for
// the reason ubm_kernels.* are: KERNELS_SHA names the x-vector extraction kernels only.
//
// Scores.  A (frame, Gaussian) score is, in fp32 and bit for bit, what ubm_diag_gselect computes:
//   acc = gconst;  for d ascending:  acc = fmaf(v_d, fl(x_d x_d), fmaf(m_d, x_d, acc)),  m = mean / var, v = -1/2 / var
// on the vector ALU, from the transposed and padded arrays of a diagonal UbmModel.  The matrix-shaped form of the same chain
// (v_mfma_f32_16x16x4_f32 with K interleaved) was not built: there is one score form here, and no second one to compare.
// Accumulation.  Everything is fp64 on fp32 inputs: occ += p, mean += double(p) double(x) (exact product), var += double(p)
// (double(x) double(x)) (exact square).  No floating-point value goes through an atomic; partial sums per (Gaussian, chunk) are
// added in chunk order and that sum is added to the running accumulator once per call: what a call adds is a function of the call's
// frames, pairs and model alone.  The kernels of this file (kDgmmNumKernels in the object):
//   dgmm_sel_loglike    one thread per (frame, slot): the score of the selected Gaussian.
//   dgmm_acc_partial    the sparse accumulator.  The pairs are bucketed by Gaussian (launch_bucket_sort) and the work items
//                       (Gaussian, chunk of kFgmmAccPairChunk pairs of its bucket) are fgmm_acc_items' (ubm_train_kernels.h), whose
//                       contract fits as it is.  A workgroup walks its chunk in K tiles of kDgmmKTile pairs gathered into LDS;
//                       thread c < D sums column c of the mean, thread D + c column c of the second moment and thread 2 D the
//                       occupancy, pairs ascending.  2 D + 1 multiply-adds per pair: a gather-reduce on the vector ALU, no SYRK.
//   dgmm_dense_logsum   a workgroup owns kDgmmLogsumFrames frames, stages (x, fl(x x)) in LDS once and walks all Gaussians in tiles
//                       of kDgmmLogsumGaussTile twice: first the exact maximum per frame, then sum_g expf(s_g - max) with the running
//                       sums in fp64.  Thread (Gaussian of the tile, half of the frames) sums over the tiles in ascending order; the
//                       kDgmmLogsumGaussTile sums of a frame are then added in ascending order by one thread: the order depends on the
//                       number of Gaussians alone.  logsum = float(double(max) + log(sum)).
//   dgmm_dense_acc      the hot kernel.  Workgroup (tile of kDgmmGaussTile Gaussians, chunk of kDgmmDenseFrameChunk frames); wave w owns
//                       Gaussians 16 w .. 16 w + 15 of the tile and every column tile of [X | X o X | 1].  Per K tile of kDgmmDenseKTile
//                       frames: the frames are staged in LDS once, as fp32 (x and fl(x x)); thread (Gaussian, quarter of the frames)
//                       recomputes the scores, p = expf(s - logsum_t) goes to LDS (rows beyond G and frames beyond the chunk as 0,
//                       set in registers); then P' [X | X o X | 1] on v_mfma_f64_16x16x4_f64 in ascending k: A = double(p), B =
//                       double(x), double(x) double(x) or 1, columns beyond 2 D + 1 zero, built in registers from the staged fp32
//                       frames.  f64 fragment maps as in ivex_kernels.h (A [lane & 15][k = lane >> 4], B [k = lane >> 4][lane & 15],
//                       C col = lane & 15, row = (lane >> 4) + 4 reg).  The occupancy is the column of ones: at D = 60 the 121 columns
//                       pad to 128 anyway; whenever 2 D is a multiple of 16 (D = 96) it costs a thirteenth column tile, 1 / 12 more
//                       matrix work, which buys one summation order for all three statistics and no second reduction path.
//                       With `post` set the scores are skipped and p = post[t][g]: the accumulation alone, for one-launch tests.
//                       Three instances, by the number of column tiles (4, 8, 13).
//   dgmm_acc_reduce     thread (Gaussian, element): the Gaussian's partial sums added in chunk order, that sum added to the running
//                       accumulator once.  Serves both paths; the flags gate what is added (occ always).
// No kernel uses scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ubm_train_kernels.h"

namespace xv {

constexpr int kDgmmThreads = 256;
constexpr int kDgmmMaxDim = 96;                // the largest feature dimension
constexpr int kDgmmKTile = 64;                 // pairs gathered into LDS at a time by the sparse accumulator
constexpr int kDgmmAccFrameBlock = 16384;      // frames per accumulate call of gmm-global-acc-stats
constexpr int kDgmmLogsumFrames = 32;          // frames per workgroup of dgmm_dense_logsum
constexpr int kDgmmLogsumGaussTile = 128;      // Gaussians per pass of that workgroup (the padding of a diagonal UbmModel)
constexpr int kDgmmGaussTile = 64;             // Gaussians per workgroup of dgmm_dense_acc
constexpr int kDgmmDenseKTile = 32;            // frames staged at a time by dgmm_dense_acc (a multiple of 4)
constexpr int kDgmmDenseFrameChunk = 4096;     // frames per workgroup of dgmm_dense_acc (a multiple of kDgmmDenseKTile)
constexpr int kDgmmNumKernels = 7;             // dgmm_dense_acc has three instances and each of the other four kernels one

// The diagonal model as a UbmModel keeps it on the device (ubm_kernels.h: UbmDiagArgs).
struct DgmmModelArgs {
  int dim, num_gauss, gauss_pad;
  const float* m_t;      // [dim][gauss_pad]  means / variances
  const float* v_t;      // [dim][gauss_pad]  -1/2 / variances
  const float* gconst;   // [gauss_pad]
};

struct DgmmSelArgs {
  DgmmModelArgs model;
  const float* feats;       // [rows][dim]
  int64_t rows;
  int n;
  const int32_t* gselect;   // [rows][n], every entry in [0, num_gauss) (the host checks)
  float* ll;                // [rows][n]
};

struct DgmmDenseArgs {
  DgmmModelArgs model;      // dense_acc with `post`: only dim and num_gauss are read
  const float* feats;       // [rows][dim]
  int64_t rows;
  float* logsum;            // [rows]: written by dense_logsum, read by dense_acc
  const float* post;        // [rows][num_gauss] or null
  int num_chunks;           // ceil(rows / kDgmmDenseFrameChunk)
  double* partial;          // [num_gauss][num_chunks][1 + 2 dim]
};

// The reduction of both paths.  item_start != null: Gaussian g owns the partial sums item_start[g] .. item_start[g + 1] (sparse);
// null: g * num_chunks .. (g + 1) * num_chunks (dense).
struct DgmmReduceArgs {
  int dim, num_gauss, flags;
  const int32_t* item_start;
  int num_chunks;
  const double* partial;    // [items][1 + 2 dim]: occ, mean [dim], second moment [dim]
  double* occ;              // [num_gauss]
  double* mean;             // [num_gauss][dim]
  double* var;              // [num_gauss][dim]
};

hipError_t launch_dgmm_sel_loglike(const DgmmSelArgs& a, hipStream_t s);
// The sparse accumulator on FgmmAccArgs (item_start filled by launch_fgmm_acc_items): partial is [num_items][1 + 2 dim] here and
// a.cov is the second moment [num_gauss][dim].  Partial sums, then the reduction.
hipError_t launch_dgmm_acc(const FgmmAccArgs& a, hipStream_t s);
hipError_t launch_dgmm_dense_logsum(const DgmmDenseArgs& a, hipStream_t s);
hipError_t launch_dgmm_dense_acc(const DgmmDenseArgs& a, hipStream_t s);   // the partial sums only
hipError_t launch_dgmm_acc_reduce(const DgmmReduceArgs& a, hipStream_t s);

}  // namespace xv
