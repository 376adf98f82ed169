// Device kernels of full-covariance UBM training: the accumulator of fgmm-global-acc-stats (semantics in ubm_train.h).  Kept out of
// kernels.hip for the reason ubm_kernels.* are: KERNELS_SHA names the x-vector extraction kernels only.
//
// fgmm_acc adds one call's posterior-weighted moments into persistent fp64 accumulators: occ [G], mean [G][D] and the packed
// lower triangles cov [G][D (D + 1) / 2].  It gets the call's frames [rows][D] in fp32 and the pairs (frame, Gaussian, p) bucketed
// by Gaussian, frames ascending inside a bucket (launch_bucket_sort of bucket_sort.h, one segment: a pair's bucket is its Gaussian's).
// Everything is fp64 on fp32 inputs; no floating-point value goes through an atomic, and every sum has an order that is a
// function of the call's pairs alone.
//   fgmm_acc_items      one workgroup: item_start[g] = the exclusive prefix sums of ceil(bucket_g / kFgmmAccPairChunk), the work
//                       items (Gaussian, chunk of its bucket) of the next kernel.  Integer work only.
//   fgmm_acc_partial    one workgroup per item.  The grid is the host's bound on their number: the workgroups beyond
//                       item_start[G] leave at once, and no count is read back.  A workgroup finds its Gaussian by bisection of
//                       item_start.  The chunk is walked in K tiles of kFgmmAccKTile pairs: the pairs' weights and their frames
//                       (zero for a pair whose weight is 0) are gathered into LDS once per K tile, as fp32, and feed every
//                       output tile.
//                         second moment   a weighted SYRK on v_mfma_f64_16x16x4_f64: A[i][k] = double(p_k) * double(x_k[i]), which
//                                         is exact (24 bits times 24 bits), B[k][j] = double(x_k[j]).  Only the tiles on and below
//                                         the diagonal of the ceil(D / 16)^2 grid exist; wave w owns tiles w, w + 4, ... (at most
//                                         6 accumulators of 4 doubles).  A k step reads one fragment per tile row from LDS and
//                                         every tile of the wave takes its A and B operand from those registers.  Rows and
//                                         columns beyond D and k beyond the chunk are masked to zero in registers.  f64
//                                         fragment maps as in ivex_kernels.h.
//                         mean, occupancy summed on the vector ALU, as ivex_stats does, not as an extra column of ones: thread
//                                         255 - d owns column d and thread 255 - D the occupancy, k ascending: the columns sit
//                                         on the last waves, which own the fewest tiles (at D = 60 wave 3 alone, with 2 of the
//                                         10 tiles).  Dealing the columns over all four waves was measured and is slower: every
//                                         wave then pays the serial loop over the K tile.  (A
//                                         column of ones would cost a seventh row of tiles at D = 96 for D + 1 useful numbers.)
//                       The sums of the item go to partial[item][1 + D + D (D + 1) / 2].
//   fgmm_acc_reduce     thread (Gaussian, element): the Gaussian's partial sums added in chunk order, and that sum added to the
//                       running accumulator once.  Gaussians with empty buckets are not touched.
// The flags (m = 1, v = 2, w = 4, already augmented: v implies m) say which of mean and cov exist; occ always does.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace xv {

constexpr int kFgmmAccThreads = 256;
constexpr int kFgmmAccPairChunk = 1024;     // pairs of one bucket per workgroup
constexpr int kFgmmAccKTile = 64;           // pairs gathered into LDS at a time (a multiple of 4)
constexpr int kFgmmAccFrameBlock = 16384;   // frames per accumulate call of fgmm-global-acc-stats
constexpr int kFgmmAccMaxDim = 96;          // the largest feature dimension
constexpr int kFgmmFlagMeans = 1, kFgmmFlagVariances = 2, kFgmmFlagWeights = 4;

struct FgmmAccArgs {
  const float* feats;            // [rows][dim]
  int64_t rows;
  int dim, num_gauss, flags;
  int64_t pairs;
  const int32_t* pair_frame;     // [pairs] row of feats, or null: pair / n
  int n;
  const float* pair_w;           // [pairs]
  const int32_t* sorted;         // [pairs] pair indices, bucket after bucket
  const int32_t* bucket_start;   // [num_gauss + 1]
  int32_t* item_start;           // [num_gauss + 1]
  int num_items;                 // the grid: pairs / kFgmmAccPairChunk + min(num_gauss, pairs), a bound on item_start[num_gauss]
  double* partial;               // [num_items][1 + dim + dim (dim + 1) / 2]
  double* occ;                   // [num_gauss]
  double* mean;                  // [num_gauss][dim]
  double* cov;                   // [num_gauss][dim (dim + 1) / 2]
};

hipError_t launch_fgmm_acc_items(const FgmmAccArgs& a, hipStream_t s);
hipError_t launch_fgmm_acc(const FgmmAccArgs& a, hipStream_t s);   // partial sums, then the reduction

}  // namespace xv
