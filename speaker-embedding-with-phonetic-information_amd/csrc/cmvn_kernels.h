// Device kernels of per-speaker cepstral mean and variance normalisation (compute-cmvn-stats / apply-cmvn; semantics in cmvn.h).
// Kept out of kernels.hip for the reason compress_kernels.* are: KERNELS_SHA names the extraction kernels only.
//
// A launch works on a ragged batch of row-major fp32 matrices that share a column count: packed rows plus row_off[n + 1].  The
// host (cmvn.cc) cuts every matrix into blocks of kCmvnRowBlock rows and lists them as work items (matrix, block), matrix after
// matrix, block after block; a launch takes the list, so there is one launch per kernel and batch whatever n is.
//   cmvn_stats_partial  one workgroup per item: the sum and the sum of squares of every column over the block's rows, in fp64, from
//                       one read of each element.  Thread (j, c) of a column tile adds rows j, j + R, j + 2 R, ... of column c in
//                       that order (R = kCmvnThreads / tile width rows are in flight at once: consecutive lanes read consecutive
//                       addresses), then the R sums of a column are added in ascending j.
//   cmvn_stats_reduce   one thread per (matrix, column): the block partials added in ascending block order, and the count slot.
//                       No floating-point atomics anywhere: the order of every sum is a function of the matrix's number of rows
//                       and columns alone, so a matrix's statistics are the same bits in whatever batch it lands.
//   cmvn_apply          out = x * scale + offset per item, the norm of matrix u being row utt_norm[u] of the table.  fp32, the
//                       product and the sum each rounded on their own (the file is compiled with contraction off).
//   cmvn_apply_select   (cmvn_select_kernel.hip) the same map behind a row selection, for the front-end of nnet3-compute (fuse_pipe.h): out[i] = raw[sel_row[i]]
//                       * scale + offset with the norm of utterance sel_utt[i]; one launch, one thread per kept element.  A kept
//                       row is bit for bit what cmvn_apply writes for it: selection commutes with an element-wise map.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace xv {

constexpr int kCmvnThreads = 256;
constexpr int kCmvnRowBlock = 256;   // rows per work item
constexpr int kCmvnColTile = 256;    // columns per pass of a workgroup (wider matrices: several passes)

struct CmvnArgs {
  const float* feats;          // [row_off[n]][cols]
  const int32_t* row_off;      // [n + 1]
  int n, cols;
  const int32_t* item_mat;     // [n_items] work items: the matrix ...
  const int32_t* item_blk;     // ... and its row block
  int n_items;
  // statistics
  const int32_t* mat_item0;    // [n + 1] first item of every matrix (matrix u owns items mat_item0[u] .. mat_item0[u + 1] - 1)
  double* partial;             // [n_items][2][cols]
  double* stats;               // [n][2][cols + 1]
  // normalisation
  const float* norms;          // [n_norms][2][cols]: row 0 the offset, row 1 the scale
  const int32_t* utt_norm;     // [n] the norm of every matrix, in [0, n_norms)
  float* out;                  // [row_off[n]][cols]
};

constexpr int kCmvnSelectRows = 64;   // output rows per workgroup of cmvn_apply_select

// sel_row / sel_utt as FrontEndArgs (kernels.h) has them.  The kernel checks nothing: every sel_row is a row of raw, every
// sel_utt an utterance whose utt_norm is a row of norms (utterances without statistics are filtered out by the host).
struct CmvnSelectArgs {
  const float* raw;            // [raw rows][cols]
  int cols;                    // >= 1
  const float* norms;          // [n_norms][2][cols]: row 0 the offset, row 1 the scale
  const int32_t* utt_norm;     // [n_utts] in [0, n_norms)
  const int32_t* sel_row;      // [n_out] absolute raw row of every kept frame
  const int32_t* sel_utt;      // [n_out] its utterance
  int n_out;
  float* out;                  // [n_out][cols]
};

hipError_t launch_cmvn_stats(const CmvnArgs& a, hipStream_t s);    // partial + reduce
hipError_t launch_cmvn_apply(const CmvnArgs& a, hipStream_t s);
hipError_t launch_cmvn_apply_select(const CmvnSelectArgs& a, hipStream_t s);   // n_out == 0: nothing to do

}  // namespace xv
