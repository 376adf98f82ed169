// Device kernels of nnet-am-compute (semantics in nnet2.h).  A file of their own beside kernels.hip, for the
// reason post_kernels.* are: KERNELS_SHA names the extraction kernels only.
//
// Activations live on the device as two planes of fp16, rows of `ld` halves (ld a multiple of 32, the columns from the width to
// ld zero): hi = fp16(x) and lo = fp16((x - hi) * 2^11), so x ~ hi + lo 2^-11 to 22 bits wherever |x| >= 2^-14, and to
// 2^-36 absolutely below that.  |x| must stay below 65504 (a larger value becomes an infinity, and shows as one).  Weights are
// split the same way on the host after a power-of-two scale that brings the largest |w| of the matrix to [2^13, 2^14).
//
//   nnet2_prep     fp32 rows -> (hi, lo) planes: the features.  One wave per row.
//   nnet2_row      fp32 pre-activations -> {none | p-norm | ReLU} -> {normalize} -> (hi, lo) planes.  One wave per row
//                  (kNnet2RowThreads / 64 rows per workgroup); the normalizer's sum of squares is the lanes' partial sums (lane l
//                  takes outputs l, l + 64, ... in that order) folded by a butterfly: one order, a function of the row alone.
//                  The row is read twice (the second time from the cache); no LDS.
//   nnet2_affine   out[t][n] = bias[n] + sum over the splice offsets c (in context order) and k of x[t + c][k] w[n][c][k], on
//                  the matrix cores: per 32 columns of K three v_mfma_f32_16x16x32_f16, hi.hi into one fp32 accumulator, hi.lo and
//                  lo.hi into a second one that enters with 2^-11 in the epilogue.  A workgroup is 4 waves and makes
//                  kNnet2TileM x kNnet2TileN outputs, a wave 32 x 64; the fragments come straight from global memory (16 bytes per
//                  lane and fragment, rows of the planes and of the weights being K-contiguous) - no LDS, no barrier.  Reads of
//                  rows outside [row_lo, row_hi) are clamped to that range, so no read leaves the planes whatever the caller
//                  passes; the layout gives every buffer halo rows so that the clamp never acts on a row that is consumed.
//                  Halo rows and context-only rows hold whatever was there (stale values of other layers, possibly Inf or NaN): a
//                  consumed row never reads them, because its dependency cone lies inside its own utterance's rows.
//                  One output element is one chain of MFMAs over (c, k) in one wave: no split-K, no atomics, and the same bits
//                  whichever tile the row falls in.
//   nnet2_head     per row of n <= kNnet2HeadMaxCols logits: maximum, sum of expf(x - max), p = max(e / sum, 1e-20), group sums
//                  (group g = columns [start[g], start[g + 1]), summed in column order by one thread), times inv_prior[g], and
//                  logf(max(p, 1e-20)).  One workgroup per row; the row stays in LDS between the passes (kNnet2HeadLdsBytes).
//                  src_row[r] names the row of the logits that output row r is made from.
// No kernel uses an atomic or a scalar-memory write.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace xv {

constexpr int kNnet2TileM = 64, kNnet2TileN = 128, kNnet2TileK = 32;
constexpr int kNnet2AffineThreads = 256;
constexpr int kNnet2RowThreads = 256;
constexpr int kNnet2HeadThreads = 256;
constexpr int kNnet2HeadMaxCols = 16384;
constexpr int kNnet2MaxContext = 32;      // time offsets of one splice
constexpr float kNnet2LoScale = 2048.f;   // 2^11
constexpr int kNnet2PrepLdsBytes = 0, kNnet2RowLdsBytes = 0, kNnet2AffineLdsBytes = 0;
constexpr int kNnet2HeadLdsBytes = kNnet2HeadMaxCols * 4 + kNnet2HeadThreads / 64 * 4;

struct Nnet2PrepArgs {
  const float* x;       // [rows][cols]
  int64_t rows;
  int cols;
  uint16_t *hi, *lo;    // [rows][ld]
  int ld;
};

struct Nnet2RowArgs {
  const float* pre;     // [rows][ldp]
  int64_t rows;
  int ldp;
  int in_dim, out_dim;  // p-norm: in_dim = group * out_dim; otherwise equal
  int nonlin;           // 0 none, 1 p-norm, 2 ReLU
  int normalize;
  uint16_t *hi, *lo;    // [rows][ld]
  int ld;
};

struct Nnet2AffineArgs {
  const uint16_t *x_hi, *x_lo;   // row 0 of the launch; rows [row_lo, row_hi) exist
  int ldx;                       // = k_pad
  int rows;                      // output rows
  int row_lo, row_hi;
  int n_ctx;
  int ctx[kNnet2MaxContext];
  int k_pad;                     // per offset, a multiple of kNnet2TileK
  const uint16_t *w_hi, *w_lo;   // [n_pad][n_ctx * k_pad]
  int n_pad, n;                  // n_pad a multiple of kNnet2TileN
  const float* bias;             // [n]
  float w_unscale;               // 1 / the power of two the weights were scaled by
  float* out;                    // [rows][ldo]
  int ldo;
};

struct Nnet2HeadArgs {
  const float* logits;      // [..][ldl]
  int ldl, n;
  const int32_t* src_row;   // [rows] or null: row r
  int rows;
  const int32_t* start;     // [n_out + 1] or null: no groups (n_out == n)
  int n_out;
  const float* inv_prior;   // [n_out] or null
  int apply_log;
  float* out;               // [rows][n_out]
};

hipError_t launch_nnet2_prep(const Nnet2PrepArgs& a, hipStream_t s);
hipError_t launch_nnet2_row(const Nnet2RowArgs& a, hipStream_t s);
hipError_t launch_nnet2_affine(const Nnet2AffineArgs& a, hipStream_t s);
hipError_t launch_nnet2_head(const Nnet2HeadArgs& a, hipStream_t s);

}  // namespace xv
