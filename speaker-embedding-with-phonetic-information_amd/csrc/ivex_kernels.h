// Device kernels of i-vector extraction (ivector-extract; semantics in ivex.h).  Kept out of kernels.hip for the reason
// ubm_kernels.* are: KERNELS_SHA names the x-vector extraction kernels only.
//
// Everything is fp64 on fp32 inputs.  No floating-point value goes through an atomic and every sum has an order that is a function
// of the utterance and the model alone: an utterance's result is the same bits alone, in any batch, at any position in it.
//   ivex_derive         one workgroup per Gaussian, plain vector fp64 (it runs once per model): SigmaInvM_g = Sigma_g^-1 M_g (j
//                       ascending) into the [G D][S] matrix, then the packed lower triangle of M_g' SigmaInvM_g (i ascending) into
//                       row g of U [G][P].
//   ivex_stats          reads every utterance's (frame, Gaussian, weight) pairs bucketed by Gaussian in frame order (bucket_sort.h,
//                       one segment per utterance).  One wave per (utterance, Gaussian): gamma = sum w and X = sum w x over the
//                       bucket front to back; lane d owns column d.  double(w) * double(x) is exact, so the sums are one fixed set of bits.  Gaussians that were not
//                       hit get zeros.
//   ivex_gemm           C[B][N] = A[B][K] W[K][N] on v_mfma_f64_16x16x4_f64.  A wave owns kIvexColTile columns and every row tile
//                       (kIvexRowTile utterances each, at most kIvexMaxRowTiles): one fetch of a W fragment feeds all of them.  K is
//                       walked in ascending steps of 4 inside [chunk kIvexKChunk blockIdx.y, ...); rows beyond B, columns beyond N and k
//                       beyond the chunk are masked to zero in registers.  With more than one chunk the results are partial sums
//                       [chunk][B][N].  f64 fragment maps (not the f32 ones): A [lane & 15][k = lane >> 4], B [k = lane >> 4][lane & 15],
//                       C/D col = lane & 15, row = (lane >> 4) + 4 reg.
//   ivex_finish_terms   l = the partial sums added in chunk order, l_0 += prior offset; 1 added to the diagonal of the packed Q.
//   ivex_solve          one workgroup per utterance: Q is unpacked into a [S + 1][S] workspace in global memory whose last row is
//                       l, factored by a left-looking blocked Cholesky (block columns of kIvexPanel; the kIvexPanel x kIvexPanel
//                       pieces of the panel rows and the diagonal block live in LDS), which leaves y = L^-1 l in the last row;
//                       then L' x = y backwards.  A pivot that is not positive and finite, or a solution that is not finite, sets
//                       the utterance's status and zeroes its outputs: no NaN leaves the kernel.  The change of the auxiliary
//                       function comes from the unfactored packed Q and l.  S <= kIvexMaxS.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace xv {

constexpr int kIvexThreads = 256;
constexpr int kIvexRowTile = 16;        // utterances per MFMA row tile
constexpr int kIvexMaxRowTiles = 4;     // row tiles a wave carries
constexpr int kIvexMaxBatch = 64;       // kIvexRowTile * kIvexMaxRowTiles utterances per launch group
constexpr int kIvexColTile = 16;        // columns per wave
constexpr int kIvexKChunk = 2048;       // K per workgroup of the linear term (a multiple of 4)
constexpr int kIvexPanel = 32;          // block-column width of the solve
constexpr int kIvexMaxS = 1024;         // the largest i-vector dimension
constexpr int kIvexMaxDim = 96;         // the largest feature dimension

struct IvexDeriveArgs {
  const double* M;           // [G][D][S]
  const double* sigma_inv;   // [G][D (D + 1) / 2] packed lower triangles
  int G, D, S;
  double* sigma_inv_m;       // [G D][S]
  double* U;                 // [G][S (S + 1) / 2]
};

struct IvexStatsArgs {
  const float* feats;          // [rows][D]
  int D, G, B;
  // the pairs of the batch, utterance after utterance, frames ascending inside one
  const int32_t* pair_frame;   // [pairs] row of feats
  const int32_t* pair_gauss;   // [pairs] in [0, G) (the host checks)
  const float* pair_w;         // [pairs] the scaled posterior
  // the pairs sorted by Gaussian inside every utterance (bucket_sort.h, one segment per utterance)
  const int32_t* bucket_start; // [B][G + 1] in pairs of the batch
  const int32_t* sorted;       // [pairs] pair indices, bucket after bucket
  double* gamma;               // [B][G]
  double* X;                   // [B][G D]
};

struct IvexGemmArgs {
  const double* A;   // [B][K]
  const double* W;   // [K][N]
  int B;
  int64_t K, N;
  int k_chunk;       // K per blockIdx.y; the grid has ceil(K / k_chunk) of them
  double* C;         // [ceil(K / k_chunk)][B][N]
};

struct IvexFinishArgs {
  const double* partial;   // [chunks][B][S]
  int chunks, B, S;
  double prior_offset;
  double* linear;          // [B][S]
  double* quadratic;       // [B][S (S + 1) / 2]: the diagonal gains 1
};

struct IvexSolveArgs {
  const double* quadratic;   // [B][S (S + 1) / 2] packed Q
  const double* linear;      // [B][S]
  int B, S;
  double prior_offset;
  double* work;              // [B][S + 1][S]
  float* ivector;            // [B][S]: x with the prior offset taken off element 0 before rounding
  double* auxf_change;       // [B] or null
  int32_t* status;           // [B]: 0, or 1 for a Q that is not positive definite
  double* solution;          // [B][S] or null: x in fp64, with the prior offset (the E-step of training reads it; ivex_train_kernels.h)
};

hipError_t launch_ivex_derive(const IvexDeriveArgs& a, hipStream_t s);
hipError_t launch_ivex_stats(const IvexStatsArgs& a, hipStream_t s);
hipError_t launch_ivex_gemm(const IvexGemmArgs& a, hipStream_t s);
hipError_t launch_ivex_finish_terms(const IvexFinishArgs& a, hipStream_t s);
hipError_t launch_ivex_solve(const IvexSolveArgs& a, hipStream_t s);

}  // namespace xv
