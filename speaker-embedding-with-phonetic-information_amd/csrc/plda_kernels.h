// Device kernels of the PLDA back-end (stage 7 of egs/sre/v2/run_sre10.sh: ivector-compute-lda, ivector-compute-plda,
// ivector-plda-scoring).  Kept out of kernels.hip/kernels.h on purpose: KERNELS_SHA (sha1 of those two files) names the
// extraction kernels in profiles and in the bench line, and these kernels must not move it.
// Everything here is fp64 arithmetic on fp32 inputs, deterministic (fixed reduction order, no float atomics).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace xv {

// Scatter statistics of rows grouped into segments (speakers), the SegMeanArgs convention: segment s holds rows
// idx[seg_off[s] .. seg_off[s+1]) of x.
//   sums[s]  = sum of the rows of segment s                      (fp64, list order)
//   s_tot    = sum over every listed row of x_i x_i^T           (fp64, dim x dim, symmetric)
//   s_bet    = sum over segments of sums[s] sums[s]^T / n_s     (fp64, dim x dim, symmetric; empty segments add nothing)
// The rank-k products run in 64 x 64 output tiles (upper triangle only, mirrored) over fixed row chunks whose count
// depends on (rows, dim) only; the chunk partials are added in chunk order: the same input gives the same bits.
struct ScatterArgs {
  const float* x;           // [*][ldx]
  int dim, ldx;
  const int32_t* seg_off;   // [n_seg + 1] (device)
  const int32_t* idx;       // [n_idx] (device)
  int n_seg, n_idx;         // n_idx == seg_off[n_seg] (host copy)
  double* sums;             // [n_seg][dim]
  double* s_tot;            // [dim][dim]
  double* s_bet;            // [dim][dim]
  double* work;             // scatter_stats_workspace(dim, n_idx, n_seg) doubles
};
size_t scatter_stats_workspace(int dim, int n_idx, int n_seg);
hipError_t launch_scatter_stats(const ScatterArgs& a, hipStream_t s);

// Kaldi's Plda::TransformIvector for a batch: y = offset + T x (fp64), then
//   normalize && !simple: y *= sqrt(dim / sum_d y_d^2 / (psi_d + 1/num_i))
//   normalize &&  simple: y *= sqrt(dim) / |y|
// y is stored rounded to fp32; scale[i] is the factor (returned whether or not it is applied).  dim <= kPldaMaxDim.
constexpr int kPldaMaxDim = 512;
struct PldaTransformArgs {
  const float* x;           // [n][dim]
  int n, dim;
  const double* tt;         // [dim][dim] TRANSPOSED transform: tt[k * dim + d] = T[d][k]
  const double* offset;     // [dim] = -T mean
  const double* psi;        // [dim]
  const double* num;        // [n] example counts
  int normalize, simple;
  float* y;                 // [n][dim]
  double* scale;            // [n]
};
hipError_t launch_plda_transform(const PldaTransformArgs& a, hipStream_t s);

// Kaldi's Plda::LogLikelihoodRatio for a list of trials (enrolment row k, test row t), fp64:
//   m_d = n psi_d/(n psi_d + 1) u_d,  var_d = 1 + psi_d/(n psi_d + 1)
//   llr = -1/2 [sum log var_d + sum (v_d - m_d)^2 / var_d] + 1/2 [sum log(1 + psi_d) + sum v_d^2 / (1 + psi_d)]
// Two kernels: per enrolment row the class-conditional mean, inverse variance and constant (work: n_u * (2 dim + 1)
// doubles), then one wave per trial.  Indices are checked by the caller.  dim <= kPldaMaxDim.
struct PldaScoreArgs {
  const float* u;           // [n_u][dim] transformed enrolment vectors
  const double* num_u;      // [n_u]
  int n_u;
  const float* v;           // [n_v][dim] transformed test vectors
  int n_v, dim;
  const double* psi;        // [dim]
  const double* inv_psi1;   // [dim] 1 / (1 + psi_d)
  const int32_t* trials;    // [n_trials][2] (k, t)
  long n_trials;
  double* work;             // n_u * (2 * dim + 1) doubles
  double* scores;           // [n_trials]
};
hipError_t launch_plda_score(const PldaScoreArgs& a, hipStream_t s);

}  // namespace xv
