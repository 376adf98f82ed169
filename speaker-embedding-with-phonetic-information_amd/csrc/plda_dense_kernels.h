// Device kernels of adaptive score normalisation (AS-norm): PLDA log-likelihood ratios of ALL pairs of two
// tables as one fp64 matrix product on v_mfma_f64_16x16x4_f64, and the exact top-N statistics of every row of such a matrix.
// Kept beside plda_kernels.h for the reason given there.  fp64 throughout, deterministic: no float atomics, no split of a sum
// that depends on the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "plda_kernels.h"

namespace xv {

// ---- dense scoring.  Plda::LogLikelihoodRatio(u_i with num_i examples, v_j) in its expanded form
//   S[i][j] = r_i + sum_d A1[i][d] v_jd + sum_d A2[i][d] v_jd^2
//   A1 = m / var,  A2 = 1/2 (1/(1 + psi) - 1/var),  r_i = 1/2 sum (log(1 + psi) - log var) - 1/2 sum m^2 / var
// with m and var of plda_enroll_kernel.  The enrolment operand is [A1 | A2] and r, the test operand [v | v^2]; both are rows
// of dense_k_stride(dim) doubles, zero beyond 2 dim.  S[i][j] is one chain over k = 0 .. stride in steps of 4 (the MFMA's),
// then one addition of r_i: a function of (u_i, num_i, v_j, psi) only, wherever the pair sits in whichever launch, and
// whichever of the two operands takes the rows of the output.
constexpr int kDenseTileM = 64;   // output rows per workgroup (4 waves as 2 x 2, a wave holds 2 x 2 fragments of 16 x 16)
constexpr int kDenseTileN = 64;   // output columns per workgroup
constexpr int kDenseKC = 32;      // k per LDS stage; the operands' row stride is a multiple of it
constexpr int kDensePad = 2;      // doubles added to an LDS row: lane (r, q) of a fragment read hits bank pair (2 r + q) mod 32

inline int dense_k_stride(int dim) { return (2 * dim + kDenseKC - 1) / kDenseKC * kDenseKC; }

struct DensePrepArgs {
  const float* u;           // [n_u][dim] transformed enrolment vectors
  const double* num_u;      // [n_u]
  int n_u;
  const float* v;           // [n_v][dim] transformed test vectors
  int n_v, dim;
  const double* psi;        // [dim]
  const double* inv_psi1;   // [dim] 1 / (1 + psi_d)
  double* a;                // [n_u][dense_k_stride(dim)]  [A1 | A2 | 0]
  double* r;                // [n_u]
  double* b;                // [n_v][dense_k_stride(dim)]  [v | v^2 | 0]
};
hipError_t launch_plda_dense_prep(const DensePrepArgs& a, hipStream_t s);

// out[i][j] = sum_k p[row0 + i][k] q[j][k] + (row_add ? row_add[row0 + i] : col_add[j]),  i < m, j < n; exactly one of the
// two addends is given (the enrolment operand's r: row_add when it is p, col_add when it is q).
struct DenseGemmArgs {
  const double* p;          // [*][k_stride]
  const double* q;          // [n][k_stride]
  const double* row_add;    // [*] or null
  const double* col_add;    // [n] or null
  int64_t row0;
  int m, n, k_stride;
  double* out;              // [m][n]
};
hipError_t launch_plda_dense_gemm(const DenseGemmArgs& a, hipStream_t s);

// ---- top-N statistics.  Per row of x [rows][cols]: the n largest values (exact: radix select on order-preserving 64-bit keys,
// eight passes of eight bits; among values equal to the n-th largest, the lowest columns), their mean and their population
// standard deviation sqrt(sum (x - mean)^2 / n), the second sum taken after the first.  -0 counts as +0.  One workgroup per
// row; each sum runs over ALL columns (a column that is not selected adds +0) lane by lane in column order, then down a fixed
// tree: the order is a function of cols only.  Where the n values are one value, that is the mean and the deviation is 0
// (no sum is taken: n x / n need not be x).  Input must be finite.  2 <= n <= cols <= kTopnMaxCols.
constexpr int kTopnMaxCols = 1 << 20;   // a workgroup walks its row eleven times: this bounds that walk (8 MiB a row)
constexpr int kTopnThreads = 256;
struct TopnArgs {
  const double* x;          // [rows][cols]
  int64_t rows;
  int cols, n;
  double* mean;             // [rows]
  double* std;              // [rows]
};
hipError_t launch_topn_stats(const TopnArgs& a, hipStream_t s);

}  // namespace xv
