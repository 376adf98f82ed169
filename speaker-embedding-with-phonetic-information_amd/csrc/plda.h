// PLDA back-end (stage 7 of egs/sre/v2/run_sre10.sh:221-252, v5/run_sre10.sh:105-137, stage 2 of v2/run_sre16.sh:76-175):
// LDA and two-covariance PLDA estimation, unsupervised PLDA adaptation, the PLDA model object, trial scoring.  Semantics are upstream Kaldi's
// (ivector/plda.cc, ivector/ivector-extractor.cc's LDA helpers, ivectorbin/*.cc) [UPSTREAM, recalled]: not vendored in
// the reference, restated here and in tests/plda_ref.py.
// The statistics over the data and the per-trial work run on the device (plda_kernels.h); the host does the small dense
// fp64 algebra on dim x dim matrices (Cholesky, inverses, a symmetric eigensolver, the EM updates).  The device entry
// points throw EngineError when there is no usable GPU: there is no CPU path.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace xv {

// ---- device entry points (host buffers in and out).  device_ms (optional): kernel time between two events.
// S_tot, sums, S_bet of plda_kernels.h ScatterArgs; s_tot / s_bet [dim][dim], sums [n_seg][dim] (any may be null).
void ScatterStats(int device, const float* x, int n, int dim, const int32_t* seg_off, const int32_t* idx, int n_seg,
                  double* s_tot, double* sums, double* s_bet, float* device_ms = nullptr);
// Plda::TransformIvector on n rows: transform [dim][dim] row-major, offset / psi [dim], num [n].
void PldaTransform(int device, const float* x, int n, int dim, const double* transform, const double* offset,
                   const double* psi, const double* num, bool normalize, bool simple, float* y, double* scale,
                   float* device_ms = nullptr);
// Plda::LogLikelihoodRatio per trial (k, t) = trials[2i], trials[2i+1]; u [n_u][dim] with counts num_u, v [n_v][dim].
void PldaScore(int device, const float* u, const double* num_u, int n_u, const float* v, int n_v, int dim,
               const double* psi, const int32_t* trials, long n_trials, double* scores, float* device_ms = nullptr);

// ---- adaptive score normalisation (plda_dense.cc, plda_dense_kernels.h)
// Plda::LogLikelihoodRatio of every pair (row i of u with num_u[i] examples, row j of v): scores [n_u][n_v].
void PldaScoreDense(int device, const float* u, const double* num_u, int n_u, const float* v, int n_v, int dim, const double* psi,
                    double* scores, float* device_ms = nullptr);
// Mean and population standard deviation of the n largest values of every row of scores [rows][cols] (finite values).
void TopnStats(int device, const double* scores, int64_t rows, int cols, int n, double* mean, double* std, float* device_ms = nullptr);
// TopnStats of PldaScoreDense without the matrix leaving the device: per row of u over all of v, or (by_column) per row of v
// over all of u.  The matrix exists one row chunk at a time in a workspace of at most DenseWorkspaceCap() bytes.
void PldaCohortStats(int device, const float* u, const double* num_u, int n_u, const float* v, int n_v, int dim, const double* psi,
                     bool by_column, int n, double* mean, double* std, float* device_ms = nullptr);
// The chunks of a rows x cols score matrix (host only, pure): rows_per_chunk is the largest count of rows whose scores fit
// the workspace, a multiple of the scoring kernel's row tile where it holds a tile at all, and at most what one launch's grid
// covers; chunk c is rows [c rows_per_chunk, min(rows, (c + 1) rows_per_chunk)).  false with *why: a bad argument, or a
// workspace that does not hold one row.
struct DensePlan {
  int64_t rows_per_chunk = 0, n_chunks = 0;
  int64_t chunk_bytes = 0;   // what the driver allocates: min(rows, rows_per_chunk) rows
};
bool PlanPldaDense(int64_t rows, int64_t cols, int dim, int64_t workspace_bytes, DensePlan* out, std::string* why);
constexpr int64_t kDenseDefaultWorkspace = (int64_t)256 << 20;
// kDenseDefaultWorkspace, or the bytes that the environment variable XVEC_PLDA_DENSE_WORKSPACE names (tests: small chunks)
int64_t DenseWorkspaceCap();

// ---- the model: <Plda> mean transform psi </Plda>
struct Plda {
  int dim = 0;
  std::vector<double> mean, transform, psi;   // transform [dim][dim] row-major
  std::vector<double> offset;                 // derived: -transform * mean
  void ComputeDerivedVars();
  // ivector-copy-plda --smoothing: c_d = 1 + s psi_d, psi_d /= c_d, row d of transform *= c_d^-1/2
  void SmoothWithinClassCovariance(double s);
};
void ReadPlda(const std::string& rxfilename, Plda* p);
void WritePlda(const std::string& wxfilename, bool binary, const Plda& p);

// ---- dense fp64 helpers (row-major n x n)
bool Cholesky(int n, const double* a, double* l);                    // a = l l^T, l lower; false if not positive definite
void InvertLower(int n, const double* l, double* li);               // li = l^-1 (lower)
bool InvertSymmetric(int n, const double* a, double* ai);           // through Cholesky; false if not positive definite
// Eigenvalues sorted descending (Kaldi's SortSvd), eigenvectors as the COLUMNS of u.  Householder + implicit QL.
void SymmetricEig(int n, const double* a, double* s, double* u);

// ---- estimators from scatter statistics (host only)
// ivector-compute-lda: s_tot / s_bet of the mean-subtracted vectors (n rows); out [lda_dim][dim + 1] = [L | -L mean].
// Returns the number of eigenvalues floored in the normalising transform.
int LdaFromStats(int dim, long n, const double* s_tot, const double* s_bet, const float* mean, double total_covariance_factor,
                 double covariance_floor, int lda_dim, float* out);
// ivector-compute-plda: per speaker sums [n_spk][dim] and counts, s_tot / s_bet over all listed rows.  Returns the number
// of between-class eigenvalues floored at zero.  log (optional) receives one line per EM iteration.
int PldaFromStats(int dim, int n_spk, const double* sums, const int32_t* counts, const double* s_tot, const double* s_bet,
                  int num_em_iters, Plda* out, std::vector<std::string>* log = nullptr);
// ivector-adapt-plda (PldaUnsupervisedAdaptor::UpdatePlda [UPSTREAM, recalled]): adapts `plda` in place to n unlabelled
// vectors with sum m [dim] and scatter v = sum x x^T [dim][dim].  The adaptation covariance (plus mean_diff_scale times the
// outer product of the mean shift) is diagonalised in the space where the model's total covariance is I; its excess over 1
// in each direction is added to the within- and between-class covariances with the two scales.  s (optional, [dim])
// receives those eigenvalues, descending.  log (optional) receives the mean shift, the eigenvalues and the old / new psi.
void AdaptPlda(long n, const double* m, const double* v, double mean_diff_scale, double within_covar_scale,
               double between_covar_scale, Plda* plda, double* s = nullptr, std::vector<std::string>* log = nullptr);

}  // namespace xv
