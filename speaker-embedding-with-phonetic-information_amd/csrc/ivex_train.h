// i-vector extractor training: what ivector-extractor-init, ivector-extractor-acc-stats, ivector-extractor-sum-accs and
// ivector-extractor-est do in sid/train_ivector_extractor.sh:97-160.  [UPSTREAM, recalled]: a restatement of Kaldi's
// ivector/ivector-extractor.cc and ivectorbin/ivector-extractor-{init,acc-stats,sum-accs,est}.cc of early 2018, written from their
// documented behaviour; Kaldi is not part of the reference tree, so parity with a Kaldi binary is not pinned by any test here.
// tests/ivector_train_ref.py is the same in numpy.  Models with i-vector-dependent weights are refused, as in ivex.h.
//
// ivector-extractor-init  (host)
//   SigmaInv_g = the UBM's inverse covariances, w_vec = its weights, the prior offset is 100.  M_g has standard normal entries with
//   column 0 replaced by mean_g / 100, mean_g = Sigma_g (Sigma_g^-1 mu_g) from the UBM's natural parameters.  Upstream draws the
//   entries from rand(); here entry e (the index into M [G][D][S]) of seed s is the Box-Muller pair member
//     sqrt(-2 log u1) cos(2 pi u2),  u1 = (mix(s, 2 e) + 1) / 2^53,  u2 = mix(s, 2 e + 1) / 2^53,
//   mix(s, c) = the top 53 bits of splitmix64's output function applied to s * 0x9E3779B97F4A7C15 + c (a counter-based generator:
//   no state, the same seed gives the same bytes).  --seed is an option of ours.
//
// The statistics (E-step, device, fp64).  Per utterance u, with SigmaInvM_g, U_g and the prior offset p of ivex.h:
//   gamma_u, X_u, l, Q, the Cholesky factor L of Q and the fp64 solution m_u of Q m = l are IvexExtract's (acoustic weight 1, no
//   max-count); m_u is with the prior offset and is not rounded.  Var_u = Q^-1 = L^-T L^-1; scatter_u = Var_u + m_u m_u' as a packed
//   lower triangle of P = S (S + 1) / 2 values; logdet Var_u = -2 sum_i log L_ii.
//   An utterance whose Q is not positive definite (the solve's status) contributes to nothing and is counted as an error.
//   Accumulated over the accepted utterances:
//     gamma [G] += gamma_u;  Y_g [D][S] += X_ug m_u';  R_g [P] += gamma_ug scatter_u;
//     S_g [D (D + 1) / 2] += sum_t w_t x_t x_t' (only with update_variances);
//     num_ivectors += 1;  ivector_sum [S] += m_u;  ivector_scatter [P] += scatter_u.
//   The objective (with compute_auxf) is the variational lower bound
//     F_u = sum_g gamma_ug (log w_g + gconst_g) - 1/2 sum_g tr(Sigma_g^-1 S_ug) + l_a . m - 1/2 m' Q_a m - 1/2 tr(Var Q_a)
//           - 1/2 (|m - p e_0|^2 + tr Var) + 1/2 logdet Var + S / 2,
//   l_a = l - p e_0, Q_a = Q - I, gconst_g = -1/2 (D log 2 pi - logdet Sigma_g^-1).  The part from "l_a . m" on is computed per
//   utterance on the device; the first two sums are linear in the statistics and are formed on the host, in fp64, from gamma and
//   S_g when the statistics are fetched.  Without update_variances there is no S_g: -1/2 sum_g gamma_g D stands in for the trace
//   (its value at the maximum-likelihood covariances), as upstream does for statistics without second-order terms.
//   `auxf` is the sum over the accepted utterances (0 without compute_auxf), `frames` the sum of gamma (always written).
//   Determinism: the statistics are a function of the model and the ordered sequence of accepted utterances alone.  The
//   accumulator owns device buffers of kIvexTrainSlots pending utterances (gamma, X, m, scatter); an accepted utterance takes slot
//   count mod kIvexTrainSlots; a full buffer triggers the two rank updates and the small sums (ivex_train_kernels.h); fetching
//   the statistics flushes the rest.  For S_g the frames of the accepted utterances are cut into blocks of kFgmmAccFrameBlock, the
//   pending frames held on the host until a block is full, and go through FgmmAccAdd (ubm_train.h): there is one SYRK.  How the
//   caller splits the utterances over calls, reader buffering and the number of frames change no bit.
//
// The update (M-step, host, fp64; SymmetricEig, Cholesky, InvertSymmetric of plda.h; num_threads threads over the Gaussians)
//   1. Projections.  For each g with gamma_g >= gaussian_min_count (below: warn and skip): R_g = U diag(lambda) U'; lambda floored
//      at max(1e-40, lambda_max / 1e4) (counted); M_g += (Y_g - M_g R_g) U diag(lambda)^-1 U'.
//   2. Variances (only if the statistics hold S_g), with the new M_g: raw_g = S_g - Y_g M_g' - M_g Y_g' + M_g R_g M_g'.  The floor
//      matrix is F = variance_floor_factor * sum raw_g / sum gamma_g over the Gaussians updated, F = L L'.  Sigma_g = raw_g / gamma_g:
//      the eigenvalues of L^-1 Sigma_g L^-T are floored at 1 (counted) and Sigma_g is rebuilt from them (always, as upstream's
//      ApplyFloor does); then inverted.
//   3. Prior.  mu = ivector_sum / n; C = ivector_scatter / n - mu mu' = P diag(s) P', s floored at 1e-7; T = diag(s)^-1/2 P';
//      v = T mu; H = I - 2 a a', a = (v / |v| - e_0) normalised (H = I if v is along e_0), takes v to |v| e_0; V = H T.  With
//      diagonalize, dimensions 1 .. S - 1 are additionally rotated by the eigenvectors (eigenvalues descending) of the lower-right
//      block of sum_g w_g (M_g V^-1)' Sigma_g^-1 (M_g V^-1).  Finally M_g <- M_g V^-1 and the prior offset becomes |v|.
//   4. The objective improvements, each per frame: projections sum_g [tr(M' Sigma^-1 Y) - tr(Sigma^-1 M R M') / 2] new minus old
//      (the old Sigma^-1); variances sum_g [-tr(Sigma^-1 raw_g) / 2 + gamma_g logdet(Sigma^-1) / 2] new minus old; prior
//      n [-(logdet C + S) / 2 + (tr C + |mu - p e_0|^2) / 2].
//
// The .acc file: <IvectorExtractorStats> <NumGauss> G <FeatDim> D <IvectorDim> S <HasVariances> bool <NumIvectors> <Auxf> <Frames>
// doubles, <gamma> <Y> <R> [<S>] <IvectorSum> <IvectorScatter> double vectors, </IvectorExtractorStats>; binary, or text with 17
// significant digits.  It is an intermediate of these tools: interchange with Kaldi's files is not claimed.
// Limits: those of ivex.h (S <= 1024, D <= 96).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "ivex.h"
#include "kio.h"

namespace xv {

struct IvexStats {
  int G = 0, D = 0, S = 0;
  bool has_variances = false;
  double num_ivectors = 0.0, auxf = 0.0, frames = 0.0;
  std::vector<double> gamma;             // [G]
  std::vector<double> Y;                 // [G][D][S]
  std::vector<double> R;                 // [G][P]
  std::vector<double> Sg;                // [G][D (D + 1) / 2] or empty
  std::vector<double> ivector_sum;       // [S]
  std::vector<double> ivector_scatter;   // [P]
  void Init(int G, int D, int S, bool has_variances);
  void Add(const IvexStats& o);          // KioError when the shapes differ
};
void ReadIvexStatsFile(const std::string& rxfilename, IvexStats* s);
void WriteIvexStatsFile(const std::string& wxfilename, bool binary, const IvexStats& s);

// ivector-extractor-init from a full-covariance UBM (host)
constexpr double kIvexInitPriorOffset = 100.0;
void IvexInit(const FullGmmData& ubm, int ivector_dim, uint64_t seed, IvexData* out);
// mix(s, c) of the header comment: 53 bits.  dubm_train.h draws from the same generator.
uint64_t Mix53(uint64_t seed, uint64_t counter);

struct IvexEstOptions {
  double variance_floor_factor = 0.1, gaussian_min_count = 100.0;
  bool diagonalize = true;
  int num_threads = 1;
};
struct IvexEstResult {
  int gauss_updated = 0, gauss_skipped = 0, eig_floored = 0, var_floored = 0, var_floored_gauss = 0, prior_floored = 0;
  double impr_proj = 0.0, impr_var = 0.0, impr_prior = 0.0;   // per frame
  std::vector<double> V;                                      // [S][S]: the transform of the i-vectors the prior update applied
  std::vector<std::string> warnings;
};
// Updates *model in place.  KioError: shapes that do not agree, no i-vectors, a covariance that cannot be inverted.
void IvexEst(const IvexStats& stats, const IvexEstOptions& opts, IvexData* model, IvexEstResult* res);

// ---- the accumulators on the model's device
class IvexAccumulator {
 public:
  ~IvexAccumulator();
  struct Impl;
  std::unique_ptr<Impl> impl_;
};
// The model must outlive the accumulator.
IvexAccumulator* IvexAccCreate(IvexModel* model, bool update_variances, bool compute_auxf);
// The arguments of IvexExtract.  status [n_utts] (may be null): 0, or 1 for an utterance that was not accepted.  device_ms3 (may be
// null): {posterior kernel, R update, Y update} of this call (the flushes it triggered).
void IvexAccAdd(IvexAccumulator* acc, const float* feats, const int32_t* row_off, int n_utts, const int32_t* post_off, const int32_t* post_idx,
                const float* post_w, int32_t* status, float* device_ms3 = nullptr);
// Flushes the pending utterances and frames and downloads everything.
void IvexAccGet(IvexAccumulator* acc, IvexStats* out, float* device_ms3 = nullptr);
// the pending slots as they are (tests): m [count][S], scatter [count][P], logdet [count], auxf [count]; returns count
int IvexAccPending(IvexAccumulator* acc, double* m, double* scatter, double* logdet, double* auxf);

// C[c_rows][ldc] (host) += A' B on rows < M and columns < N through the update kernel alone: A [64][M], B [64][N] (host).
void IvexRankUpdateHost(int device, const double* A, const double* B, double* C, int slots, int64_t M, int64_t N, int64_t c_rows, int64_t ldc);

}  // namespace xv
