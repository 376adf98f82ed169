// The GMM-UBM stage of the i-vector baseline: what add-deltas, fgmm-global-to-gmm, gmm-gselect, fgmm-global-gselect-to-post and
// scale-post do in sid/extract_ivectors.sh:58-68 (and at the head of sid/train_full_ubm.sh and sid/train_ivector_extractor.sh).
// A restatement of Kaldi's feat/feature-functions.cc (DeltaFeatures), gmm/diag-gmm.cc, gmm/full-gmm.cc and
// fgmmbin/fgmm-global-gselect-to-post.cc of early 2018, written from their documented behaviour: parity with a Kaldi binary is
// not pinned by any test here.  tests/ubm_ref.py is the same in numpy.
//
// Deltas (order, window W; fp32 throughout, every product and every sum rounded on its own):
//   scales[0] = [1];  scales[i][k + j + W] += float(j) * scales[i - 1][k] for j in [-W, W], then scales[i] *= float(1 / sum_j j^2)
//   block i of output frame t = 0 + sum over j ascending of scales[i][j] * in[clamp(t + j, 0, T - 1)], scales that are exactly
//   0 skipped; the output has (order + 1) * D columns; truncate = n > 0 keeps the first n input columns.
// Diagonal model, per frame x and Gaussian g:
//   loglike = gconst_g + sum_d (mu / sigma^2)_gd x_d - 1/2 sum_d (1 / sigma^2)_gd x_d^2
//   Selection keeps the n largest per frame in descending order (equal scores: the lower index first).  -0 and +0 are equal
//   scores: the order is that of score + 0, here and in the second-stage selection of gmm_classify.h.  -infinity is below every
//   finite score; a frame that holds a NaN scores NaN everywhere and selects n distinct Gaussians, which ones is not stated.
// Full model, on the selected Gaussians only:
//   loglike = gconst_g + (Sigma^-1 mu)_g . x - 1/2 x' Sigma_g^-1 x
//   posteriors = softmax over the selected set (its log-sum is what the log line averages).  min_post != 0: remember the arg-max,
//   zero every posterior < min_post, and if nothing is left give the arg-max 1, else scale by 1 / (what is left).  The entries
//   that are not 0 are emitted as (index, posterior) in selection order.  A selected Gaussian that scores -infinity has posterior 0.
//   A frame whose largest selected log-likelihood is not finite has no posterior.  It has zero entries, every slot posterior is 0,
//   and the log-sum is that largest value as computed (-infinity or NaN).  That is a frame whose selected gconsts are all
//   -infinity, or one that holds a NaN; the accumulators of ubm_train.h and dubm_train.h, which skip weights of 0, leave it out.
// Gconsts are recomputed (fp64, stored as float) after every read of a model, whether the file has <GCONSTS> or not:
//   diagonal:  log w_g - 1/2 (D log 2 pi - sum_d log (1/sigma^2)_gd + sum_d (mu/sigma^2)_gd^2 / (1/sigma^2)_gd)
//   full:      log w_g - 1/2 (D log 2 pi + log det Sigma_g + (Sigma^-1 mu)' Sigma (Sigma^-1 mu))
//   A gconst that is not finite (a covariance that is not positive definite) is stored as -infinity and counted.
// fgmm-global-to-gmm, per component in fp64: Sigma = (Sigma^-1)^-1, variances = its diagonal, mean = Sigma (Sigma^-1 mu).
//
// On the device (ubm_kernels.h) everything is fp32 products with fp32 accumulation in an order that is a function of the frame and
// the model alone.  A model is uploaded once, behind a UbmModel.  Limits: n <= 64 selected Gaussians, dimension <= 96.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "bucket_sort.h"
#include "device.h"
#include "kio.h"

namespace xv {

// Host only.  scales[i]: 2 i window + 1 floats.
void DeltaScales(int order, int window, std::vector<std::vector<float>>* scales);
// feats: [row_off[n]][cols]; out: [row_off[n]][(order + 1) * D], D = truncate > 0 ? truncate : cols.  Blocking.
void AddDeltas(int device, const float* feats, const int32_t* row_off, int n, int cols, int order, int window, int truncate, float* out,
               float* device_ms = nullptr);

// Host only; return the number of gconsts that are not finite.
int ComputeGconsts(DiagGmmData* m);
int ComputeGconsts(FullGmmData* m);
// Host only (fp64).  KioError: an inverse covariance that cannot be inverted.
void FullGmmToDiag(const FullGmmData& full, DiagGmmData* diag);
// Whole-file model objects through rxfilenames / wxfilenames ("file", "-", "cmd |"); the readers recompute the gconsts.
void ReadDiagGmmFile(const std::string& rxfilename, DiagGmmData* m);
void ReadFullGmmFile(const std::string& rxfilename, FullGmmData* m);
void WriteDiagGmmFile(const std::string& wxfilename, bool binary, const DiagGmmData& m);
void WriteFullGmmFile(const std::string& wxfilename, bool binary, const FullGmmData& m);

// A model on one device.  Created once per process and device; the calls below only read it.
class UbmModel {
 public:
  ~UbmModel();
  int device() const;
  int num_gauss() const;
  int dim() const;
  bool full() const;
  struct Impl;
  std::unique_ptr<Impl> impl_;
};
// gconsts [G], means_invvars / inv_vars [G][D]
UbmModel* UbmDiagCreate(int device, int num_gauss, int dim, const float* gconsts, const float* means_invvars, const float* inv_vars);
// gconsts [G], means_invcovars [G][D], inv_covars [G][D (D + 1) / 2] packed lower triangles
UbmModel* UbmFullCreate(int device, int num_gauss, int dim, const float* gconsts, const float* means_invcovars, const float* inv_covars);

// The device arrays of a diagonal model, as the selection kernel reads them (ubm_kernels.h: UbmDiagArgs), for the E-steps of
// dubm_train.h.  KioError for a full-covariance model.
struct UbmDiagView {
  int device, num_gauss, dim, gauss_pad;
  const float *m_t, *v_t, *gconst;
};
UbmDiagView UbmDiagArrays(const UbmModel& diag);

// feats: [row_off[n_utts]][dim] packed; idx: [rows][n]; ll: the same shape or null.  n <= min(64, num_gauss).  Blocking.
void UbmGselect(const UbmModel& diag, const float* feats, const int32_t* row_off, int n_utts, int n, int32_t* idx, float* ll,
                float* device_ms = nullptr);
// Host only: log sum_i exp(v_i) in fp64, what the selection tools' log lines average over the frames' ll; -inf when every v_i is.
inline double LogSumExp(const float* v, int n) {
  double mx = v[0];
  for (int i = 1; i < n; ++i) mx = v[i] > mx ? v[i] : mx;
  if (isinf(mx)) return mx;
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += exp((double)v[i] - mx);
  return mx + log(s);
}
// gselect: [rows][n], every entry in [0, num_gauss).  count: [rows]; idx / post: [rows][n], the first count[t] of frame t are set.
// ll ([rows][n], the log-likelihoods before the softmax) and logsum ([rows]) may be null.  device_ms: {sort, scores, softmax}.
void UbmPost(const UbmModel& full, const float* feats, const int32_t* row_off, int n_utts, const int32_t* gselect, int n, float min_post,
             int32_t* count, int32_t* idx, float* post, float* ll, float* logsum, float* device_ms3 = nullptr);

// What UbmPost does on the device for one part of a call's frames, for the callers that keep the results there (ubm_train.h):
// upload, sort, scores, softmax.  The buffers live as long as the object and only grow.  Run checks nothing: CheckUbmSelection
// comes first.  KioError from the check names `who`.
void CheckUbmSelection(const char* who, const UbmModel& full, const int32_t* gselect, int64_t rows, int n);
struct UbmFullArgs;   // ubm_kernels.h
struct UbmPostDevice {
  DevBuf feats, gselect;                // the inputs of the part: [rows][dim], [rows][n]
  BucketSorter sort;                    // its start: [num_gauss + 1] buckets of its sorted: [rows * n] pair indices
  DevBuf ll, count, idx, post, logsum;  // UbmPost's results
  DevBuf slot_post;                     // with_slot_post: [rows][n] the posterior of selection slot i at i, zeros kept
  // device_ms3 (may be null): {sort, scores, softmax} are added to it
  void Run(const UbmModel& full, const float* host_feats, const int32_t* host_gselect, int64_t rows, int n, float min_post, bool with_slot_post,
           float* device_ms3);
  // The first half of Run for the callers that rank the scores instead (gmm_classify.h): upload, sort, scores.  *a comes back
  // filled up to ll; the posterior outputs are null.  tm is marked before the sort, after it and after the scores.
  void Scores(const UbmModel& full, const float* host_feats, const int32_t* host_gselect, int64_t rows, int n, UbmFullArgs* a, EventTimer* tm);
};

}  // namespace xv
