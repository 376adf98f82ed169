// Diagonal UBM training: what gmm-global-init-from-feats, gmm-global-acc-stats, gmm-global-sum-accs and gmm-global-est do in
// sid/train_diag_ubm.sh:105-137.  A restatement of Kaldi's gmm/mle-diag-gmm.cc, gmm/diag-gmm.cc and gmmbin/gmm-global-*.cc of early
// 2018, written from their documented behaviour: as in ubm_train.h, parity with a Kaldi binary is not pinned by any test here.  The
// .acc files are intermediates that only these tools read; interchange with Kaldi's is not claimed.  tests/dubm_train_ref.py is the
// same in numpy.
//
// The generator.  mix(s, c) is ivex_train.h's (Mix53).  Entry e of seed s gives the integers a(e) = mix(s, 2 e), b(e) = mix(s, 2 e + 1)
// and the Box-Muller value gauss(e) = sqrt(-2 log((a(e) + 1) / 2^53)) cos(2 pi b(e) / 2^53).  The three users draw from disjoint
// entries: frame sampling e = 2^60 + r; the initial frames e = 2 * 2^60 + attempt; Split e = 3 * 2^60 + stream * 2^36 + i * D + d for
// dimension d of the Gaussian that the split creates at index i (stream: 0 in gmm-global-est, iteration + 1 in
// gmm-global-init-from-feats).  --seed is an option of ours; the same seed gives the same bytes.
//
// gmm-global-acc-stats [--binary=true] [--update-flags=mvw] --gselect=<rspecifier> <model-in> <feature-rspecifier> <stats-out>  (device)
//   Reading, the per-utterance errors (no gselect entry, wrong length, wrong width, no rows) and the closing log lines are
//   fgmm-global-acc-stats' (ubm_train.h): the two tools run one driver, GmmAccStats of gmm_acc_tool.h.
//   Per frame x (fp32) with selected Gaussians s_1 .. s_n: the scores are the diagonal model's on the selection, bit for bit what
//   gmm-gselect ranked; the posteriors are ubm_post's fp32 softmax with min_post = 0, kept in the
//   selection's slots; the frame's log-sum is added to the total log-likelihood.  Per pair (g, p) with p != 0, in fp64:
//   occ_g += p; with m: mean_g += p x; with v: var_g += p (x x) (the flags augmented: v implies m, m implies w).
//   The accepted frames are concatenated and cut into blocks of exactly kDgmmAccFrameBlock frames, one device call each, the last
//   possibly short: no option, utterance boundary or reader buffering changes a bit of the output.
//   Refused by name: running without --gselect, and --weights.  A Gaussian index outside [0, G) is fatal before anything is
//   uploaded; a dimension above 96 or more than 64 selected Gaussians is an error that names the limit.
// Accumulator file
//   <GMMACCS> <VECSIZE> dim <NUMCOMPONENTS> G <FLAGS> uint16 <OCCUPANCY> float vector <MEANACCS> float matrix [G][D], then, only with
//   v, <DIAGVARACCS> float matrix [G][D], and </GMMACCS>.  The fp64 accumulators are rounded to float once, at the write.
// gmm-global-sum-accs [--binary=true] <stats-out> <stats-in1> ...  (host)
//   Adds in argument order, in fp64; dimensions, counts and flags must agree.  Log: "Summed N stats", "Written stats to <out>".
// gmm-global-est [--binary] [--update-flags=mvw] [--min-gaussian-weight=1e-5] [--min-gaussian-occupancy=10] [--min-variance=0.001]
//                [--remove-low-count-gaussians=true] [--mix-up=0] [--perturb-factor=0.01] [--seed=0] <model-in> <stats-in> <model-out>
//   (host, fp64: MleDiagGmmUpdate.)  The model's floats are widened: mu_old = (mu / var) / (1 / var), var_old = 1 / (1 / var).
//   0. Update flags that the accumulators lack are an error.
//   1. The objective before: sum_g occ_g gconst_g + sum mean_acc . (mu / var) - 1/2 sum var_acc . (1 / var); the mean term only with
//      m and the last term only with v among the accumulator's flags.
//   2. For every g: prob = occ_g / sum occ, or 1 / G if the sum is 0.
//      occ_g > min_occ and prob > min_weight: the weight is prob; with m in the accumulators mu = mean_acc_g / occ_g; with v
//        var = var_acc_g / occ_g - mu^2, plus (mu - mu_old)^2 when m is not updated; every element below --min-variance is raised to
//        it, the raised elements and the Gaussians they belong to are counted.  Only what the update flags name is copied back:
//        1 / var is stored as float(1 / var_use) when v is updated (else it keeps its bits) and mu / var as float(mu_use / var_use)
//        when m or v is, var_use and mu_use being the new or the old values.
//      Otherwise, with --remove-low-count-gaussians and fewer than G - 1 Gaussians marked so far: warn "Too little data - removing
//        Gaussian (weight W, occupation count C, vector size D)" and mark it; it keeps its old weight until it is taken out.
//      Otherwise: warn that the Gaussian is kept and set its weight to max(prob, min_weight).
//   3. With w updated the weights are renormalised; the gconsts are recomputed; the objective after, on all G Gaussians; the marked
//      Gaussians are removed, the weights renormalised again and the gconsts recomputed.
//   4. Log "Overall objective function improvement is I per frame over F frames", the floor counts if any, "Written model to <out>".
//   --mix-up=N above the size after the update runs Split(N, perturb_factor) (stream 0) before the model is written.
// Split(target, perturb)  (DiagGmm::Split)
//   Until the model has `target` Gaussians: take the Gaussian of the largest weight (the lowest index on ties), halve its weight, append
//   a copy at index i, and move the two mu / var rows by +(copy) and -(original) perturb * r, r_d = gauss(e(i, d)) sqrt((1 / var)_d),
//   in fp64 rounded to float.  The gconsts are recomputed at the end.
// gmm-global-init-from-feats [--binary=true] [--num-gauss=100] [--num-gauss-init=0] [--num-iters=50] [--num-frames=200000]
//                            [--num-threads=4 (ignored)] [the four M-step options] [--seed=0] <feature-rspecifier> <model-out>  (device)
//   Sampling: read row number r (from 1) is kept while r <= num_frames; after that it is kept iff a(e) / 2^53 < num_frames / r and then
//   overwrites slot b(e) mod num_frames.  Widths that differ are fatal.  Log "Kept N out of R input frames = P%." or the warning
//   "Number of frames read R was less than target number N, using all we read."
//   Initialisation (InitGmmFromRandomFrames): num_gauss_init <= 0 or above num_gauss means num_gauss; fewer than 10 num_gauss_init
//   frames: "Too few frames to train on"; the global mean and variance in fp64 (sum x / T, sum x^2 / T - mean^2, frames ascending); a
//   variance that is not positive is an error; Gaussian g's mean is frame a(e) mod T of the first attempt (counted over all Gaussians,
//   from 0) that names a frame not yet used; variances the global one, weights 1 / G.
//   EM: gauss_inc = (num_gauss - num_gauss_init) / (num_iters / 2) in integers (num_iters < 2: the whole difference, where upstream
//   divides by zero).  Per iteration: the dense E-step over all kept frames with all flags and weight 1 (scores against ALL Gaussians;
//   per frame the exact maximum, sum_g expf(s_g - max) in fp64, logsum = float(max + log(sum)), p = expf(s - logsum)); log "Likelihood
//   per frame on iteration I was L over T frames."; the M-step above; log "Objective-function change on iteration I was C over T
//   frames."; then Split(min(num_gauss, cur + gauss_inc), 0.1) with stream I + 1 if that is above the model's size.  At the end
//   "Wrote model to <out>".  The kept frames are uploaded once; per iteration the model goes up and the statistics come down.
//
// On the device: dubm_train_kernels.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "gmm_train.h"
#include "kio.h"
#include "ubm.h"

namespace xv {

// ---- the generator
uint64_t DgmmDrawA(uint64_t seed, uint64_t e);
uint64_t DgmmDrawB(uint64_t seed, uint64_t e);
double DgmmGauss(uint64_t seed, uint64_t e);
constexpr uint64_t kDgmmEntrySample = (uint64_t)1 << 60, kDgmmEntryInit = (uint64_t)2 << 60, kDgmmEntrySplit = (uint64_t)3 << 60;

// The accumulators on the host (DgmmAccs: `second` holds var [G][D]) and their file: gmm_train.h.

// ---- the M-step (host, fp64)
struct DgmmEstOptions {
  double min_gaussian_weight = 1e-5, min_gaussian_occupancy = 10.0, min_variance = 0.001;
  bool remove_low_count_gaussians = true;
};
using DgmmEstResult = GmmEstResult;
void DgmmEst(const DgmmAccs& accs, int update_flags, const DgmmEstOptions& opts, DiagGmmData* model, DgmmEstResult* res);
// No-op when target <= the model's size.  split_of (may be null): for every Gaussian added, the index it was copied from.
void DgmmSplit(DiagGmmData* model, int target, double perturb_factor, uint64_t seed, uint64_t stream, std::vector<int32_t>* split_of = nullptr);

// ---- gmm-global-init-from-feats on the host
// The reservoir of the sampling rule: Add every row in reading order.
struct DgmmFrameSampler {
  int num_frames = 0, dim = 0;
  uint64_t seed = 0;
  int64_t num_read = 0;
  std::vector<float> kept;   // [min(num_read, num_frames)][dim]
  void Add(const float* row);
  int64_t rows() const { return dim ? (int64_t)(kept.size() / dim) : 0; }
};
void DgmmInitFromFrames(const float* feats, int64_t rows, int dim, int num_gauss, uint64_t seed, DiagGmmData* out);

// ---- the accumulators on one device
class DgmmAccumulator {
 public:
  ~DgmmAccumulator();
  int num_gauss() const;
  int dim() const;
  int flags() const;   // augmented
  struct Impl;
  std::unique_ptr<Impl> impl_;
};
DgmmAccumulator* DgmmAccCreate(int device, int num_gauss, int dim, int flags);
// Back to zero, with a new number of Gaussians; the frames of DgmmAccSetFrames stay.
void DgmmAccReset(DgmmAccumulator* acc, int num_gauss);
// The caller's sparse pairs through the accumulator kernels alone (the arguments of FgmmAccAdd).  device_ms2: {sort, dgmm_acc}.
void DgmmAccAdd(DgmmAccumulator* acc, const float* feats, int64_t rows, const int32_t* post_off, const int32_t* post_idx, const float* post_w,
                float* device_ms2 = nullptr);
// The fused sparse E-step for one block of frames.  gselect [rows][n]; loglikes [rows][n] may be null; logsum [rows].  device_ms4 (may
// be null): {sort, scores, softmax, dgmm_acc}.
void DgmmAccAddGselect(DgmmAccumulator* acc, const UbmModel& diag, const float* feats, int64_t rows, const int32_t* gselect, int n, float* loglikes,
                       float* logsum, float* device_ms4 = nullptr);
// A caller's dense posteriors [rows][G] through dgmm_dense_acc and the reduction alone.
void DgmmAccAddDensePost(DgmmAccumulator* acc, const float* feats, int64_t rows, const float* post);
// The fused dense E-step.  feats == null: the frames of DgmmAccSetFrames.  logsum [rows] may be null.  device_ms3 (may be null):
// {dgmm_dense_logsum, dgmm_dense_acc, reduction}.
void DgmmAccSetFrames(DgmmAccumulator* acc, const float* feats, int64_t rows);
void DgmmAccAddDense(DgmmAccumulator* acc, const UbmModel& diag, const float* feats, int64_t rows, float* logsum, float* device_ms3 = nullptr);
// any of the three may be null
void DgmmAccGet(const DgmmAccumulator& acc, double* occ, double* mean, double* var);

}  // namespace xv
