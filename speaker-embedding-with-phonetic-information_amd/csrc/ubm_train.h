// Full-covariance UBM training: what gmm-global-to-fgmm, subsample-feats, fgmm-global-acc-stats, fgmm-global-sum-accs and
// fgmm-global-est do in sid/train_full_ubm.sh:69-118.  A restatement of Kaldi's gmm/mle-full-gmm.cc, fgmmbin/*.cc and
// featbin/subsample-feats.cc of early 2018, written from their documented behaviour: as in ubm.h, parity with a Kaldi binary is not
// pinned by any test here.  The .acc files are intermediates that only these tools read; interchange with Kaldi's is not claimed.
// tests/ubm_train_ref.py is the same in numpy.
//
// gmm-global-to-fgmm [--binary=true] <diag-in> <full-out>  (host)
//   The weights are copied, means_invcovars = means_invvars, inv_covars_g = diag(inv_vars_g); the gconsts are recomputed by
//   ComputeGconsts(FullGmmData*).  Log: "Written full GMM to <out>".
// subsample-feats [--n=1] [--offset=0] <feats-rspecifier> <feats-wspecifier>  (host row gather)
//   n > 0 keeps the rows offset, offset + n, ...; an utterance that keeps no row gets a warning, counts as an error and is not
//   written.  n < 0 repeats every row |n| times; --offset must then be 0.  n == 0 is a usage error.  Log: "Processed N feature
//   matrices; M with errors." and "Processed X input frames and Y output frames."  Exit status 0 iff a matrix was written.
// fgmm-global-acc-stats [--binary=true] [--update-flags=mvw] --gselect=<rspecifier> <model-in> <feats-rspecifier> <stats-out>  (device)
//   Per utterance: no frames: warn and skip; no gselect entry: warn "No gselect information for utterance <key>", count an error
//   and skip; a gselect entry of the wrong length: warn, count an error and skip.
//   Per frame x (fp32) with selected Gaussians s_1 .. s_n: the log-likelihoods come from the full model on the selection, exactly
//   what UbmPost computes; the posteriors are the softmax, with min_post = 0; the frame's log-sum is added to the utterance's and
//   to the total log-likelihood.
//   Per pair (g, p) with p != 0, in fp64 (p and x are the fp32 values widened):  occ_g += p;  with m or v in the flags
//   mean_g += p x;  with v  cov_g += p x x', lower triangle.
//   The flags are augmented as Kaldi's accumulator does it (AugmentGmmFlags: v implies m, m implies w) before they are used and
//   before they are written: the issue's "m or v" and "v" are then "m" and "v" of the augmented set.
//   Log: every 10 utterances "Avg like per frame so far is ..." at verbose level 1 or above; at the end "Done N files; M with
//   errors." and "Overall likelihood per frame = L over F (weighted) frames."  Exit status 0 iff N > 0.
//   Refused by name, since no script of the recipes does either: running without --gselect, and --weights.
//   A Gaussian index outside [0, G), n > 64 or a dimension above 96 is an error that names the limit.
// Accumulator file
//   <GMMACCS> <VECSIZE> dim <NUMCOMPONENTS> G <FLAGS> flags (a uint16 whose bits are m = 1, v = 2, w = 4; binary: size byte 2 and
//   two bytes) <OCCUPANCY> float vector <MEANACCS> float matrix [G][D], then, only with v, <FULLVARACCS> followed by G packed float
//   lower triangles, and </GMMACCS>.  The fp64 accumulators are rounded to float once, at the write, and are not rescaled.  Binary
//   and text are both written and read.
// fgmm-global-sum-accs [--binary=true] <stats-out> <stats-in1> ...  (host)
//   Reads each input into fp64 accumulators and adds them in argument order; the dimensions, the count and the flags must agree.
//   Log: "Summed N stats" and "Written stats to <out>".
// fgmm-global-est [--binary] [--update-flags=mvw] [--min-gaussian-weight=1e-5] [--min-gaussian-occupancy=100]
//                 [--variance-floor=0.001] [--max-condition=1e5] [--remove-low-count-gaussians=true] <model-in> <stats-in> <model-out>
//   (host, fp64; the algebra is plda.h's SymmetricEig and InvertSymmetric.)  The update flags must be among the accumulator's.
//   1. The objective before the update: sum_g occ_g gconst_g + sum_g mean_acc_g . (Sigma^-1 mu)_g - 1/2 sum_g tr(cov_acc_g Sigma_g^-1),
//      the last term only with v among the accumulator's flags (Kaldi's MlObjective looks at the accumulator, not at the update).
//   2. For every g, prob = occ_g / sum occ, or 1 / G if the sum is 0.
//      occ_g > min_occ and prob > min_weight: the weight is prob; mu_new = mean_acc_g / occ_g (without m the old mean is kept);
//        with v: C = cov_acc_g / occ_g - mu_new mu_new', without m plus (mu_old - mu_new)(mu_old - mu_new)';
//        floor = max(variance_floor, max |eig(C)| / max_condition); every eigenvalue below floor is raised to it and C is rebuilt
//        from its eigenvectors (only if one was raised); the floored eigenvalues and the Gaussians they belong to are counted.
//      Otherwise, with --remove-low-count-gaussians and more than one Gaussian left after the removals so far: warn "Too little
//        data - removing Gaussian (weight ..., occupation count ..., vector size D)" and mark the Gaussian for removal; until step 7 it
//        keeps its old weight, as in Kaldi, so that the objective of step 6 is finite.
//      Otherwise: warn that the Gaussian is kept, set its weight to max(prob, min_weight), leave its other parameters alone.
//   3. Renormalise the weights.  Without w among the update flags the model keeps its old weights instead (Kaldi copies back only
//      what the flags name).
//   4. Back to the natural parameters Sigma^-1 and Sigma^-1 mu, for the Gaussians that were updated: the others keep their bits.
//   5. Recompute the gconsts.
//   6. The objective after the update, on the G Gaussians, before any removal.
//   7. Remove the marked Gaussians, renormalise the weights again and recompute the gconsts.
//   8. Log "Overall objective function improvement is I per frame over F frames", I = (after - before) / F, F = sum occ; the floor
//      counts if there are any; "Written model to <out>".
//   --mix-up other than 0 is refused by name.
//
// On the device (ubm_train_kernels.h) the accumulated statistics are a function of the model and of the SEQUENCE OF FRAMES alone:
// fgmm-global-acc-stats concatenates the frames of the utterances it accepts, cuts that stream into blocks of exactly
// kFgmmAccFrameBlock frames (an utterance may straddle a block: the E-step is per frame) and makes one accumulate call per block,
// the last one possibly short.  No option, no utterance boundary and no reader buffering changes a bit of the output.
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

// The update flags, the accumulators on the host (FgmmAccs: `second` holds the packed lower triangles cov [G][D (D + 1) / 2]) and
// their file: gmm_train.h.

// ---- the M-step (host, fp64)
struct FgmmEstOptions {
  double min_gaussian_weight = 1e-5, min_gaussian_occupancy = 100.0, variance_floor = 0.001, max_condition = 1e5;
  bool remove_low_count_gaussians = true;
};
using FgmmEstResult = GmmEstResult;
// Updates *model in place (num_gauss shrinks by removed.size()).  KioError: shapes that do not agree, update flags the
// accumulators do not have, a covariance that cannot be inverted.
void FgmmEst(const FgmmAccs& accs, int update_flags, const FgmmEstOptions& opts, FullGmmData* model, FgmmEstResult* res);
// gmm-global-to-fgmm
void DiagGmmToFull(const DiagGmmData& diag, FullGmmData* full);

// ---- the accumulators on one device
class FgmmAccumulator {
 public:
  ~FgmmAccumulator();
  int num_gauss() const;
  int dim() const;
  int flags() const;   // augmented
  struct Impl;
  std::unique_ptr<Impl> impl_;
};
// flags are augmented here.  The accumulators start at zero.
FgmmAccumulator* FgmmAccCreate(int device, int num_gauss, int dim, int flags);
// One call, no internal blocking.  feats [rows][dim]; frame t has the pairs post_off[t] .. post_off[t + 1] of post_idx (Gaussian,
// in [0, G): anything else is a KioError before anything is uploaded) and post_w.  device_ms2 (may be null): {sort, fgmm_acc}.
void FgmmAccAdd(FgmmAccumulator* acc, const float* feats, int64_t rows, const int32_t* post_off, const int32_t* post_idx, const float* post_w,
                float* device_ms2 = nullptr);
// The fused E-step of fgmm-global-acc-stats for one block of frames: upload, sort, scores, softmax (min_post = 0) and fgmm_acc,
// without the posteriors leaving the device.  gselect [rows][n]; logsum [rows] is all that comes back.  device_ms4 (may be null):
// {sort, scores, softmax, fgmm_acc}.
void FgmmAccAddGselect(FgmmAccumulator* acc, const UbmModel& full, const float* feats, int64_t rows, const int32_t* gselect, int n, float* logsum,
                       float* device_ms4 = nullptr);
// any of the three may be null
void FgmmAccGet(const FgmmAccumulator& acc, double* occ, double* mean, double* cov);

}  // namespace xv
