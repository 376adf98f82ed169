// The GMM classifiers of the i-vector baseline: what fgmm-gselect --gselect=, fgmm-global-get-frame-likes, compute-vad-from-frame-likes
// and merge-vads do in sid/gender_id.sh:88-118, sid/music_id.sh:73-104 and sid/compute_vad_decision_gmm.sh:91-127.  A restatement of
// Kaldi's gmm/full-gmm.cc (GaussianSelectionPreselect), fgmmbin/fgmm-gselect.cc, fgmmbin/fgmm-global-get-frame-likes.cc,
// ivectorbin/compute-vad-from-frame-likes.cc and ivectorbin/merge-vads.cc of early 2018, written from their documented behaviour:
// parity with a Kaldi binary is not pinned by any test here.  tests/gmm_classify_ref.py is the same in numpy.
//
// Second-stage selection.  A frame comes with a preselection of n_in Gaussians (slots, in the order of the first stage; an index
// may repeat and is then kept as often as it comes).  Every slot is scored by the full model,
//   loglike = gconst_g + (Sigma^-1 mu)_g . x - 1/2 x' Sigma_g^-1 x      (ubm.h; on the device the very kernel of the posteriors)
// and the n_keep = min(n_out, n_in) best slots are returned as (Gaussian, loglike), best first.  The order is total: score
// descending, then Gaussian ascending, then slot ascending; scores are compared as the integer keys of the first-stage selection, so
// -infinity (a gconst that is not finite) ranks below every finite score and NaNs have a place.
// Frame likelihoods.  like_t = log sum over the frame's selection of exp(loglike): the log-sum of the posteriors' softmax (ubm.h)
// with min_post = 0, bit for bit.  Without a selection the model is scored on the identity selection 0 .. G - 1, G <= 64.
// VAD from frame likelihoods.  Frame t goes to the first class j that maximises like_j[t] + log(prior_j) (a later class wins only
// by strict >); priors are 1 when none are given; the label is map[j], or j without a map.
// Merging two VADs.  Without a map 1 iff both are 1, else 0; with a map of triples (a, b, c) the pair (a, b) gives c, and a pair
// that is not in the map is an error that names it.
//
// Limits on the device: n_in <= 64 (kUbmMaxSelect), dimension <= 96 (kUbmMaxDim), dense frame likelihoods only for G <= 64.
#pragma once
#include <stdint.h>

#include "ubm.h"

namespace xv {

// preselect: [rows][n_in], every entry in [0, num_gauss); idx / ll (may be null): [rows][min(n_out, n_in)].  device_ms3 (may be
// null): {sort, scores, rerank}.  Blocking.
void UbmFullGselect(const UbmModel& full, const float* feats, const int32_t* row_off, int n_utts, const int32_t* preselect, int n_in, int n_out,
                    int32_t* idx, float* ll, float* device_ms3 = nullptr);
// gselect: [rows][n], or null for the identity selection (n is then ignored; num_gauss <= 64).  likes: [rows].  device_ms3 (may be
// null): {sort, scores, softmax}.  Blocking.
void UbmFrameLikes(const UbmModel& full, const float* feats, const int32_t* row_off, int n_utts, const int32_t* gselect, int n, float* likes,
                   float* device_ms3 = nullptr);

// Host only.  likes: n_classes arrays of `rows` floats; priors and map: null or [n_classes]; out: [rows].
void VadFromFrameLikes(int n_classes, const float* const* likes, int64_t rows, const float* priors, const int32_t* map, float* out);
// Host only.  map_triples: null (n_triples = 0: the AND of the two) or [n_triples][3]; out: [rows].
void MergeVads(const float* a, const float* b, int64_t rows, const int32_t* map_triples, int n_triples, float* out);

}  // namespace xv
