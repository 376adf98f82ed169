// Per-speaker cepstral mean and variance normalisation: what compute-cmvn-stats and apply-cmvn do in front of the acoustic-model
// path of the recipes (steps/compute_cmvn_stats.sh:104; sid/nnet3_cvector/am/extract_bn.sh:59).  A restatement of Kaldi's
// transform/cmvn.cc of early 2018; tests/cmvn_ref.py is the same in numpy.
//
// Statistics of a rows x cols matrix: double stats[2][cols + 1]
//   stats[0][d] = sum of column d, stats[0][cols] = rows;  stats[1][d] = sum of squares of column d, stats[1][cols] = 0
//   Sums are formed on the device in fp64 (cmvn_kernels.h), in an order that depends on the matrix's shape only: the same bits in
//   whatever batch the matrix lands.  Speaker statistics are utterance statistics added on the host, in spk2utt list order.
// Norm of one statistics matrix (CmvnNorm; fp64 throughout, stored as float): float norm[2][cols], row 0 offset, row 1 scale
//   count = stats[0][cols] (count < 1: an error);  mean = stats[0][d] / count
//   mean only:      scale = 1,              offset = -mean
//   with variance:  var = stats[1][d] / count - mean * mean, floored at 1e-20;  scale = 1 / sqrt(var),  offset = -(mean * scale)
//   reverse:        scale = sqrt(var) (1 without variance), offset = mean
//   a skipped dim:  stats[0][d] = 0, stats[1][d] = count first (mean 0, variance 1)
//   neither means nor variances: scale = 1, offset = 0
// Application: out = x * scale + offset in fp32, the product and the sum each rounded on their own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "feat_batch.h"   // CmvnCompressed
#include "kio.h"

namespace xv {

struct CmvnArgError : public std::runtime_error {
  explicit CmvnArgError(const std::string& m) : std::runtime_error(m) {}
};

// Host only.  Returns the number of variances that were floored.  KioError: count < 1; CmvnArgError: variances without means.
int CmvnNorm(const double* stats, int cols, bool norm_means, bool norm_vars, bool reverse, const int* skip_dims, int n_skip,
             float* norm);

// The value of --skip-dims: "a:b:c" -> {a, b, c}; false for anything else (an empty string is the empty list)
bool ParseSkipDims(const std::string& value, std::vector<int>* dims);

// stats: [n][2][cols + 1].  Blocking.  device_ms: the kernels' time.
void CmvnStats(int device, const float* feats, const int32_t* row_off, int n, int cols, double* stats, float* device_ms = nullptr,
               const CmvnCompressed* cm = nullptr);
// norms: [n_norms][2][cols]; utt_norm[u]: the norm of matrix u, or -1 for a matrix that is left out (its rows of out are not
// written).  out: [row_off[n]][cols].  Blocking.
void CmvnApply(int device, const float* feats, const int32_t* row_off, int n, int cols, const float* norms, int n_norms,
               const int32_t* utt_norm, float* out, float* device_ms = nullptr, const CmvnCompressed* cm = nullptr);
// The same behind a row selection, as one launch (cmvn_kernels.h cmvn_apply_select; what nnet3-compute runs in front of the
// network for the per-speaker pipeline, fuse_pipe.h): out[i] = feats[sel_row[i]] * scale + offset with the norm of utterance
// sel_utt[i].  sel_row: absolute rows of feats, each inside its utterance; every utterance that has a selected row has
// utt_norm >= 0 (the others may be -1 and are not touched).  out: [n_out][cols].  Blocking; KioError on a bad table.
void CmvnApplySelect(int device, const float* feats, const int32_t* row_off, int n, int cols, const float* norms, int n_norms,
                     const int32_t* utt_norm, const int32_t* sel_row, const int32_t* sel_utt, int n_out, float* out,
                     float* device_ms = nullptr);

}  // namespace xv
