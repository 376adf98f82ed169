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

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

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

// The matrices of a device call may come as stored: "CM" objects (compress.h) back to back in `bytes`, object u at off[u]; they
// are uploaded at one byte per element and expanded on the device (kernels.h CmExpandArgs; cols <= 64).  feats is then ignored.
struct CmvnCompressed {
  const uint8_t* bytes;
  const int64_t* off;   // [n]
  size_t nbytes;
  int max_rows;
};

// stats: [n][2][cols + 1].  Blocking.  device_ms: the kernels' time.
void CmvnStats(int device, const float* feats, const int32_t* row_off, int n, int cols, double* stats, float* device_ms = nullptr,
               const CmvnCompressed* cm = nullptr);
// norms: [n_norms][2][cols]; utt_norm[u]: the norm of matrix u, or -1 for a matrix that is left out (its rows of out are not
// written).  out: [row_off[n]][cols].  Blocking.
void CmvnApply(int device, const float* feats, const int32_t* row_off, int n, int cols, const float* norms, int n_norms,
               const int32_t* utt_norm, float* out, float* device_ms = nullptr, const CmvnCompressed* cm = nullptr);

// Reads a feature table ahead in batches of one column count for the calls above.  A table whose objects can be addressed (an
// archive in a regular file, a script file) is read through views of the mapped files, and its "CM" objects are handed on as
// stored; anything else goes through the sequential reader.
class FeatBatchReader {
 public:
  struct Batch {
    std::vector<std::string> keys;
    std::vector<int32_t> row_off;   // [keys.size() + 1]
    int cols = 0;
    bool compressed = false;        // true: cm / cm_off hold the objects, feats is empty
    std::vector<float> feats;
    std::vector<uint8_t> cm;
    std::vector<int64_t> cm_off;
    int max_rows = 0;
    CmvnCompressed View() const { return CmvnCompressed{cm.data(), cm_off.data(), cm.size(), max_rows}; }
  };
  struct Problem {
    std::string key, what;   // what empty: a matrix without rows
  };
  FeatBatchReader(const std::string& rspecifier, int64_t max_frames, bool allow_compressed);
  ~FeatBatchReader();
  // false: the table is exhausted (and *b is empty).  problems: the entries met on the way that could not be read or have no rows.
  bool Next(Batch* b, std::vector<Problem>* problems);

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

}  // namespace xv
