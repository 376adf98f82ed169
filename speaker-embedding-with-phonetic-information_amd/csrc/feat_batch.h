// Shared by the tools that read a feature table ahead in batches for device calls (ubm_tools_main.cc, gmm_classify_tools_main.cc,
// gmm_acc_tool.h, post_tools_main.cc, ivex_tools_main.cc, ivex_train_tools_main.cc, dubm_train_tools_main.cc, cmvn_tools_main.cc):
// the batch reader, and the one walk over its batches that reports the entries that could not be read.  Host only: kio.h, cli.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "kio.h"

namespace xv {

// The matrices of a device call may come as stored: "CM" objects (compress.h) back to back in `bytes`, object u at off[u]; they
// are uploaded at one byte per element and expanded on the device (kernels.h CmExpandArgs; cols <= 64).  feats is then ignored.
struct CmvnCompressed {
  const uint8_t* bytes;
  const int64_t* off;   // [n]
  size_t nbytes;
  int max_rows;
};

// Reads a feature table ahead in batches of one column count for the device calls.  A table whose objects can be addressed (an
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

constexpr int64_t kBatchFrames = 1 << 16;   // frames read ahead per device call, where a tool has no reason for another number

// What a tool makes of the entries the reader could not deliver.
enum class FeatProblems {
  kCount,            // both kinds warned and counted as errors
  kCountUnreadable,  // both warned; a matrix without rows is skipped, not an error
  kThrowUnreadable,  // a matrix without rows is ignored; one that cannot be read is fatal (KioError)
};

// The walk over a feature table, which the constructor opens: Run hands every batch to `each`, after the problems met on the
// way to it have been reported, and returns the number of entries counted as errors.
class FeatBatchWalk {
 public:
  FeatBatchWalk(const std::string& rspecifier, int64_t max_frames, bool allow_compressed, FeatProblems policy)
      : reader_(rspecifier, max_frames, allow_compressed), policy_(policy) {}
  long Run(const std::function<void(const FeatBatchReader::Batch&)>& each);

 private:
  FeatBatchReader reader_;
  FeatProblems policy_;
};

}  // namespace xv
