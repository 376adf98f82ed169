// Internal to ubm_train.cc and dubm_train.cc: the sparse accumulator on one device that FgmmAccumulator and DgmmAccumulator embed.
// The running fp64 sums, a call's pairs, their counting sort (bucket_sort.h) and the work items and partial sums of the
// accumulation kernels (ubm_train_kernels.h, dubm_train_kernels.h).  Defined in gmm_train.cc.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>

#include "bucket_sort.h"
#include "device.h"
#include "ubm_train_kernels.h"

namespace xv {

struct GmmSparseAcc {
  int device = 0, num_gauss = 0, dim = 0, flags = 0;   // flags: augmented
  size_t second_width = 0;                              // D (D + 1) / 2 or D
  const char* who_needs = "";                           // UseDevice's
  DevBuf occ, mean, second;                             // the running accumulators: [G], [G][D], [G][second_width]
  DevBuf feats, idx, w, frame;                          // UploadPairs
  BucketSorter sort;                                    // Sort: its start [G + 1] buckets of its sorted [pairs] pair indices
  DevBuf item_start, partial;                           // Accumulate

  // Selects the device; the accumulators get num_gauss rows and start at zero.
  void Reset(int num_gauss);
  // The caller's pairs (the arguments of FgmmAccAdd): checked, the messages prefixed by `who`, then uploaded with the frame of
  // every pair.  Returns their number; 0 before the buffers are looked at and before anything is uploaded.
  int64_t UploadPairs(const char* who, const float* host_feats, int64_t rows, const int32_t* post_off, const int32_t* post_idx, const float* post_w);
  // The counting sort of bucket_sort.h on `pairs` pairs whose Gaussians are d_gauss, as one segment; returns the ms when timed.
  float Sort(const int32_t* d_gauss, int64_t pairs, bool timed);
  // The work items, then `launch` (partial sums and reduction).  a: feats, rows, pairs, pair_frame / n, pair_w, sorted and
  // bucket_start; the rest is filled here.  refuse(bound on the items, bytes of partial sums) throws what the kind does not take.
  float Accumulate(FgmmAccArgs a, const std::function<void(int64_t, size_t)>& refuse, hipError_t (*launch)(const FgmmAccArgs&, hipStream_t),
                   const char* launch_name, bool timed);
  // any of the three may be null
  void Get(double* host_occ, double* host_mean, double* host_second, const char* second_what) const;
};

}  // namespace xv
