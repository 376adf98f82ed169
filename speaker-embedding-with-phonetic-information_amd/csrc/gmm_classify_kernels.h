// Device kernel of the GMM classifier tools (fgmm-gselect; semantics in gmm_classify.h).  Kept out of ubm_kernels.hip, whose kernels
// are counted by a test; the scores it ranks are ubm_full_loglike's (ubm_kernels.h), unchanged.
//   ubm_full_rerank    one wave per frame, lane = slot of the preselection.  A lane holds its slot's score as the order-preserving
//                      integer key of ubm_diag_gselect, and its Gaussian.  Slot j's pair is broadcast from lane j (v_readlane, a
//                      scalar operand: no LDS, no atomics, no scratch) for j = 0 .. n_in - 1, and every lane counts the slots that
//                      precede its own in the total order (score descending, Gaussian ascending, slot ascending).  That count is
//                      the lane's rank; the lanes with rank < n_keep store (Gaussian, score) at it.  Integer work only: a frame's
//                      result is a function of its n_in pairs alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace xv {

constexpr int kRerankThreads = 256;
constexpr int kRerankFramesPerBlock = 4;   // frames per workgroup of the rerank kernel: one per wave (kRerankThreads / 64)

struct UbmRerankArgs {
  int64_t rows;
  int n_in;                   // slots per frame, 1 <= n_in <= kUbmMaxSelect (the lanes of a wave)
  int n_keep;                 // 1 <= n_keep <= n_in
  const int32_t* preselect;   // [rows][n_in] the Gaussian of every slot
  const float* ll;            // [rows][n_in] its score
  int32_t* out_idx;           // [rows][n_keep] best first
  float* out_ll;              // [rows][n_keep] or null
};

hipError_t launch_ubm_full_rerank(const UbmRerankArgs& a, hipStream_t s);

}  // namespace xv
