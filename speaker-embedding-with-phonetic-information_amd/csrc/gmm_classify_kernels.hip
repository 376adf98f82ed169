// Kernel of the GMM classifier tools: see gmm_classify_kernels.h for the launch and gmm_classify.h for the semantics.
#include "gmm_classify_kernels.h"

#include "ubm_kernels.h"

namespace xv {
namespace {

static_assert(kRerankThreads == 64 * kRerankFramesPerBlock, "one wave per frame");
static_assert(kUbmMaxSelect <= 64, "a slot per lane");

// float -> unsigned key with the same order (and a place for every NaN): ubm_diag_gselect's, the two zeros one score
__device__ inline uint32_t score_key(float x) {
  const uint32_t b = __float_as_uint(x + 0.f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(kRerankThreads) void ubm_full_rerank_kernel(const UbmRerankArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * kRerankFramesPerBlock + wave;
  if (t >= a.rows) return;   // the whole wave
  const int n_in = a.n_in, n_keep = a.n_keep;
  const bool live = lane < n_in;
  float score = 0.f;
  int32_t g = 0;
  if (live) {
    score = a.ll[t * n_in + lane];
    g = a.preselect[t * n_in + lane];
  }
  const uint32_t key = score_key(score);
  int rank = 0;
  for (int j = 0; j < n_in; ++j) {   // j is the same in every lane: the reads below are scalar broadcasts
    const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)key, j);
    const int32_t gj = __builtin_amdgcn_readlane(g, j);
    // no short circuit: four compares and no branch
    rank += (int)((kj > key) | ((kj == key) & ((gj < g) | ((gj == g) & (j < lane)))));
  }
  if (live && rank < n_keep) {
    a.out_idx[t * n_keep + rank] = g;
    if (a.out_ll) a.out_ll[t * n_keep + rank] = score;
  }
}

}  // namespace

hipError_t launch_ubm_full_rerank(const UbmRerankArgs& a, hipStream_t s) {
  if (a.rows < 1 || a.n_in < 1 || a.n_in > kUbmMaxSelect || a.n_keep < 1 || a.n_keep > a.n_in || !a.preselect || !a.ll || !a.out_idx)
    return hipErrorInvalidValue;
  const int64_t blocks = (a.rows + kRerankFramesPerBlock - 1) / kRerankFramesPerBlock;
  if (blocks > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ubm_full_rerank_kernel, dim3((unsigned)blocks), dim3(kRerankThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
