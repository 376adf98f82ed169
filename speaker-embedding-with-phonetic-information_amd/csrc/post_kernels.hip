// Kernels of logprob-to-post: see post_kernels.h for the launches and post.h for the semantics.
#include "post_kernels.h"

#include "counter_rng.h"

namespace xv {
namespace {

constexpr int kWave = 64;
constexpr int kLoads = kPostTile / kWave;
static_assert(kPostTile % kWave == 0 && kPostThreads % kWave == 0, "whole waves");

// Largest u with off[u] <= r (off non-decreasing, off[0] <= r < off[n]); empty utterances are stepped over.
__device__ inline int find_segment(const int32_t* off, int n, int64_t r) {
  int lo = 0, hi = n;   // answer in [lo, hi)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= r) lo = mid;
    else hi = mid;
  }
  return lo;
}

// What a wave knows about its row.
struct Row {
  const float* x;
  uint64_t seed;
  uint32_t t;   // the row's index within its utterance
};

// The fate of column c of the row: true and *v for a kept column.  NaN is dropped and flagged.
__device__ inline bool decide(const LogprobPostArgs& a, const Row& row, float x, uint32_t c, float* v, bool* is_nan) {
  *is_nan = x != x;
  if (*is_nan) return false;
  const float p = expf(x);
  *v = p;
  if (!(a.min_post > 0.f) || p >= a.min_post) return true;
  if (!a.random_prune) return false;
  const float q = p / a.min_post;
  // u is at least 2^-24: below that nothing is kept and nothing is drawn
  if (!(q >= 1.0f / 16777216.0f)) return false;
  *v = a.min_post;
  return q >= counter_unit_open0(counter_bits(row.seed, row.t, c));
}

// One wave, one row: kept columns are numbered in ascending column order.  WRITE: the pairs go to idx / w from off[r] on.
template <bool WRITE>
__global__ __launch_bounds__(kPostThreads) void logprob_post_kernel(const LogprobPostArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t r = (int64_t)blockIdx.x * (kPostThreads / kWave) + (threadIdx.x >> 6);
  if (r >= a.rows) return;   // the whole wave
  Row row;
  row.x = a.x + r * a.cols;
  row.seed = 0;
  row.t = 0;
  if (a.random_prune && a.min_post > 0.f) {
    const int u = find_segment(a.row_off, a.n_utts, a.row0 + r);
    row.seed = a.utt_seed[u];
    row.t = (uint32_t)(a.row0 + r - a.row_off[u]);
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  int64_t base = WRITE ? (int64_t)a.off[r] : 0;   // WRITE: the next free slot; else the count so far
  int nans = 0;
  for (int64_t c0 = 0; c0 < a.cols; c0 += kPostTile) {
    float x[kLoads];
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
      const int64_t c = c0 + k * kWave + lane;
      x[k] = c < a.cols ? row.x[c] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
      const int64_t c = c0 + k * kWave + lane;
      float v = 0.f;
      bool is_nan = false;
      const bool keep = c < a.cols && decide(a, row, x[k], (uint32_t)c, &v, &is_nan);
      const unsigned long long kept = __ballot(keep);
      if (WRITE) {
        if (keep) {
          const int64_t slot = base + __popcll(kept & below);
          a.idx[slot] = (int32_t)c;
          a.w[slot] = v;
        }
      } else {
        nans += __popcll(__ballot(c < a.cols && is_nan));
      }
      base += __popcll(kept);
    }
  }
  if (!WRITE && lane == 0) {
    a.count[r] = (int32_t)base;
    a.nan[r] = nans;
  }
}

// off[0 .. rows] = exclusive prefix sums of count.  Thread i owns the rows [i per, (i + 1) per).
__global__ __launch_bounds__(kPostScanThreads) void logprob_post_scan_kernel(const LogprobPostArgs a) {
  __shared__ int32_t part[kPostScanThreads];
  const int tid = threadIdx.x;
  const int per = (a.rows + kPostScanThreads - 1) / kPostScanThreads;
  const int64_t lo64 = (int64_t)tid * per;
  const int lo = lo64 < a.rows ? (int)lo64 : a.rows, hi = lo64 + per < a.rows ? (int)(lo64 + per) : a.rows;
  int32_t s = 0;
  for (int r = lo; r < hi; ++r) s += a.count[r];
  part[tid] = s;
  __syncthreads();
  int32_t base = 0;
  for (int i = 0; i < tid; ++i) base += part[i];
  for (int r = lo; r < hi; ++r) {
    a.off[r] = base;
    base += a.count[r];
  }
  if (tid == kPostScanThreads - 1) a.off[a.rows] = base;
}

}  // namespace

hipError_t launch_logprob_post_count(const LogprobPostArgs& a, hipStream_t s) {
  if (a.rows < 1) return hipSuccess;
  const unsigned grid = (unsigned)(((int64_t)a.rows + kPostThreads / kWave - 1) / (kPostThreads / kWave));
  hipLaunchKernelGGL(logprob_post_kernel<false>, dim3(grid), dim3(kPostThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_logprob_post_scan(const LogprobPostArgs& a, hipStream_t s) {
  if (a.rows < 1) return hipSuccess;
  hipLaunchKernelGGL(logprob_post_scan_kernel, dim3(1), dim3(kPostScanThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_logprob_post_write(const LogprobPostArgs& a, hipStream_t s) {
  if (a.rows < 1) return hipSuccess;
  const unsigned grid = (unsigned)(((int64_t)a.rows + kPostThreads / kWave - 1) / (kPostThreads / kWave));
  hipLaunchKernelGGL(logprob_post_kernel<true>, dim3(grid), dim3(kPostThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
