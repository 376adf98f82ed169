// Kernels of per-speaker CMVN: see cmvn_kernels.h for the launches and cmvn.h for the semantics.
#include "cmvn_kernels.h"

// One rounding per operation: x * scale + offset must not become a fused multiply-add (the Makefile passes -ffp-contract=off as
// well; the pragma keeps any other compile line honest).
#pragma clang fp contract(off)

namespace xv {
namespace {

__global__ __launch_bounds__(kCmvnThreads) void cmvn_stats_partial_kernel(const CmvnArgs a) {
  const int item = blockIdx.x;
  const int u = a.item_mat[item];
  const int r0 = a.item_blk[item] * kCmvnRowBlock;
  const int rows = a.row_off[u + 1] - a.row_off[u];
  const int nr = rows - r0 < kCmvnRowBlock ? rows - r0 : kCmvnRowBlock;
  const int cols = a.cols;
  const int tid = threadIdx.x;
  const float* src = a.feats + ((int64_t)a.row_off[u] + r0) * cols;
  double* dst = a.partial + (int64_t)item * 2 * cols;
  __shared__ double ssum[kCmvnThreads], ssq[kCmvnThreads];
  for (int c0 = 0; c0 < cols; c0 += kCmvnColTile) {
    const int gc = cols - c0 < kCmvnColTile ? cols - c0 : kCmvnColTile;
    const int R = kCmvnThreads / gc;   // rows in flight: thread (j, c) = j * gc + c
    const int j = tid / gc, c = tid - j * gc;
    double s = 0.0, q = 0.0;
    if (j < R) {
      const float* p = src + c0 + c;
#pragma unroll 4
      for (int r = j; r < nr; r += R) {
        const double x = (double)p[(int64_t)r * cols];
        s += x;
        q += x * x;   // exact: the square of a float has 48 significant bits
      }
    }
    ssum[tid] = s;
    ssq[tid] = q;
    __syncthreads();
    if (tid < gc) {
      double ts = 0.0, tq = 0.0;
      for (int k = 0; k < R; ++k) {
        ts += ssum[k * gc + tid];
        tq += ssq[k * gc + tid];
      }
      dst[c0 + tid] = ts;
      dst[cols + c0 + tid] = tq;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kCmvnThreads) void cmvn_stats_reduce_kernel(const CmvnArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * kCmvnThreads + threadIdx.x;
  const int w = a.cols + 1;
  if (idx >= (int64_t)a.n * w) return;
  const int u = (int)(idx / w), c = (int)(idx - (int64_t)u * w);
  double* st = a.stats + (int64_t)u * 2 * w;
  if (c == a.cols) {
    st[a.cols] = (double)(a.row_off[u + 1] - a.row_off[u]);
    st[w + a.cols] = 0.0;
    return;
  }
  double s = 0.0, q = 0.0;
  for (int i = a.mat_item0[u]; i < a.mat_item0[u + 1]; ++i) {
    const double* p = a.partial + (int64_t)i * 2 * a.cols;
    s += p[c];
    q += p[a.cols + c];
  }
  st[c] = s;
  st[w + c] = q;
}

__global__ __launch_bounds__(kCmvnThreads) void cmvn_apply_kernel(const CmvnArgs a) {
  const int item = blockIdx.x;
  const int u = a.item_mat[item];
  const int r0 = a.item_blk[item] * kCmvnRowBlock;
  const int rows = a.row_off[u + 1] - a.row_off[u];
  const int nr = rows - r0 < kCmvnRowBlock ? rows - r0 : kCmvnRowBlock;
  const int cols = a.cols;
  const float* offset = a.norms + (int64_t)a.utt_norm[u] * 2 * cols;
  const float* scale = offset + cols;
  const int64_t base = ((int64_t)a.row_off[u] + r0) * cols;
  const float* src = a.feats + base;
  float* dst = a.out + base;
  // the block's rows are one contiguous run of nr * cols < 2^31 elements (the launcher checks): a 32-bit index, and the column
  // carried along instead of a division per element
  const int total = nr * cols;
  const int step = kCmvnThreads % cols;
  int c = (int)threadIdx.x % cols;
  for (int i = threadIdx.x; i < total; i += kCmvnThreads) {
    const float prod = src[i] * scale[c];
    dst[i] = prod + offset[c];
    c += step;
    if (c >= cols) c -= cols;
  }
}

bool cmvn_items_ok(const CmvnArgs& a) {
  return a.n > 0 && a.cols > 0 && a.n_items > 0 && a.feats && a.row_off && a.item_mat && a.item_blk;
}

}  // namespace

hipError_t launch_cmvn_stats(const CmvnArgs& a, hipStream_t s) {
  if (a.n < 1 || a.cols < 1 || a.n_items < 0 || !a.row_off || !a.mat_item0 || !a.stats) return hipErrorInvalidValue;
  if (a.n_items > 0) {
    if (!cmvn_items_ok(a) || !a.partial) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cmvn_stats_partial_kernel, dim3((unsigned)a.n_items), dim3(kCmvnThreads), 0, s, a);
  }
  const int64_t total = (int64_t)a.n * (a.cols + 1);
  hipLaunchKernelGGL(cmvn_stats_reduce_kernel, dim3((unsigned)((total + kCmvnThreads - 1) / kCmvnThreads)), dim3(kCmvnThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cmvn_apply(const CmvnArgs& a, hipStream_t s) {
  if (!cmvn_items_ok(a) || !a.norms || !a.utt_norm || !a.out) return hipErrorInvalidValue;
  if (a.cols > (INT32_MAX - kCmvnThreads) / kCmvnRowBlock) return hipErrorInvalidValue;   // a block's run is indexed in 32 bits
  hipLaunchKernelGGL(cmvn_apply_kernel, dim3((unsigned)a.n_items), dim3(kCmvnThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
