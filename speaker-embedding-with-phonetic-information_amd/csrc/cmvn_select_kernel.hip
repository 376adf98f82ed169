// The affine map of per-speaker CMVN behind a row selection: see cmvn_kernels.h for the launch and cmvn.h for the semantics.  A
// file of its own beside cmvn_kernels.hip, whose three kernels tests/test_cmvn_resources.py counts.
#include "cmvn_kernels.h"

// One rounding per operation, as in cmvn_kernels.hip: x * scale + offset must not become a fused multiply-add (the Makefile passes
// -ffp-contract=off as well; the pragma keeps any other compile line honest).
#pragma clang fp contract(off)

namespace xv {
namespace {

// Block b makes output rows [b * kCmvnSelectRows, ...): nr * cols elements, one thread per element, consecutive threads on
// consecutive elements of the OUTPUT (stores coalesce; the loads do wherever kept rows follow each other in the input, which is
// all of them without a selection and runs of them behind a voice activity decision).  What a row needs - where it comes from
// and which norm it takes, the end of the chain sel_utt -> utt_norm - is looked up once per row into LDS, so that the element
// loop has no load that waits for another global load and can keep several rows' elements in flight.  The row and the column
// of a thread's element are carried along from one element to the next - a division per thread, none per element.
static_assert(kCmvnSelectRows <= kCmvnThreads, "one thread per row looks the row up");
__global__ __launch_bounds__(kCmvnThreads) void cmvn_apply_select_kernel(const CmvnSelectArgs a) {
  __shared__ int32_t s_row[kCmvnSelectRows], s_norm[kCmvnSelectRows];
  const int cols = a.cols;
  const int r0 = blockIdx.x * kCmvnSelectRows;
  const int nr = a.n_out - r0 < kCmvnSelectRows ? a.n_out - r0 : kCmvnSelectRows;
  if ((int)threadIdx.x < nr) {
    s_row[threadIdx.x] = a.sel_row[r0 + threadIdx.x];
    s_norm[threadIdx.x] = a.utt_norm[a.sel_utt[r0 + threadIdx.x]];
  }
  __syncthreads();
  const int total = nr * cols;   // < 2^31: the launcher checks
  const int step_r = kCmvnThreads / cols, step_c = kCmvnThreads % cols;
  int r = (int)threadIdx.x / cols, c = (int)threadIdx.x - r * cols;
  float* dst = a.out + (int64_t)r0 * cols;
#pragma unroll 4
  for (int i = threadIdx.x; i < total; i += kCmvnThreads) {
    const float* offset = a.norms + (int64_t)s_norm[r] * 2 * cols;
    const float x = a.raw[(int64_t)s_row[r] * cols + c];
    const float prod = x * offset[cols + c];
    dst[i] = prod + offset[c];
    r += step_r;
    c += step_c;
    if (c >= cols) {
      c -= cols;
      ++r;
    }
  }
}

}  // namespace

hipError_t launch_cmvn_apply_select(const CmvnSelectArgs& a, hipStream_t s) {
  if (a.n_out < 0 || a.cols < 1 || a.cols > (INT32_MAX - kCmvnThreads) / kCmvnSelectRows) return hipErrorInvalidValue;
  if (a.n_out == 0) return hipSuccess;
  if (!a.raw || !a.norms || !a.utt_norm || !a.sel_row || !a.sel_utt || !a.out) return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((a.n_out + kCmvnSelectRows - 1) / kCmvnSelectRows);
  hipLaunchKernelGGL(cmvn_apply_select_kernel, dim3(blocks), dim3(kCmvnThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
