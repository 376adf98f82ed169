// Device kernels of i-vector extractor training: see ivex_train_kernels.h for what each one does and ivex_train.h for the semantics.
#include "ivex_train_kernels.h"

#include <math.h>

#include "ivex_kernels.h"

namespace xv {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ inline int64_t tri(int64_t r) { return r * (r + 1) / 2; }

constexpr int kThreads = kIvexTrainThreads;
constexpr int kPostThreads = kIvexPosteriorThreads;
constexpr int kColsPerThread = kIvexMaxS / kPostThreads;   // columns of Z a thread owns at the largest S
constexpr int kShares = 5;                             // tr Var, tr(Var Q_a), m' Q_a m, l_a . m, |m - p e_0|^2
static_assert(kIvexMaxS % kPostThreads == 0 && (kPostThreads & (kPostThreads - 1)) == 0 && kIvexTrainSlots <= 256 && kIvexTrainSlots % 4 == 0, "the training kernels' thread maps");

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPostThreads) void ivex_posterior_kernel(const IvexPosteriorArgs a) {
  __shared__ double ms[kIvexMaxS];
  __shared__ double red[kShares][kPostThreads];
  const int tid = threadIdx.x, S = a.S, G = a.G, D = a.D;
  const int u = a.src[blockIdx.x], slot = a.slot[blockIdx.x];
  const int64_t P = tri(S);
  const double* L = a.work + (int64_t)u * (S + 1) * S;
  const double* Qp = a.quadratic + (int64_t)u * P;
  const double* l = a.linear + (int64_t)u * S;
  double* Z = a.zwork + (int64_t)slot * S * S;
  for (int c = tid; c < S; c += kPostThreads) ms[c] = a.solution[(int64_t)u * S + c];

  // 1. Z = L^-1 by rows.  Thread tid owns columns tid, tid + kPostThreads, ...: what it reads of Z it wrote itself.
  const int k_first = tid & ~63;   // the wave's lowest column: rows of Z above it are zero in every column of the wave
  for (int i = 0; i < S; ++i) {
    const double* Li = L + (int64_t)i * S;
    double acc[kColsPerThread];
#pragma unroll
    for (int m = 0; m < kColsPerThread; ++m) acc[m] = 0.0;
#pragma unroll 8
    for (int k = k_first; k < i; ++k) {   // unrolled so that the loads of several k are in flight; the sums stay in k order
      const double lik = Li[k];
      const double* Zk = Z + (int64_t)k * S;
#pragma unroll
      for (int m = 0; m < kColsPerThread; ++m) {
        const int c = tid + m * kPostThreads;
        if (c <= k) acc[m] += lik * Zk[c];   // c <= k < i < S
      }
    }
    const double d = Li[i];
#pragma unroll
    for (int m = 0; m < kColsPerThread; ++m) {
      const int c = tid + m * kPostThreads;
      if (c <= i) Z[(int64_t)i * S + c] = ((c == i ? 1.0 : 0.0) - acc[m]) / d;
    }
  }
  __syncthreads();   // the other threads' columns of Z, and ms

  // 2. Var = Z' Z, the scatter and the shares of the traces
  const double p = a.prior_offset;
  double tr_var = 0.0, tr_var_q = 0.0, m_q_m = 0.0;
  double* scatter = a.p_scatter + (int64_t)slot * P;
  for (int64_t e = tid; e < P; e += kPostThreads) {
    int r = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
    while (tri(r) > e) --r;
    while (tri(r + 1) <= e) ++r;
    const int c = (int)(e - tri(r));   // r >= c
    double var = 0.0;
#pragma unroll 8
    for (int k = r; k < S; ++k) var += Z[(int64_t)k * S + r] * Z[(int64_t)k * S + c];
    const double mm = ms[r] * ms[c];
    scatter[e] = var + mm;
    const double qa = Qp[e] - (r == c ? 1.0 : 0.0);
    const double twice = r == c ? 1.0 : 2.0;
    if (r == c) tr_var += var;
    tr_var_q += twice * var * qa;
    m_q_m += twice * mm * qa;
  }
  double la_m = 0.0, dist = 0.0;
  for (int j = tid; j < S; j += kPostThreads) {
    const double off = j == 0 ? p : 0.0;
    la_m += (l[j] - off) * ms[j];
    dist += (ms[j] - off) * (ms[j] - off);
  }
  red[0][tid] = tr_var;
  red[1][tid] = tr_var_q;
  red[2][tid] = m_q_m;
  red[3][tid] = la_m;
  red[4][tid] = dist;
  __syncthreads();
  for (int step = kPostThreads / 2; step > 0; step >>= 1) {
    if (tid < step) {
#pragma unroll
      for (int q = 0; q < kShares; ++q) red[q][tid] += red[q][tid + step];
    }
    __syncthreads();
  }
  // 3. and 4.
  if (tid == 0) {
    double sum_log = 0.0;
    for (int i = 0; i < S; ++i) sum_log += log(L[(int64_t)i * S + i]);
    const double logdet = -2.0 * sum_log;
    a.p_logdet[slot] = logdet;
    a.p_auxf[slot] = red[3][0] - 0.5 * red[2][0] - 0.5 * red[1][0] - 0.5 * (red[4][0] + red[0][0]) + 0.5 * logdet + 0.5 * (double)S;
  }
  // 5.
  for (int c = tid; c < S; c += kPostThreads) a.p_m[(int64_t)slot * S + c] = ms[c];
  for (int g = tid; g < G; g += kPostThreads) a.p_gamma[(int64_t)slot * G + g] = a.gamma[(int64_t)u * G + g];
  const int64_t K = (int64_t)G * D;
  for (int64_t e = tid; e < K; e += kPostThreads) a.p_X[(int64_t)slot * K + e] = a.X[(int64_t)u * K + e];
}

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ivex_rank_update_kernel(const IvexRankUpdateArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const int64_t row0 = ((int64_t)blockIdx.x * (kThreads / 64) + wave) * 16;
  if (row0 >= a.M) return;   // the whole wave: nothing here waits on it
  const int64_t arow = row0 + r16;
  double av[kIvexTrainSlots / 4];
#pragma unroll
  for (int step = 0; step < kIvexTrainSlots / 4; ++step) {
    const int k = 4 * step + kq;
    av[step] = (k < a.count && arow < a.M) ? a.A[(int64_t)k * a.M + arow] : 0.0;
  }
  for (int ct = 0; ct < kIvexRankColTiles; ++ct) {
    const int64_t col0 = ((int64_t)blockIdx.y * kIvexRankColTiles + ct) * 16;
    if (col0 >= a.N) break;
    const int64_t col = col0 + r16;
    const bool col_in = col < a.N;
    f64x4 c;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t row = row0 + kq + 4 * reg;   // the f64 map of ivex_kernels.h
      c[reg] = (col_in && row < a.M) ? a.C[row * a.ldc + col] : 0.0;
    }
#pragma unroll
    for (int step = 0; step < kIvexTrainSlots / 4; ++step) {
      const int k = 4 * step + kq;
      const double b = (k < a.count && col_in) ? a.B[(int64_t)k * a.N + col] : 0.0;
      c = __builtin_amdgcn_mfma_f64_16x16x4f64(av[step], b, c, 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t row = row0 + kq + 4 * reg;
      if (col_in && row < a.M) a.C[row * a.ldc + col] = c[reg];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ivex_small_sums_kernel(const IvexSmallSumsArgs a) {
  const int64_t P = tri(a.S);
  const int64_t total = (int64_t)a.G + a.S + P + 1;
  int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  const double* src;
  double* dst;
  int64_t stride;
  if (e < a.G) {
    src = a.p_gamma + e;
    dst = a.gamma + e;
    stride = a.G;
  } else if ((e -= a.G) < a.S) {
    src = a.p_m + e;
    dst = a.ivector_sum + e;
    stride = a.S;
  } else if ((e -= a.S) < P) {
    src = a.p_scatter + e;
    dst = a.ivector_scatter + e;
    stride = P;
  } else {
    src = a.p_auxf;
    dst = a.auxf;
    stride = 1;
  }
  double sum = 0.0;
  for (int k = 0; k < a.count; ++k) sum += src[(int64_t)k * stride];
  *dst += sum;
}

}  // namespace

hipError_t launch_ivex_posterior(const IvexPosteriorArgs& a, hipStream_t s) {
  if (a.n < 1) return hipSuccess;
  if (a.n > kIvexTrainSlots || a.S < 1 || a.S > kIvexMaxS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ivex_posterior_kernel, dim3((unsigned)a.n), dim3(kPostThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ivex_rank_update(const IvexRankUpdateArgs& a, hipStream_t s) {
  if (a.count < 0 || a.count > kIvexTrainSlots || a.M < 0 || a.N < 0 || a.ldc < a.N) return hipErrorInvalidValue;
  if (a.count == 0 || a.M == 0 || a.N == 0) return hipSuccess;
  const int64_t gx = (a.M + 63) / 64, gy = (a.N + 16 * kIvexRankColTiles - 1) / (16 * kIvexRankColTiles);
  if (gx > INT32_MAX || gy > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ivex_rank_update_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ivex_small_sums(const IvexSmallSumsArgs& a, hipStream_t s) {
  if (a.count < 1) return hipSuccess;
  const int64_t total = (int64_t)a.G + a.S + (int64_t)a.S * (a.S + 1) / 2 + 1;
  hipLaunchKernelGGL(ivex_small_sums_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
