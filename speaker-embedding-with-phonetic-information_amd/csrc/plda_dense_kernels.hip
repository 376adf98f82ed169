// Dense PLDA scoring and top-N statistics (plda_dense_kernels.h).  fp64; 256-thread workgroups.
#include "plda_dense_kernels.h"

#include <math.h>

namespace xv {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// Per enrolment row, one wave: [A1 | A2 | 0] and r.  m and var are plda_enroll_kernel's.
__global__ __launch_bounds__(256) void plda_dense_enroll_kernel(const DensePrepArgs a, int ks) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= a.n_u) return;
  const double n = a.num_u[k];
  double* row = a.a + (size_t)k * ks;
  double lg = 0.0, q = 0.0;
  for (int d = lane; d < a.dim; d += 64) {
    const double p = a.psi[d];
    const double m = n * p / (n * p + 1.0) * (double)a.u[(size_t)k * a.dim + d];
    const double var = 1.0 + p / (n * p + 1.0);
    const double iv = 1.0 / var;
    const double a1 = m * iv;
    row[d] = a1;
    row[a.dim + d] = 0.5 * (a.inv_psi1[d] - iv);
    lg += log(1.0 + p) - log(var);
    q = fma(m, a1, q);
  }
  for (int d = 2 * a.dim + lane; d < ks; d += 64) row[d] = 0.0;
  lg = wave_sum(lg);
  q = wave_sum(q);
  if (lane == 0) a.r[k] = 0.5 * lg - 0.5 * q;
}

// [v | v^2 | 0] per test row, a thread per element (v^2 of an fp32 value is exact in fp64).
__global__ __launch_bounds__(256) void plda_dense_test_kernel(const DensePrepArgs a, int ks) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)a.n_v * ks) return;
  const size_t j = e / ks;
  const int k = (int)(e - j * ks);
  double x = 0.0;
  if (k < 2 * a.dim) {
    const double v = (double)a.v[j * a.dim + (k < a.dim ? k : k - a.dim)];
    x = k < a.dim ? v : v * v;
  }
  a.b[e] = x;
}

// ---------------------------------------------------------------------------------------------------------------------
// A 64 x 64 tile of out per workgroup; both operands go through LDS kDenseKC columns of k at a time, the accumulators stay in
// registers over the whole k range.  Fragment maps of v_mfma_f64_16x16x4_f64 as in ivex_kernels.hip: lane (r16, kq) gives
// p[r16][kq] and q[r16][kq] and receives out[kq + 4 reg][r16].
__global__ __launch_bounds__(256) void plda_dense_gemm_kernel(const DenseGemmArgs a) {
  __shared__ double ps[kDenseTileM][kDenseKC + kDensePad], qs[kDenseTileN][kDenseKC + kDensePad];
  static_assert(kDenseTileM == 64 && kDenseTileN == 64 && kDenseKC == 32, "the thread maps below");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r16 = lane & 15, kq = lane >> 4;
  const int m0 = blockIdx.y * kDenseTileM, n0 = blockIdx.x * kDenseTileN;
  const int lk = tid & 31, lr = tid >> 5;   // staging: column of k, row (8 rows a pass)
  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < a.k_stride; k0 += kDenseKC) {
#pragma unroll
    for (int i = 0; i < kDenseTileM / 8; ++i) {
      const int r = lr + 8 * i;
      ps[r][lk] = m0 + r < a.m ? a.p[(size_t)(a.row0 + m0 + r) * a.k_stride + k0 + lk] : 0.0;
      qs[r][lk] = n0 + r < a.n ? a.q[(size_t)(n0 + r) * a.k_stride + k0 + lk] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kDenseKC; kk += 4) {
      double pa[2], qb[2];
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        pa[f] = ps[wm * 32 + f * 16 + r16][kk + kq];
        qb[f] = qs[wn * 32 + f * 16 + r16][kk + kq];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[i], qb[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn * 32 + j * 16 + r16;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = m0 + wm * 32 + i * 16 + kq + 4 * reg;
        if (row < a.m && col < a.n)
          a.out[(size_t)row * a.n + col] = acc[i][j][reg] + (a.row_add ? a.row_add[a.row0 + row] : a.col_add[col]);
      }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double topn_canon(double x) { return x == 0.0 ? 0.0 : x; }   // -0 -> +0
// larger double <=> larger key
__device__ __forceinline__ uint64_t topn_key(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  return b ^ ((b >> 63) ? 0xffffffffffffffffull : 0x8000000000000000ull);
}

// Wave w owns the columns [w L, (w + 1) L), L = ceil(cols / 4) rounded up to 64, and walks them 64 at a time.
__global__ __launch_bounds__(kTopnThreads) void topn_stats_kernel(const TopnArgs a) {
  __shared__ uint32_t hist[256];
  __shared__ uint64_t s_prefix;
  __shared__ uint32_t s_remaining;
  __shared__ uint32_t wave_ties[kTopnThreads / 64];
  __shared__ double wave_part[kTopnThreads / 64];
  static_assert(kTopnThreads == 256, "one thread per histogram bin, four waves");
  const double* x = a.x + (size_t)blockIdx.x * a.cols;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per_wave = ((a.cols + 3) / 4 + 63) / 64 * 64;
  const int c0 = wave * per_wave < a.cols ? wave * per_wave : a.cols;
  const int c1 = c0 + per_wave < a.cols ? c0 + per_wave : a.cols;

  // the key of the n-th largest value, eight bits a pass: `prefix` holds the bits found, `remaining` the rank among the keys
  // that share them, counted from the largest
  uint64_t prefix = 0, mask = 0;
  uint32_t remaining = (uint32_t)a.n;
  for (int shift = 56; shift >= 0; shift -= 8) {
    hist[tid] = 0u;
    __syncthreads();
    for (int c = c0 + lane; c < c1; c += 64) {
      const uint64_t key = topn_key(topn_canon(x[c]));
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t above = 0;
      int b = 255;
      for (; b > 0; --b) {
        if (above + hist[b] >= remaining) break;
        above += hist[b];
      }
      s_prefix = prefix | ((uint64_t)b << shift);
      s_remaining = remaining - above;
    }
    __syncthreads();
    prefix = s_prefix;
    remaining = s_remaining;
    mask |= 0xffull << shift;
  }
  const uint64_t nth = prefix;        // every larger key is selected,
  const uint32_t quota = remaining;   // and the first `quota` columns that hold this one
  if (quota == (uint32_t)a.n) {       // nothing is larger: the n values are one value, which is their mean exactly
    if (tid == 0) {
      a.mean[blockIdx.x] = __longlong_as_double((long long)(nth ^ ((nth >> 63) ? 0x8000000000000000ull : 0xffffffffffffffffull)));
      a.std[blockIdx.x] = 0.0;
    }
    return;                           // the whole workgroup
  }

  // columns equal to the n-th largest in the waves before this one
  uint32_t ties = 0;
  for (int cb = c0; cb < c1; cb += 64) {
    const int c = cb + lane;
    const bool tie = c < c1 && topn_key(topn_canon(x[c])) == nth;
    ties += (uint32_t)__popcll(__ballot(tie));
  }
  if (lane == 0) wave_ties[wave] = ties;
  __syncthreads();
  uint32_t before = 0;
  for (int w = 0; w < wave; ++w) before += wave_ties[w];

  // pass 0: the mean; pass 1: the squared deviations from it
  double mean = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    double acc = 0.0;
    uint32_t seen = before;
    for (int cb = c0; cb < c1; cb += 64) {
      const int c = cb + lane;
      const bool in = c < c1;
      const double v = in ? topn_canon(x[c]) : 0.0;
      const uint64_t key = topn_key(v);
      const bool tie = in && key == nth;
      const uint64_t tied = __ballot(tie);
      const uint32_t rank = seen + (uint32_t)__popcll(tied & ((1ull << lane) - 1ull));
      const bool sel = in && (key > nth || (tie && rank < quota));
      if (pass == 0) {
        acc += sel ? v : 0.0;
      } else {
        const double d = sel ? v - mean : 0.0;
        acc = fma(d, d, acc);
      }
      seen += (uint32_t)__popcll(tied);
    }
    acc = wave_sum(acc);
    __syncthreads();   // the partials of pass 0 have been read
    if (lane == 0) wave_part[wave] = acc;
    __syncthreads();
    const double total = ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
    if (pass == 0) {
      mean = total / (double)a.n;
    } else if (tid == 0) {
      a.mean[blockIdx.x] = mean;
      a.std[blockIdx.x] = sqrt(total / (double)a.n);
    }
  }
}

}  // namespace

hipError_t launch_plda_dense_prep(const DensePrepArgs& a, hipStream_t s) {
  if (a.dim < 1 || a.dim > kPldaMaxDim || a.n_u < 0 || a.n_v < 0) return hipErrorInvalidValue;
  const int ks = dense_k_stride(a.dim);
  if (a.n_u > 0) {
    hipLaunchKernelGGL(plda_dense_enroll_kernel, dim3((a.n_u + 3) / 4), dim3(256), 0, s, a, ks);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (a.n_v > 0) {
    const size_t n = (size_t)a.n_v * ks;
    hipLaunchKernelGGL(plda_dense_test_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, ks);
    return hipGetLastError();
  }
  return hipSuccess;
}

hipError_t launch_plda_dense_gemm(const DenseGemmArgs& a, hipStream_t s) {
  if (a.m <= 0 || a.n <= 0) return hipSuccess;
  if (a.k_stride < kDenseKC || a.k_stride % kDenseKC != 0 || (a.row_add != nullptr) == (a.col_add != nullptr))
    return hipErrorInvalidValue;
  const unsigned gx = (unsigned)((a.n + kDenseTileN - 1) / kDenseTileN), gy = (unsigned)((a.m + kDenseTileM - 1) / kDenseTileM);
  if (gy > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(plda_dense_gemm_kernel, dim3(gx, gy), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_topn_stats(const TopnArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  if (a.cols < 2 || a.cols > kTopnMaxCols || a.n < 2 || a.n > a.cols || a.rows > 0x7fffffffll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(topn_stats_kernel, dim3((unsigned)a.rows), dim3(kTopnThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
