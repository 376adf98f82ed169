// Device kernels of i-vector extraction: see ivex_kernels.h for what each one does and ivex.h for the semantics.
#include "ivex_kernels.h"

#include <math.h>

namespace xv {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ inline int64_t tri(int64_t r) { return r * (r + 1) / 2; }

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kIvexThreads) void ivex_derive_kernel(const IvexDeriveArgs a) {
  __shared__ double sig[kIvexMaxDim * (kIvexMaxDim + 1) / 2];
  const int g = blockIdx.x, tid = threadIdx.x, D = a.D, S = a.S;
  const int tri_d = D * (D + 1) / 2;
  const int64_t P = tri(S);
  for (int e = tid; e < tri_d; e += kIvexThreads) sig[e] = a.sigma_inv[(int64_t)g * tri_d + e];
  __syncthreads();
  const double* M = a.M + (int64_t)g * D * S;
  double* sim = a.sigma_inv_m + (int64_t)g * D * S;
  for (int e = tid; e < D * S; e += kIvexThreads) {
    const int i = e / S, s = e - i * S;
    double sum = 0.0;
    for (int j = 0; j < D; ++j) {
      const double v = j <= i ? sig[i * (i + 1) / 2 + j] : sig[j * (j + 1) / 2 + i];
      sum += v * M[(int64_t)j * S + s];
    }
    sim[e] = sum;
  }
  __syncthreads();   // the workgroup reads back what it wrote
  double* U = a.U + (int64_t)g * P;
  for (int64_t e = tid; e < P; e += kIvexThreads) {
    int r = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
    while (tri(r) > e) --r;
    while (tri(r + 1) <= e) ++r;
    const int c = (int)(e - tri(r));
    double sum = 0.0;
    for (int i = 0; i < D; ++i) sum += M[(int64_t)i * S + r] * sim[(int64_t)i * S + c];
    U[e] = sum;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// One wave per (utterance, Gaussian); lane d owns columns d and d + 64.
__global__ __launch_bounds__(kIvexThreads) void ivex_stats_kernel(const IvexStatsArgs a) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * (kIvexThreads / 64) + (threadIdx.x >> 6), u = blockIdx.y;
  if (g >= a.G) return;
  const int D = a.D;
  const int32_t* start = a.bucket_start + (int64_t)u * (a.G + 1);
  const int lo = start[g], hi = start[g + 1];
  double gamma = 0.0, x0 = 0.0, x1 = 0.0;
  for (int i = lo; i < hi; ++i) {
    const int p = a.sorted[i];
    const double w = (double)a.pair_w[p];
    const float* row = a.feats + (int64_t)a.pair_frame[p] * D;
    gamma += w;
    if (lane < D) x0 += w * (double)row[lane];
    if (lane + 64 < D) x1 += w * (double)row[lane + 64];
  }
  double* X = a.X + ((int64_t)u * a.G + g) * D;
  if (lane < D) X[lane] = x0;
  if (lane + 64 < D) X[lane + 64] = x1;
  if (lane == 0) a.gamma[(int64_t)u * a.G + g] = gamma;
}

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kIvexThreads) void ivex_gemm_kernel(const IvexGemmArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t col0 = ((int64_t)blockIdx.x * (kIvexThreads / 64) + wave) * kIvexColTile;
  if (col0 >= a.N) return;   // the whole wave: nothing here waits on it
  const int64_t col = col0 + (lane & 15);
  const int kq = lane >> 4, r16 = lane & 15;
  const int64_t k_begin = (int64_t)blockIdx.y * a.k_chunk;
  const int64_t k_end = k_begin + a.k_chunk < a.K ? k_begin + a.k_chunk : a.K;
  const bool col_in = col < a.N;
  f64x4 acc[kIvexMaxRowTiles];
#pragma unroll
  for (int rt = 0; rt < kIvexMaxRowTiles; ++rt) acc[rt] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int64_t k = k_begin; k < k_end; k += 16) {
#pragma unroll
    for (int step = 0; step < 4; ++step) {   // four k steps in flight; a step beyond the chunk multiplies zeros
      const int64_t kk = k + 4 * step + kq;
      const bool k_in = kk < k_end;
      const double b = (k_in && col_in) ? a.W[kk * a.N + col] : 0.0;
#pragma unroll
      for (int rt = 0; rt < kIvexMaxRowTiles; ++rt) {
        if (rt * kIvexRowTile < a.B) {
          const int row = rt * kIvexRowTile + r16;
          const double av = (k_in && row < a.B) ? a.A[(int64_t)row * a.K + kk] : 0.0;
          acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b, acc[rt], 0, 0, 0);
        }
      }
    }
  }
  if (!col_in) return;
  double* C = a.C + (int64_t)blockIdx.y * a.B * a.N;
#pragma unroll
  for (int rt = 0; rt < kIvexMaxRowTiles; ++rt) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = rt * kIvexRowTile + kq + 4 * reg;   // the f64 map: not (lane >> 4) * 4 + reg
      if (row < a.B) C[(int64_t)row * a.N + col] = acc[rt][reg];
    }
  }
}

__global__ __launch_bounds__(kIvexThreads) void ivex_finish_terms_kernel(const IvexFinishArgs a) {
  const int u = blockIdx.x, S = a.S;
  for (int s = threadIdx.x; s < S; s += kIvexThreads) {
    double sum = 0.0;
    for (int c = 0; c < a.chunks; ++c) sum += a.partial[((int64_t)c * a.B + u) * S + s];
    if (s == 0) sum += a.prior_offset;
    a.linear[(int64_t)u * S + s] = sum;
  }
  double* Q = a.quadratic + (int64_t)u * tri(S);
  for (int r = threadIdx.x; r < S; r += kIvexThreads) Q[tri(r) + r] += 1.0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int NB = kIvexPanel;
constexpr int kSolveRowTile = kIvexThreads / 4;   // rows per pass of the block-column update: 4 threads of 8 columns per row
static_assert(NB == 32 && kIvexThreads == 256 && kIvexMaxS <= 4 * kIvexThreads, "the solve's thread maps");

__global__ __launch_bounds__(kIvexThreads) void ivex_solve_kernel(const IvexSolveArgs a) {
  __shared__ double Lp[NB][NB + 1];   // [column of the block][k]: rows k0 .. k0 + nb of L, columns kk .. kk + NB
  __shared__ double Dg[NB][NB + 1];   // the diagonal block, the identity beyond nb
  __shared__ double ys[kIvexMaxS], xs[kIvexMaxS], dg[kIvexMaxS];
  __shared__ double red[kIvexThreads];
  __shared__ int bad;
  const int u = blockIdx.x, tid = threadIdx.x, S = a.S;
  const double* Qp = a.quadratic + (int64_t)u * tri(S);
  const double* l = a.linear + (int64_t)u * S;
  double* A = a.work + (int64_t)u * (S + 1) * S;
  const int rows = S + 1;   // the last row is l: the factorisation turns it into y = L^-1 l
  if (tid == 0) bad = 0;
  for (int r = 0; r < S; ++r)
    for (int c = tid; c <= r; c += kIvexThreads) A[(int64_t)r * S + c] = Qp[tri(r) + c];
  for (int c = tid; c < S; c += kIvexThreads) A[(int64_t)S * S + c] = l[c];
  __syncthreads();

  for (int k0 = 0; k0 < S; k0 += NB) {
    const int nb = S - k0 < NB ? S - k0 : NB;
    // the block column minus what the columns before it contribute, k ascending
    if (k0 > 0) {
      const int cg = (tid & 3) * 8;
      for (int i0 = k0; i0 < rows; i0 += kSolveRowTile) {
        const int i = i0 + (tid >> 2);
        double acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = 0.0;
        for (int kk = 0; kk < k0; kk += NB) {
          __syncthreads();
          for (int e = tid; e < NB * NB; e += kIvexThreads) {
            const int c = e / NB, k = e % NB;
            Lp[c][k] = c < nb ? A[(int64_t)(k0 + c) * S + kk + k] : 0.0;
          }
          __syncthreads();
          if (i < rows) {
            const double* ai = A + (int64_t)i * S + kk;
#pragma unroll 8
            for (int k = 0; k < NB; ++k) {
              const double av = ai[k];
#pragma unroll
              for (int c = 0; c < 8; ++c) acc[c] += av * Lp[cg + c][k];
            }
          }
        }
        if (i < rows) {
#pragma unroll
          for (int c = 0; c < 8; ++c)
            if (cg + c < nb && k0 + cg + c <= i) A[(int64_t)i * S + k0 + cg + c] -= acc[c];
        }
      }
      __syncthreads();
    }
    // the diagonal block, in LDS
    for (int e = tid; e < NB * NB; e += kIvexThreads) {
      const int r = e / NB, c = e % NB;
      Dg[r][c] = (r < nb && c <= r) ? A[(int64_t)(k0 + r) * S + k0 + c] : (r == c ? 1.0 : 0.0);
    }
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
      if (tid == 0) {
        double d = Dg[j][j];
        if (!(d > 0.0) || !isfinite(d)) {   // not positive definite: flag it and go on with numbers that stay finite
          bad = 1;
          d = 1.0;
        }
        Dg[j][j] = sqrt(d);
      }
      __syncthreads();
      if (tid > j && tid < nb) Dg[tid][j] /= Dg[j][j];
      __syncthreads();
      for (int e = tid; e < NB * NB; e += kIvexThreads) {
        const int r = e / NB, c = e % NB;
        if (c > j && c <= r && r < nb) Dg[r][c] -= Dg[r][j] * Dg[c][j];
      }
      __syncthreads();
    }
    for (int e = tid; e < NB * NB; e += kIvexThreads) {
      const int r = e / NB, c = e % NB;
      if (r < nb && c <= r) A[(int64_t)(k0 + r) * S + k0 + c] = Dg[r][c];
    }
    // the rows below the block: row . (diagonal block)^-T, one thread per row, eight columns at a time (the columns before
    // them are read back from the row itself)
    for (int i = k0 + nb + tid; i < rows; i += kIvexThreads) {
      double* ai = A + (int64_t)i * S + k0;
#pragma unroll 1
      for (int c0 = 0; c0 < nb; c0 += 8) {
        double x[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) x[c] = c0 + c < nb ? ai[c0 + c] : 0.0;
#pragma unroll 1
        for (int m = 0; m < c0; ++m) {
          const double am = ai[m];
#pragma unroll
          for (int c = 0; c < 8; ++c) x[c] -= am * Dg[c0 + c][m];
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          double v = x[c];
#pragma unroll
          for (int m = 0; m < c; ++m) v -= x[m] * Dg[c0 + c][c0 + m];
          x[c] = v / Dg[c0 + c][c0 + c];
        }
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (c0 + c < nb) ai[c0 + c] = x[c];
      }
    }
    __syncthreads();
  }

  // L' x = y, backwards; row j of L is read one step ahead of its use
  for (int c = tid; c < S; c += kIvexThreads) {
    ys[c] = A[(int64_t)S * S + c];
    dg[c] = A[(int64_t)c * S + c];
  }
  double nxt[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int i = tid + m * kIvexThreads;
    nxt[m] = i < S - 1 ? A[(int64_t)(S - 1) * S + i] : 0.0;
  }
  __syncthreads();
  for (int j = S - 1; j >= 0; --j) {
    double cur[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      cur[m] = nxt[m];
      const int i = tid + m * kIvexThreads;
      nxt[m] = (j > 0 && i < j - 1) ? A[(int64_t)(j - 1) * S + i] : 0.0;
    }
    const double xj = ys[j] / dg[j];
    if (tid == 0) xs[j] = xj;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int i = tid + m * kIvexThreads;
      if (i < j) ys[i] -= cur[m] * xj;
    }
    __syncthreads();
  }
  for (int c = tid; c < S; c += kIvexThreads)
    if (!isfinite(xs[c])) bad = 1;
  __syncthreads();
  const bool fail = bad != 0;
  for (int c = tid; c < S; c += kIvexThreads)
    a.ivector[(int64_t)u * S + c] = fail ? 0.f : (float)(xs[c] - (c == 0 ? a.prior_offset : 0.0));
  if (tid == 0) a.status[u] = fail ? 1 : 0;
  if (a.solution)
    for (int c = tid; c < S; c += kIvexThreads) a.solution[(int64_t)u * S + c] = fail ? 0.0 : xs[c];
  if (!a.auxf_change) return;
  // F(x) - F(p e_0), F(v) = l . v - v' Q v / 2, from the unfactored Q
  double t = 0.0;
  for (int j = tid; j < S; j += kIvexThreads) {
    double r = 0.0;
    for (int k = 0; k < S; ++k) r += (k <= j ? Qp[tri(j) + k] : Qp[tri(k) + j]) * xs[k];
    t += xs[j] * (l[j] - 0.5 * r);
  }
  red[tid] = t;
  __syncthreads();
  for (int step = kIvexThreads / 2; step > 0; step >>= 1) {
    if (tid < step) red[tid] += red[tid + step];
    __syncthreads();
  }
  if (tid == 0) {
    const double p = a.prior_offset;
    const double f0 = l[0] * p - 0.5 * p * p * Qp[0];
    const double d = red[0] - f0;
    a.auxf_change[u] = (fail || !isfinite(d)) ? 0.0 : d;
  }
}

}  // namespace

hipError_t launch_ivex_derive(const IvexDeriveArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ivex_derive_kernel, dim3((unsigned)a.G), dim3(kIvexThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ivex_stats(const IvexStatsArgs& a, hipStream_t s) {
  const unsigned gx = (unsigned)((a.G + kIvexThreads / 64 - 1) / (kIvexThreads / 64));
  hipLaunchKernelGGL(ivex_stats_kernel, dim3(gx, (unsigned)a.B), dim3(kIvexThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ivex_gemm(const IvexGemmArgs& a, hipStream_t s) {
  const int64_t cols_per_wg = (int64_t)kIvexColTile * (kIvexThreads / 64);
  const unsigned gx = (unsigned)((a.N + cols_per_wg - 1) / cols_per_wg);
  const unsigned gy = (unsigned)((a.K + a.k_chunk - 1) / a.k_chunk);
  hipLaunchKernelGGL(ivex_gemm_kernel, dim3(gx, gy), dim3(kIvexThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ivex_finish_terms(const IvexFinishArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ivex_finish_terms_kernel, dim3((unsigned)a.B), dim3(kIvexThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ivex_solve(const IvexSolveArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ivex_solve_kernel, dim3((unsigned)a.B), dim3(kIvexThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
