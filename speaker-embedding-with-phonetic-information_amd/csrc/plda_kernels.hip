// PLDA back-end kernels (plda_kernels.h): scatter statistics for LDA / PLDA estimation, Kaldi's TransformIvector, and
// the per-trial log-likelihood ratio.  fp64 arithmetic with plain FMA, 256-thread workgroups (64 for the segment sums), fixed
// reduction orders.
#include "plda_kernels.h"

namespace xv {

namespace {

constexpr int kTile = 64;   // output tile of the rank-k products (64 x 64 doubles, 4 x 4 per thread)
constexpr int kKs = 16;     // rows per LDS stage

struct RankKArgs {
  const float* xf;          // fp32 rows (x[idx[r]]), or
  const double* xd;         // fp64 rows (xd[r])
  int ld;
  const int32_t* idx;       // xf rows: row r is xf[idx[r]]
  const int32_t* seg_off;   // xd rows: the B side of row r is divided by seg_off[r+1] - seg_off[r] (0 rows: skipped)
  int n_rows, dim;
  int rows_per_chunk, n_chunks;
  double* part;             // [n_chunks][dim][dim], tiles ti <= tj only
};

// Fixed chunking: a function of (rows, dim) only, so the reduction order never depends on the launch.
void Chunking(int n_rows, int dim, int* rows_per_chunk, int* n_chunks) {
  const int t = (dim + kTile - 1) / kTile;
  const int tiles = t * (t + 1) / 2;
  int c = (1024 + tiles - 1) / tiles;              // about 1024 workgroups of work
  if (c > 64) c = 64;
  const int by_rows = (n_rows + 63) / 64;          // at least 64 rows per chunk
  if (c > by_rows) c = by_rows;
  if (c < 1) c = 1;
  int rpc = (n_rows + c - 1) / c;
  rpc = (rpc + kKs - 1) / kKs * kKs;
  if (rpc < kKs) rpc = kKs;
  *rows_per_chunk = rpc;
  *n_chunks = n_rows > 0 ? (n_rows + rpc - 1) / rpc : 0;
}

// part[c] tile (ti, tj) = sum over rows r of chunk c of a_r[i] * b_r[j], one fma chain per output in row order.
__global__ __launch_bounds__(256) void rankk_kernel(const RankKArgs a) {
  const int t = (a.dim + kTile - 1) / kTile;
  const int ti = blockIdx.x / t, tj = blockIdx.x % t;
  if (ti > tj) return;
  const int c = blockIdx.y;
  const int r0 = c * a.rows_per_chunk;
  const int r1 = min(a.n_rows, r0 + a.rows_per_chunk);
  __shared__ double as[kKs][kTile + 1], bs[kKs][kTile + 1];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
  for (int rb = r0; rb < r1; rb += kKs) {
    // stage: row rb + ty, columns tx + 16 q of both tiles
    const int r = rb + ty;
    long src = -1;
    double w = 1.0;
    if (r < r1) {
      if (a.xf) {
        src = a.idx[r];
      } else {
        const int n = a.seg_off[r + 1] - a.seg_off[r];
        if (n > 0) {
          src = r;
          w = (double)n;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ca = ti * kTile + tx + 16 * q, cb = tj * kTile + tx + 16 * q;
      double va = 0.0, vb = 0.0;
      if (src >= 0) {
        if (a.xf) {
          if (ca < a.dim) va = (double)a.xf[src * a.ld + ca];
          if (cb < a.dim) vb = (double)a.xf[src * a.ld + cb];
        } else {
          if (ca < a.dim) va = a.xd[src * a.ld + ca];
          if (cb < a.dim) vb = a.xd[src * a.ld + cb] / w;
        }
      }
      as[ty][tx + 16 * q] = va;
      bs[ty][tx + 16 * q] = vb;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < kKs; ++k) {
      double av[4], bv[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) av[p] = as[k][tx + 16 * p];
#pragma unroll
      for (int q = 0; q < 4; ++q) bv[q] = bs[k][ty + 16 * q];
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = fma(av[p], bv[q], acc[p][q]);
    }
    __syncthreads();
  }
  double* dst = a.part + (size_t)c * a.dim * a.dim;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int i = ti * kTile + tx + 16 * p;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = tj * kTile + ty + 16 * q;
      if (i < a.dim && j < a.dim) dst[(size_t)i * a.dim + j] = acc[p][q];
    }
  }
}

// out[i][j] = out[j][i] = sum over chunks (in chunk order) of part[c][i][j], i <= j.
__global__ __launch_bounds__(256) void chunk_sum_kernel(const double* part, int n_chunks, int dim, double* out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)dim * dim) return;
  const int i = (int)(e / dim), j = (int)(e % dim);
  if (i > j) return;
  double s = 0.0;
  for (int c = 0; c < n_chunks; ++c) s += part[(size_t)c * dim * dim + e];
  out[e] = s;
  out[(size_t)j * dim + i] = s;
}

// sums[s] = rows of segment s added in list order (fp64).  One wave per (segment, 64 columns), a lane per column.  The
// rows are loaded kSumAhead at a time before any of them is added, so the loads overlap while every column keeps one
// add chain in list order (the same bits as one add per loaded row).  A segment of the whole table (ivector-adapt-plda)
// thus runs on dim / 64 waves with kSumAhead loads in flight each, instead of one load at a time.
constexpr int kSumAhead = 64;

__global__ __launch_bounds__(64) void segment_sum64_kernel(const ScatterArgs a) {
  const int s = blockIdx.x;
  const int k = blockIdx.y * 64 + threadIdx.x;
  if (k >= a.dim) return;
  const int b = a.seg_off[s], e = a.seg_off[s + 1];
  double acc = 0.0;
  int i = b;
  for (; i + kSumAhead <= e; i += kSumAhead) {
    float v[kSumAhead];
#pragma unroll
    for (int u = 0; u < kSumAhead; ++u) v[u] = a.x[(long)a.idx[i + u] * a.ldx + k];
#pragma unroll
    for (int u = 0; u < kSumAhead; ++u) acc += (double)v[u];
  }
  for (; i < e; ++i) acc += (double)a.x[(long)a.idx[i] * a.ldx + k];
  a.sums[(size_t)s * a.dim + k] = acc;
}

hipError_t rank_k(const RankKArgs& r, double* out, hipStream_t s) {
  if (r.n_chunks > 0) {
    const int t = (r.dim + kTile - 1) / kTile;
    hipLaunchKernelGGL(rankk_kernel, dim3(t * t, r.n_chunks), dim3(256), 0, s, r);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const size_t n = (size_t)r.dim * r.dim;
  hipLaunchKernelGGL(chunk_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const double*)r.part, r.n_chunks,
                     r.dim, out);
  return hipGetLastError();
}

}  // namespace

size_t scatter_stats_workspace(int dim, int n_idx, int n_seg) {
  int rpc, c1, c2;
  Chunking(n_idx, dim, &rpc, &c1);
  Chunking(n_seg, dim, &rpc, &c2);
  const int c = c1 > c2 ? c1 : c2;
  return (size_t)(c > 0 ? c : 1) * dim * dim;
}

hipError_t launch_scatter_stats(const ScatterArgs& a, hipStream_t s) {
  if (a.dim < 1 || a.n_seg < 0 || a.n_idx < 0) return hipErrorInvalidValue;
  if (a.n_seg > 0) {
    hipLaunchKernelGGL(segment_sum64_kernel, dim3(a.n_seg, (a.dim + 63) / 64), dim3(64), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  RankKArgs t = {};
  t.xf = a.x;
  t.ld = a.ldx;
  t.idx = a.idx;
  t.n_rows = a.n_idx;
  t.dim = a.dim;
  t.part = a.work;
  Chunking(t.n_rows, t.dim, &t.rows_per_chunk, &t.n_chunks);
  hipError_t e = rank_k(t, a.s_tot, s);
  if (e != hipSuccess) return e;
  RankKArgs b = {};
  b.xd = a.sums;
  b.ld = a.dim;
  b.seg_off = a.seg_off;
  b.n_rows = a.n_seg;
  b.dim = a.dim;
  b.part = a.work;   // stream order: the S_tot partials have been summed by now
  Chunking(b.n_rows, b.dim, &b.rows_per_chunk, &b.n_chunks);
  return rank_k(b, a.s_bet, s);
}

// ---------------------------------------------------------------------------------------------------------------------
// TransformIvector: 4 waves x 4 rows per workgroup; lane owns outputs d = lane + 64 j (j < J), T^T read coalesced
// (one pass over T per 4 rows), x from LDS.  Lane sums are reduced with a fixed xor-shuffle tree.
constexpr int kTrRows = 4;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

template <int J>
__global__ __launch_bounds__(256) void plda_transform_kernel(const PldaTransformArgs a) {
  __shared__ float xs[4 * kTrRows][kPldaMaxDim];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = blockIdx.x * 4 * kTrRows;
  for (int e = threadIdx.x; e < 4 * kTrRows * a.dim; e += 256) {
    const int r = e / a.dim, k = e % a.dim;
    xs[r][k] = row0 + r < a.n ? a.x[(long)(row0 + r) * a.dim + k] : 0.f;
  }
  __syncthreads();
  double acc[kTrRows][J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int d = lane + 64 * j;
    const double o = d < a.dim ? a.offset[d] : 0.0;
#pragma unroll
    for (int r = 0; r < kTrRows; ++r) acc[r][j] = o;
  }
  for (int k = 0; k < a.dim; ++k) {
    double tv[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int d = lane + 64 * j;
      tv[j] = d < a.dim ? a.tt[(long)k * a.dim + d] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < kTrRows; ++r) {
      const double xv = (double)xs[wave * kTrRows + r][k];
#pragma unroll
      for (int j = 0; j < J; ++j) acc[r][j] = fma(tv[j], xv, acc[r][j]);
    }
  }
#pragma unroll
  for (int r = 0; r < kTrRows; ++r) {
    const int row = row0 + wave * kTrRows + r;
    double ss = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int d = lane + 64 * j;
      if (d < a.dim) {
        const double y2 = acc[r][j] * acc[r][j];
        ss += a.simple ? y2 : y2 / (a.psi[d] + 1.0 / (row < a.n ? a.num[row] : 1.0));
      }
    }
    ss = wave_sum(ss);
    const double scale = a.simple ? sqrt((double)a.dim) / sqrt(ss) : sqrt((double)a.dim / ss);
    if (row < a.n) {
      if (lane == 0) a.scale[row] = scale;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int d = lane + 64 * j;
        if (d < a.dim) a.y[(long)row * a.dim + d] = (float)(a.normalize ? acc[r][j] * scale : acc[r][j]);
      }
    }
  }
}

// Per enrolment row: work = [m (n_u x dim) | 1/var (n_u x dim) | const (n_u)].
__global__ __launch_bounds__(256) void plda_enroll_kernel(const PldaScoreArgs a) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= a.n_u) return;
  const double n = a.num_u[k];
  double* m = a.work + (size_t)k * a.dim;
  double* iv = a.work + (size_t)a.n_u * a.dim + (size_t)k * a.dim;
  double lg = 0.0;
  for (int d = lane; d < a.dim; d += 64) {
    const double p = a.psi[d];
    m[d] = n * p / (n * p + 1.0) * (double)a.u[(long)k * a.dim + d];
    const double var = 1.0 + p / (n * p + 1.0);
    iv[d] = 1.0 / var;
    lg += log(1.0 + p) - log(var);
  }
  lg = wave_sum(lg);
  if (lane == 0) a.work[(size_t)2 * a.n_u * a.dim + k] = 0.5 * lg;
}

// One wave per trial.
__global__ __launch_bounds__(256) void plda_score_kernel(const PldaScoreArgs a) {
  const int lane = threadIdx.x & 63;
  const long tr = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tr >= a.n_trials) return;
  const int k = a.trials[2 * tr], t = a.trials[2 * tr + 1];
  const double* m = a.work + (size_t)k * a.dim;
  const double* iv = a.work + (size_t)a.n_u * a.dim + (size_t)k * a.dim;
  const float* v = a.v + (long)t * a.dim;
  double s1 = 0.0, s2 = 0.0;
  for (int d = lane; d < a.dim; d += 64) {
    const double x = (double)v[d];
    const double df = x - m[d];
    s1 = fma(df * df, iv[d], s1);
    s2 = fma(x * x, a.inv_psi1[d], s2);
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) a.scores[tr] = a.work[(size_t)2 * a.n_u * a.dim + k] - 0.5 * s1 + 0.5 * s2;
}

hipError_t launch_plda_transform(const PldaTransformArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (a.dim < 1 || a.dim > kPldaMaxDim) return hipErrorInvalidValue;
  const dim3 grid((a.n + 4 * kTrRows - 1) / (4 * kTrRows)), block(256);
  const int j = (a.dim + 63) / 64;
  if (j <= 1) hipLaunchKernelGGL(plda_transform_kernel<1>, grid, block, 0, s, a);
  else if (j <= 2) hipLaunchKernelGGL(plda_transform_kernel<2>, grid, block, 0, s, a);
  else if (j <= 3) hipLaunchKernelGGL(plda_transform_kernel<3>, grid, block, 0, s, a);
  else if (j <= 4) hipLaunchKernelGGL(plda_transform_kernel<4>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(plda_transform_kernel<8>, grid, block, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_plda_score(const PldaScoreArgs& a, hipStream_t s) {
  if (a.dim < 1 || a.dim > kPldaMaxDim || a.n_u < 0) return hipErrorInvalidValue;
  if (a.n_u > 0) {
    hipLaunchKernelGGL(plda_enroll_kernel, dim3((a.n_u + 3) / 4), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (a.n_trials <= 0) return hipSuccess;
  hipLaunchKernelGGL(plda_score_kernel, dim3((unsigned)((a.n_trials + 3) / 4)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
