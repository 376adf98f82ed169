// Kernels of diagonal UBM training: see dubm_train_kernels.h for the launches and dubm_train.h for the semantics.
#include "dubm_train_kernels.h"

#include <math.h>

// The scores are compared with ubm_diag_gselect's for equality: fl(x x) is a rounding of its own, and every fused multiply-add is
// written out as fmaf.
#pragma clang fp contract(off)

namespace xv {
namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

static_assert(2 * kDgmmMaxDim + 1 <= kDgmmThreads, "a thread per column of the sparse accumulator and of the reduction");
static_assert(kDgmmDenseFrameChunk % kDgmmDenseKTile == 0 && kDgmmDenseKTile % 4 == 0, "tile shapes");
static_assert(kDgmmGaussTile == 16 * (kDgmmThreads / 64) && kDgmmGaussTile == 64, "a wave per 16 Gaussians, a thread per Gaussian and quarter");
static_assert(kDgmmLogsumGaussTile == 128 && kDgmmThreads / kDgmmLogsumGaussTile == 2, "two waves per half of the frames");

// NF frames fbase .. fbase + NF of the staged block against one Gaussian: the chain of ubm_diag_gselect.  aug: [2 dim][STRIDE],
// x then fl(x x); mp / vp: the Gaussian's column of the transposed model.
template <int NF, int STRIDE>
__device__ inline void score_tile(const float* aug, int dim, const float* mp, const float* vp, int64_t pad, float gc, int fbase, float (&acc)[NF]) {
#pragma unroll
  for (int k = 0; k < NF; ++k) acc[k] = gc;
  for (int d = 0; d < dim; ++d) {
    const float m = mp[(int64_t)d * pad], v = vp[(int64_t)d * pad];
    const float4* xp = (const float4*)(aug + d * STRIDE + fbase);
    const float4* qp = (const float4*)(aug + (dim + d) * STRIDE + fbase);
#pragma unroll
    for (int k = 0; k < NF / 4; ++k) {
      const float4 x = xp[k], q = qp[k];
      acc[4 * k + 0] = fmaf(v, q.x, fmaf(m, x.x, acc[4 * k + 0]));
      acc[4 * k + 1] = fmaf(v, q.y, fmaf(m, x.y, acc[4 * k + 1]));
      acc[4 * k + 2] = fmaf(v, q.z, fmaf(m, x.z, acc[4 * k + 2]));
      acc[4 * k + 3] = fmaf(v, q.w, fmaf(m, x.w, acc[4 * k + 3]));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDgmmThreads) void dgmm_sel_loglike_kernel(const DgmmSelArgs a) {
  const int64_t p = (int64_t)blockIdx.x * kDgmmThreads + threadIdx.x;
  if (p >= a.rows * a.n) return;
  const int dim = a.model.dim;
  const int64_t pad = a.model.gauss_pad;
  const int32_t g = a.gselect[p];
  const float* x = a.feats + (p / a.n) * dim;
  const float* mp = a.model.m_t + g;
  const float* vp = a.model.v_t + g;
  float acc = a.model.gconst[g];
  for (int d = 0; d < dim; ++d) {
    const float xd = x[d];
    const float q = xd * xd;
    acc = fmaf(vp[(int64_t)d * pad], q, fmaf(mp[(int64_t)d * pad], xd, acc));
  }
  a.ll[p] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDgmmThreads) void dgmm_acc_partial_kernel(const FgmmAccArgs a) {
  __shared__ float xs[kDgmmKTile * kDgmmMaxDim];
  __shared__ float ws[kDgmmKTile];
  __shared__ int32_t fs[kDgmmKTile];
  const int item = blockIdx.x, tid = threadIdx.x;
  if (item >= a.item_start[a.num_gauss]) return;   // the grid is the host's upper bound; the whole workgroup leaves
  int g = 0;   // the last Gaussian whose items start at or before this one
  {
    int hi = a.num_gauss;
    while (hi - g > 1) {
      const int mid = (g + hi) >> 1;
      if (a.item_start[mid] <= item) g = mid;
      else hi = mid;
    }
  }
  const int bucket_end = a.bucket_start[g + 1];
  const int begin = a.bucket_start[g] + (item - a.item_start[g]) * kFgmmAccPairChunk;   // inside the bucket: no overflow
  const int end = bucket_end - begin < kFgmmAccPairChunk ? bucket_end : begin + kFgmmAccPairChunk;
  const int D = a.dim;
  const int xc = tid < D ? tid : tid - D;   // the column of the frames this thread reads, when tid < 2 D
  double sum = 0.0;
  for (int k0 = begin; k0 < end; k0 += kDgmmKTile) {
    const int cnt = end - k0 < kDgmmKTile ? end - k0 : kDgmmKTile;
    __syncthreads();   // the previous tile's reads
    if (tid < kDgmmKTile) {
      float w = 0.f;
      int32_t f = 0;
      if (tid < cnt) {
        const int32_t p = a.sorted[k0 + tid];
        w = a.pair_w[p];
        f = a.pair_frame ? a.pair_frame[p] : p / a.n;
      }
      ws[tid] = w;
      fs[tid] = f;
    }
    __syncthreads();
    for (int e = tid; e < cnt * D; e += kDgmmThreads) {
      const int r = e / D, d = e - r * D;
      xs[e] = ws[r] != 0.f ? a.feats[(int64_t)fs[r] * D + d] : 0.f;   // p = 0: the pair does not exist
    }
    __syncthreads();
    if (tid < D) {
      for (int r = 0; r < cnt; ++r) sum += (double)ws[r] * (double)xs[r * D + xc];
    } else if (tid < 2 * D) {
      for (int r = 0; r < cnt; ++r) {
        const double x = (double)xs[r * D + xc];
        sum += (double)ws[r] * (x * x);
      }
    } else if (tid == 2 * D) {
      for (int r = 0; r < cnt; ++r) sum += (double)ws[r];
    }
  }
  double* P = a.partial + (int64_t)item * (1 + 2 * D);
  if (tid < 2 * D) P[1 + tid] = sum;
  else if (tid == 2 * D) P[0] = sum;
}

__global__ __launch_bounds__(kDgmmThreads) void dgmm_acc_reduce_kernel(const DgmmReduceArgs a) {
  const int g = blockIdx.x, D = a.dim, e = threadIdx.x;
  int64_t first;
  int chunks;
  if (a.item_start) {
    first = a.item_start[g];
    chunks = a.item_start[g + 1] - a.item_start[g];
  } else {
    first = (int64_t)g * a.num_chunks;
    chunks = a.num_chunks;
  }
  if (chunks == 0) return;
  const int stride = 1 + 2 * D;
  const int used = (a.flags & kFgmmFlagVariances) ? stride : (a.flags & kFgmmFlagMeans) ? 1 + D : 1;
  if (e >= used) return;
  const double* P = a.partial + first * stride + e;
  double sum = P[0];
  for (int c = 1; c < chunks; ++c) sum += P[(int64_t)c * stride];
  double* dst = e == 0 ? a.occ + g : e <= D ? a.mean + (int64_t)g * D + (e - 1) : a.var + (int64_t)g * D + (e - 1 - D);
  *dst += sum;
}

// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kLsFramesPerThread = kDgmmLogsumFrames / (kDgmmThreads / kDgmmLogsumGaussTile);   // 16
constexpr int kLsWaves = kDgmmThreads / 64;

__global__ __launch_bounds__(kDgmmThreads) void dgmm_dense_logsum_kernel(const DgmmDenseArgs a) {
  __shared__ __attribute__((aligned(16))) float aug[2 * kDgmmMaxDim * kDgmmLogsumFrames];   // [2 dim][frames]: x, then fl(x x)
  __shared__ float wmax[kLsWaves][kLsFramesPerThread];
  __shared__ double wsum[kLsWaves][kLsFramesPerThread];
  const int tid = threadIdx.x, dim = a.model.dim, G = a.model.num_gauss;
  const int64_t pad = a.model.gauss_pad;
  const int64_t f0 = (int64_t)blockIdx.x * kDgmmLogsumFrames;
  for (int e = tid; e < kDgmmLogsumFrames * dim; e += kDgmmThreads) {
    const int f = e / dim, d = e - f * dim;
    const float x = f0 + f < a.rows ? a.feats[(f0 + f) * dim + d] : 0.f;
    aug[d * kDgmmLogsumFrames + f] = x;
    aug[(dim + d) * kDgmmLogsumFrames + f] = x * x;
  }
  __syncthreads();
  const int gsub = tid % kDgmmLogsumGaussTile, fh = tid / kDgmmLogsumGaussTile;
  const int wave = tid >> 6, lane = tid & 63;
  float acc[kLsFramesPerThread], mx[kLsFramesPerThread];
#pragma unroll
  for (int k = 0; k < kLsFramesPerThread; ++k) mx[k] = -INFINITY;
  for (int g0 = 0; g0 < pad; g0 += kDgmmLogsumGaussTile) {
    const int g = g0 + gsub;
    score_tile<kLsFramesPerThread, kDgmmLogsumFrames>(aug, dim, a.model.m_t + g, a.model.v_t + g, pad, a.model.gconst[g], fh * kLsFramesPerThread, acc);
    if (g < G) {
#pragma unroll
      for (int k = 0; k < kLsFramesPerThread; ++k) mx[k] = fmaxf(mx[k], acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < kLsFramesPerThread; ++k) {
    for (int off = 32; off >= 1; off >>= 1) mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off));
    if (lane == 0) wmax[wave][k] = mx[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kLsFramesPerThread; ++k) mx[k] = fmaxf(wmax[2 * fh][k], wmax[2 * fh + 1][k]);   // the frame's exact maximum
  double sum[kLsFramesPerThread];
#pragma unroll
  for (int k = 0; k < kLsFramesPerThread; ++k) sum[k] = 0.0;
  for (int g0 = 0; g0 < pad; g0 += kDgmmLogsumGaussTile) {   // the scores again: the same bits
    const int g = g0 + gsub;
    score_tile<kLsFramesPerThread, kDgmmLogsumFrames>(aug, dim, a.model.m_t + g, a.model.v_t + g, pad, a.model.gconst[g], fh * kLsFramesPerThread, acc);
    const bool in = g < G;
#pragma unroll
    for (int k = 0; k < kLsFramesPerThread; ++k) sum[k] += in ? (double)expf(acc[k] - mx[k]) : 0.0;
  }
  // a butterfly over the wave's lanes, then the two waves of the half: a fixed order for a given number of Gaussians
#pragma unroll
  for (int k = 0; k < kLsFramesPerThread; ++k) {
    for (int off = 32; off >= 1; off >>= 1) sum[k] += __shfl_xor(sum[k], off);
    if (lane == 0) wsum[wave][k] = sum[k];
  }
  __syncthreads();
  if (gsub == 0) {
#pragma unroll
    for (int k = 0; k < kLsFramesPerThread; ++k) {
      const int64_t t = f0 + fh * kLsFramesPerThread + k;
      if (t < a.rows) a.logsum[t] = (float)((double)mx[k] + log(wsum[2 * fh][k] + wsum[2 * fh + 1][k]));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kDaKS = kDgmmDenseKTile + 4;   // the staged frames' stride: a multiple of 4 (float4 reads of the scores) that spreads
                                             // the 16 columns of a B fragment over the banks (column * 36 + k)
constexpr int kDaPS = 80;                    // the stride of p [k][Gaussian]: the 4 k rows of an A fragment land 16 banks apart
constexpr int kDaFramesPerThread = kDgmmDenseKTile / (kDgmmThreads / kDgmmGaussTile);   // 8
static_assert(kDaKS % 4 == 0 && kDaPS >= kDgmmGaussTile && kDaFramesPerThread % 4 == 0, "the strides");

template <int NT>
__global__ __launch_bounds__(kDgmmThreads) void dgmm_dense_acc_kernel(const DgmmDenseArgs a) {
  // [2 dim + 2][kDaKS]: x, then fl(x x), then a row of ones and a row of zeros.  A B operand is the product of two widened
  // entries (x 1, x x, 1 1 or 0 0: all exact), so that what a column is costs two offsets per lane and no mask in the K loop.
  __shared__ __attribute__((aligned(16))) float aug[(2 * kDgmmMaxDim + 2) * kDaKS];
  __shared__ float ps[kDgmmDenseKTile * kDaPS];                                 // [k][Gaussian of the tile]
  __shared__ float ls[kDgmmDenseKTile];
  const int tid = threadIdx.x, D = a.model.dim, G = a.model.num_gauss;
  const int64_t pad = a.model.gauss_pad;
  const int g0 = blockIdx.x * kDgmmGaussTile, chunk = blockIdx.y;
  const int64_t fbeg = (int64_t)chunk * kDgmmDenseFrameChunk;
  const int64_t fend = a.rows - fbeg < kDgmmDenseFrameChunk ? a.rows : fbeg + kDgmmDenseFrameChunk;
  const int ncols = 2 * D + 1, nt = (ncols + 15) >> 4;   // nt <= NT: the launcher chooses NT
  const int lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gsub = tid & (kDgmmGaussTile - 1), fq = tid / kDgmmGaussTile;
  const int g = g0 + gsub;   // < gauss_pad: the model's arrays are padded to a multiple of 128
  f64x4 acc[NT];
  int off_a[NT], off_b[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int col = j * 16 + r16, ones = 2 * D * kDaKS, zeros = (2 * D + 1) * kDaKS;
    off_a[j] = (col < D ? col * kDaKS : col < 2 * D ? (col - D) * kDaKS : col == 2 * D ? ones : zeros) + kq;   // columns beyond 2 D + 1 are zero
    off_b[j] = (col < D ? ones : col < 2 * D ? (col - D) * kDaKS : col == 2 * D ? ones : zeros) + kq;
  }
  if (tid < kDaKS) {
    aug[2 * D * kDaKS + tid] = 1.f;
    aug[(2 * D + 1) * kDaKS + tid] = 0.f;
  }
  for (int64_t k0 = fbeg; k0 < fend; k0 += kDgmmDenseKTile) {
    const int cnt = fend - k0 < kDgmmDenseKTile ? (int)(fend - k0) : kDgmmDenseKTile;
    __syncthreads();   // the previous tile's reads
    for (int e = tid; e < kDgmmDenseKTile * D; e += kDgmmThreads) {
      const int f = e / D, d = e - f * D;
      const float x = f < cnt ? a.feats[(k0 + f) * D + d] : 0.f;
      aug[d * kDaKS + f] = x;
      aug[(D + d) * kDaKS + f] = x * x;
    }
    if (tid < kDgmmDenseKTile) ls[tid] = (!a.post && tid < cnt) ? a.logsum[k0 + tid] : 0.f;
    __syncthreads();
    if (a.post) {
#pragma unroll
      for (int k = 0; k < kDaFramesPerThread; ++k) {
        const int f = fq * kDaFramesPerThread + k;
        ps[f * kDaPS + gsub] = (g < G && f < cnt) ? a.post[(k0 + f) * G + g] : 0.f;
      }
    } else {
      float s[kDaFramesPerThread];
      score_tile<kDaFramesPerThread, kDaKS>(aug, D, a.model.m_t + g, a.model.v_t + g, pad, a.model.gconst[g], fq * kDaFramesPerThread, s);
#pragma unroll
      for (int k = 0; k < kDaFramesPerThread; ++k) {
        const int f = fq * kDaFramesPerThread + k;
        ps[f * kDaPS + gsub] = (g < G && f < cnt) ? expf(s[k] - ls[f]) : 0.f;   // rows beyond G and frames beyond the chunk
      }
    }
    __syncthreads();
    for (int kk = 0; kk < cnt; kk += 4) {
      const int k = kk + kq;   // < kDgmmDenseKTile; beyond cnt p is 0 and x is 0
      const double av = (double)ps[k * kDaPS + wave * 16 + r16];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        if (j < nt) {   // the same for the whole workgroup
          const double b = (double)aug[off_a[j] + kk] * (double)aug[off_b[j] + kk];
          acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b, acc[j], 0, 0, 0);
        }
      }
    }
  }
  const int stride = 1 + 2 * D;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    if (j < nt) {
      const int col = j * 16 + r16;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int gg = g0 + wave * 16 + kq + 4 * reg;   // the f64 map: not (lane >> 4) * 4 + reg
        if (gg < G && col < ncols) a.partial[((int64_t)gg * a.num_chunks + chunk) * stride + (col == 2 * D ? 0 : 1 + col)] = acc[j][reg];
      }
    }
  }
}

template <int NT>
hipError_t launch_dense(const DgmmDenseArgs& a, hipStream_t s) {
  const unsigned tiles = (unsigned)((a.model.num_gauss + kDgmmGaussTile - 1) / kDgmmGaussTile);
  hipLaunchKernelGGL(dgmm_dense_acc_kernel<NT>, dim3(tiles, (unsigned)a.num_chunks), dim3(kDgmmThreads), 0, s, a);
  return hipGetLastError();
}

bool model_ok(const DgmmModelArgs& m) {
  return m.dim >= 1 && m.dim <= kDgmmMaxDim && m.num_gauss >= 1 && m.gauss_pad >= m.num_gauss && m.gauss_pad % kDgmmLogsumGaussTile == 0 && m.m_t &&
         m.v_t && m.gconst;
}

}  // namespace

hipError_t launch_dgmm_sel_loglike(const DgmmSelArgs& a, hipStream_t s) {
  if (!model_ok(a.model) || a.rows < 1 || a.n < 1 || a.rows * a.n >= INT32_MAX || !a.feats || !a.gselect || !a.ll) return hipErrorInvalidValue;
  const int64_t pairs = a.rows * a.n;
  hipLaunchKernelGGL(dgmm_sel_loglike_kernel, dim3((unsigned)((pairs + kDgmmThreads - 1) / kDgmmThreads)), dim3(kDgmmThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_dgmm_acc(const FgmmAccArgs& a, hipStream_t s) {
  if (a.rows < 1 || a.dim < 1 || a.dim > kDgmmMaxDim || a.num_gauss < 1 || a.pairs < 1 || a.pairs >= INT32_MAX || !a.sorted || !a.bucket_start ||
      !a.item_start || !(a.pair_frame || (a.n >= 1 && a.pairs == a.rows * a.n)) || !a.pair_w || !a.partial || !a.feats || !a.occ || !a.mean || !a.cov)
    return hipErrorInvalidValue;
  const int64_t bound = a.pairs / kFgmmAccPairChunk + (a.num_gauss < a.pairs ? a.num_gauss : a.pairs);
  if (a.num_items != bound) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dgmm_acc_partial_kernel, dim3((unsigned)a.num_items), dim3(kDgmmThreads), 0, s, a);
  DgmmReduceArgs r;
  r.dim = a.dim;
  r.num_gauss = a.num_gauss;
  r.flags = a.flags;
  r.item_start = a.item_start;
  r.num_chunks = 0;
  r.partial = a.partial;
  r.occ = a.occ;
  r.mean = a.mean;
  r.var = a.cov;
  return launch_dgmm_acc_reduce(r, s);
}

hipError_t launch_dgmm_dense_logsum(const DgmmDenseArgs& a, hipStream_t s) {
  if (!model_ok(a.model) || a.rows < 1 || !a.feats || !a.logsum) return hipErrorInvalidValue;
  const int64_t blocks = (a.rows + kDgmmLogsumFrames - 1) / kDgmmLogsumFrames;
  if (blocks > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dgmm_dense_logsum_kernel, dim3((unsigned)blocks), dim3(kDgmmThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_dgmm_dense_acc(const DgmmDenseArgs& a, hipStream_t s) {
  const bool shape_ok = a.model.dim >= 1 && a.model.dim <= kDgmmMaxDim && a.model.num_gauss >= 1;
  if (!shape_ok || (!a.post && (!model_ok(a.model) || !a.logsum)) || a.rows < 1 || !a.feats || !a.partial) return hipErrorInvalidValue;
  if (a.num_chunks != (int)((a.rows + kDgmmDenseFrameChunk - 1) / kDgmmDenseFrameChunk) || a.num_chunks > 65535) return hipErrorInvalidValue;
  const int nt = (2 * a.model.dim + 1 + 15) / 16;
  if (nt <= 4) return launch_dense<4>(a, s);
  if (nt <= 8) return launch_dense<8>(a, s);
  return launch_dense<13>(a, s);
}

hipError_t launch_dgmm_acc_reduce(const DgmmReduceArgs& a, hipStream_t s) {
  if (a.dim < 1 || a.dim > kDgmmMaxDim || a.num_gauss < 1 || (!a.item_start && a.num_chunks < 1) || !a.partial || !a.occ || !a.mean || !a.var)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(dgmm_acc_reduce_kernel, dim3((unsigned)a.num_gauss), dim3(kDgmmThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
