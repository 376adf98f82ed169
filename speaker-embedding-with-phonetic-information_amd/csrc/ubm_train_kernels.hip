// Kernels of full-covariance UBM training: see ubm_train_kernels.h for the launches and ubm_train.h for the semantics.
#include "ubm_train_kernels.h"

namespace xv {
namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kAccWaves = kFgmmAccThreads / 64;
constexpr int kAccMaxTileRows = kFgmmAccMaxDim / 16;                                        // 6
constexpr int kAccTilesPerWave = (kAccMaxTileRows * (kAccMaxTileRows + 1) / 2 + kAccWaves - 1) / kAccWaves;   // 21 tiles: 6
constexpr int kAccMaxTiles = kAccMaxTileRows * (kAccMaxTileRows + 1) / 2;
// 16 over a multiple of 32 floats: the four k rows of a fragment read, 16 floats each, land in four disjoint groups of banks
constexpr int kAccXS = kFgmmAccMaxDim + 16;
// tile t of the lower triangle, row by row: (kTileRow[t], kTileCol[t]).  Wave t % 4 owns it, in accumulator t / 4.
constexpr int kTileRow[kAccMaxTiles] = {0, 1, 1, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 4, 5, 5, 5, 5, 5, 5};
constexpr int kTileCol[kAccMaxTiles] = {0, 0, 1, 0, 1, 2, 0, 1, 2, 3, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 5};
static_assert(kAccXS % 32 == 16 && kAccMaxTiles == 21, "the bank layout and the tile table");
static_assert(kFgmmAccMaxDim % 16 == 0 && kFgmmAccKTile % 4 == 0 && kFgmmAccKTile <= kFgmmAccThreads, "tile shapes");
static_assert(kFgmmAccMaxDim + 1 <= kFgmmAccThreads, "a thread per column of the mean, and one for the occupancy");

__device__ inline int tri(int n) { return n * (n + 1) / 2; }

// the work items: chunks per Gaussian, then their exclusive prefix sums
__global__ __launch_bounds__(kFgmmAccThreads) void fgmm_acc_items_kernel(const FgmmAccArgs a) {
  __shared__ int32_t part[kFgmmAccThreads];
  const int tid = threadIdx.x, G = a.num_gauss;
  const int per = (G + kFgmmAccThreads - 1) / kFgmmAccThreads;
  const int lo = tid * per < G ? tid * per : G, hi = lo + per < G ? lo + per : G;
  int32_t sum = 0;
  for (int g = lo; g < hi; ++g) sum += (a.bucket_start[g + 1] - a.bucket_start[g] + kFgmmAccPairChunk - 1) / kFgmmAccPairChunk;
  part[tid] = sum;
  __syncthreads();
  for (int step = 1; step < kFgmmAccThreads; step <<= 1) {
    const int32_t add = tid >= step ? part[tid - step] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  int32_t run = part[tid] - sum;
  for (int g = lo; g < hi; ++g) {
    a.item_start[g] = run;
    run += (a.bucket_start[g + 1] - a.bucket_start[g] + kFgmmAccPairChunk - 1) / kFgmmAccPairChunk;
  }
  if (tid == kFgmmAccThreads - 1) a.item_start[G] = part[tid];
}

__global__ __launch_bounds__(kFgmmAccThreads) void fgmm_acc_partial_kernel(const FgmmAccArgs a) {
  __shared__ float xs[kFgmmAccKTile * kAccXS];
  __shared__ float ws[kFgmmAccKTile];
  __shared__ int32_t fs[kFgmmAccKTile];
  const int item = blockIdx.x, tid = threadIdx.x;
  if (item >= a.item_start[a.num_gauss]) return;   // the grid is the host's upper bound; the whole workgroup leaves
  // the Gaussian g with item_start[g] <= item < item_start[g + 1]: the last one that starts at or before the item
  int g = 0;
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
  const int D = a.dim, T = (D + 15) >> 4, ntiles = tri(T);
  const bool do_mean = (a.flags & (kFgmmFlagMeans | kFgmmFlagVariances)) != 0, do_cov = (a.flags & kFgmmFlagVariances) != 0;
  const int lane = tid & 63, kq = lane >> 4, r16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // a scalar: what depends on it alone branches, it does not mask
  uint32_t mine = 0;   // bit t: tile t exists and is this wave's
  for (int t = wave; t < ntiles; t += kAccWaves) mine |= 1u << t;
  f64x4 acc[kAccTilesPerWave];
#pragma unroll
  for (int s = 0; s < kAccTilesPerWave; ++s) acc[s] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int vcol = kFgmmAccThreads - 1 - tid;   // the column of the mean this thread sums; D: the occupancy
  double vsum = 0.0;
  for (int k0 = begin; k0 < end; k0 += kFgmmAccKTile) {
    const int cnt = end - k0 < kFgmmAccKTile ? end - k0 : kFgmmAccKTile;
    __syncthreads();   // the previous tile's reads
    if (tid < kFgmmAccKTile) {
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
    if (do_mean) {
      for (int e = tid; e < cnt * D; e += kFgmmAccThreads) {
        const int r = e / D, d = e - r * D;
        xs[r * kAccXS + d] = ws[r] != 0.f ? a.feats[(int64_t)fs[r] * D + d] : 0.f;   // p = 0: the pair does not exist
      }
      __syncthreads();
    }
    if (do_cov) {
      for (int kk = 0; kk < cnt; kk += 4) {
        const int k = kk + kq;
        const bool k_in = k < cnt;
        const double w = k_in ? (double)ws[k] : 0.0;
        const float* row = xs + (k_in ? k : 0) * kAccXS;
        const int lim = k_in ? D : 0;   // one compare per fragment that changes with k: nothing to keep across the loop
        // the k step's fragments, one read per tile row: B is x, A is p x
        double xf[kAccMaxTileRows], wf[kAccMaxTileRows];
#pragma unroll
        for (int j = 0; j < kAccMaxTileRows; ++j) {
          const int c = j * 16 + r16;
          xf[j] = c < lim ? (double)row[c] : 0.0;   // columns beyond D (a tile row beyond T has no other) and k beyond the chunk
          wf[j] = w * xf[j];
        }
#pragma unroll
        for (int t = 0; t < kAccMaxTiles; ++t) {
          if ((mine >> t) & 1u)   // the same for the whole wave
            acc[t / kAccWaves] = __builtin_amdgcn_mfma_f64_16x16x4f64(wf[kTileRow[t]], xf[kTileCol[t]], acc[t / kAccWaves], 0, 0, 0);
        }
      }
    }
    if (vcol == D) {
      for (int r = 0; r < cnt; ++r) vsum += (double)ws[r];
    } else if (vcol < D && do_mean) {
      for (int r = 0; r < cnt; ++r) vsum += (double)ws[r] * (double)xs[r * kAccXS + vcol];
    }
  }
  double* P = a.partial + (int64_t)item * (1 + D + tri(D));
  if (vcol == D) P[0] = vsum;
  else if (vcol < D && do_mean) P[1 + vcol] = vsum;
  if (do_cov) {
#pragma unroll
    for (int t = 0; t < kAccMaxTiles; ++t) {
      if ((mine >> t) & 1u) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int row = kTileRow[t] * 16 + kq + 4 * reg, col = kTileCol[t] * 16 + r16;   // the f64 map: not (lane >> 4) * 4 + reg
          if (row < D && col <= row) P[1 + D + tri(row) + col] = acc[t / kAccWaves][reg];
        }
      }
    }
  }
}

__global__ __launch_bounds__(kFgmmAccThreads) void fgmm_acc_reduce_kernel(const FgmmAccArgs a) {
  const int g = blockIdx.x, D = a.dim;
  const int first = a.item_start[g], chunks = a.item_start[g + 1] - first;
  if (chunks == 0) return;
  const int stride = 1 + D + tri(D);
  const int used = (a.flags & kFgmmFlagVariances) ? stride : (a.flags & kFgmmFlagMeans) ? 1 + D : 1;
  const int e = blockIdx.y * kFgmmAccThreads + threadIdx.x;
  if (e >= used) return;
  const double* P = a.partial + (int64_t)first * stride + e;
  double sum = P[0];
  for (int c = 1; c < chunks; ++c) sum += P[(int64_t)c * stride];
  double* dst = e == 0 ? a.occ + g : e <= D ? a.mean + (int64_t)g * D + (e - 1) : a.cov + (int64_t)g * tri(D) + (e - 1 - D);
  *dst += sum;
}

bool acc_args_ok(const FgmmAccArgs& a) {
  return a.rows > 0 && a.dim >= 1 && a.dim <= kFgmmAccMaxDim && a.num_gauss >= 1 && a.pairs > 0 && a.pairs < INT32_MAX && a.sorted &&
         a.bucket_start && a.item_start && (a.pair_frame || (a.n >= 1 && a.pairs == a.rows * a.n));
}

}  // namespace

hipError_t launch_fgmm_acc_items(const FgmmAccArgs& a, hipStream_t s) {
  if (!acc_args_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fgmm_acc_items_kernel, dim3(1), dim3(kFgmmAccThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_fgmm_acc(const FgmmAccArgs& a, hipStream_t s) {
  const bool mean = (a.flags & (kFgmmFlagMeans | kFgmmFlagVariances)) != 0, cov = (a.flags & kFgmmFlagVariances) != 0;
  if (!acc_args_ok(a) || !a.pair_w || !a.partial || !a.occ || (mean && (!a.mean || !a.feats)) || (cov && !a.cov)) return hipErrorInvalidValue;
  // num_items is the host's bound: every bucket that is not empty has at most one chunk that is not full
  const int64_t bound = a.pairs / kFgmmAccPairChunk + (a.num_gauss < a.pairs ? a.num_gauss : a.pairs);
  if (a.num_items != bound) return hipErrorInvalidValue;
  const int stride = 1 + a.dim + a.dim * (a.dim + 1) / 2;
  hipLaunchKernelGGL(fgmm_acc_partial_kernel, dim3((unsigned)a.num_items), dim3(kFgmmAccThreads), 0, s, a);
  hipLaunchKernelGGL(fgmm_acc_reduce_kernel, dim3((unsigned)a.num_gauss, (unsigned)((stride + kFgmmAccThreads - 1) / kFgmmAccThreads)),
                     dim3(kFgmmAccThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
