// Kernels of the GMM-UBM stage: see ubm_kernels.h for the launches and ubm.h for the semantics.
#include "ubm_kernels.h"

#include <math.h>

// add_deltas is compared with an fp32 restatement for equality: one rounding per operation (the Makefile passes
// -ffp-contract=off as well).  Where a fused multiply-add is wanted below it is written as fmaf.
#pragma clang fp contract(off)

namespace xv {
namespace {

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kUbmThreads) void add_deltas_kernel(const DeltaArgs a) {
  const int item = blockIdx.x;
  const int u = a.item_mat[item];
  const int r0 = a.item_blk[item] * kDeltaRowBlock;
  const int rows = a.row_off[u + 1] - a.row_off[u];
  const int nr = rows - r0 < kDeltaRowBlock ? rows - r0 : kDeltaRowBlock;
  const int dim = a.dim, oc = (a.order + 1) * dim;
  const float* src = a.feats + (int64_t)a.row_off[u] * a.in_stride;
  float* dst = a.out + ((int64_t)a.row_off[u] + r0) * oc;
  const int total = nr * oc;   // < 2^31: the launcher checks
  for (int e = threadIdx.x; e < total; e += kUbmThreads) {
    const int r = e / oc, c = e - r * oc;
    const int i = c / dim, d = c - i * dim;
    const int t = r0 + r, half = i * a.window;
    const float* sc = a.scales + a.scale_off[i] + half;
    float acc = 0.f;
    for (int j = -half; j <= half; ++j) {
      const float s = sc[j];
      if (s == 0.f) continue;
      int tt = t + j;
      tt = tt < 0 ? 0 : (tt > rows - 1 ? rows - 1 : tt);
      const float prod = s * src[(int64_t)tt * a.in_stride + d];
      acc = acc + prod;
    }
    dst[e] = acc;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// float -> unsigned key with the same order (and a place for every NaN), and back.  The key is that of x + 0: -0 + 0 is +0, so
// the two zeros are one score and their Gaussians go by index (ubm.h).
__device__ inline uint32_t score_key(float x) {
  const uint32_t b = __float_as_uint(x + 0.f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float key_score(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

constexpr int kDiagFramesPerThread = kUbmFrameBlock / (kUbmThreads / kUbmGaussTile);   // 16
constexpr int kDiagWaves = kUbmThreads / 64;
constexpr int kDiagFramesPerWave = kUbmFrameBlock / kDiagWaves;                         // 8
constexpr int kDiagCand = kUbmMaxSelect + kUbmGaussTile;
static_assert(kDiagFramesPerThread % 4 == 0 && kUbmGaussTile % 64 == 0 && kUbmFrameBlock % kDiagWaves == 0, "tile shapes");

__global__ __launch_bounds__(kUbmThreads) void ubm_diag_gselect_kernel(const UbmDiagArgs a) {
  extern __shared__ float4 dyn_lds[];
  float* aug = (float*)dyn_lds;   // [2 dim][kUbmFrameBlock]: x, then x * x
  __shared__ float sc[kUbmFrameBlock][kUbmGaussTile + 1];
  __shared__ uint32_t top_key[kUbmFrameBlock][kUbmMaxSelect];
  __shared__ int32_t top_idx[kUbmFrameBlock][kUbmMaxSelect];
  __shared__ uint32_t cand_key[kDiagWaves][kDiagCand];
  __shared__ int32_t cand_idx[kDiagWaves][kDiagCand];
  const int tid = threadIdx.x, dim = a.dim, n = a.n;
  const int64_t f0 = (int64_t)blockIdx.x * kUbmFrameBlock;
  for (int e = tid; e < kUbmFrameBlock * dim; e += kUbmThreads) {
    const int f = e / dim, d = e - f * dim;
    const float x = f0 + f < a.rows ? a.feats[(f0 + f) * dim + d] : 0.f;
    aug[d * kUbmFrameBlock + f] = x;
    aug[(dim + d) * kUbmFrameBlock + f] = x * x;
  }
  for (int e = tid; e < kUbmFrameBlock * kUbmMaxSelect; e += kUbmThreads) {
    (&top_key[0][0])[e] = 0u;
    (&top_idx[0][0])[e] = 0;
  }
  __syncthreads();
  const int gsub = tid % kUbmGaussTile, fh = tid / kUbmGaussTile;
  const int wave = tid >> 6, lane = tid & 63;
  int cnt = 0;   // entries of every frame's running list: the same for all frames
  for (int g0 = 0; g0 < a.gauss_pad; g0 += kUbmGaussTile) {
    {
      const int g = g0 + gsub;
      float acc[kDiagFramesPerThread];
      const float gc = a.gconst[g];
#pragma unroll
      for (int k = 0; k < kDiagFramesPerThread; ++k) acc[k] = gc;
      const float* mp = a.m_t + g;
      const float* vp = a.v_t + g;
      for (int d = 0; d < dim; ++d) {
        const float m = mp[(int64_t)d * a.gauss_pad], v = vp[(int64_t)d * a.gauss_pad];
        const float4* xp = (const float4*)(aug + d * kUbmFrameBlock + fh * kDiagFramesPerThread);
        const float4* qp = (const float4*)(aug + (dim + d) * kUbmFrameBlock + fh * kDiagFramesPerThread);
#pragma unroll
        for (int k = 0; k < kDiagFramesPerThread / 4; ++k) {
          const float4 x = xp[k], q = qp[k];
          acc[4 * k + 0] = fmaf(v, q.x, fmaf(m, x.x, acc[4 * k + 0]));
          acc[4 * k + 1] = fmaf(v, q.y, fmaf(m, x.y, acc[4 * k + 1]));
          acc[4 * k + 2] = fmaf(v, q.z, fmaf(m, x.z, acc[4 * k + 2]));
          acc[4 * k + 3] = fmaf(v, q.w, fmaf(m, x.w, acc[4 * k + 3]));
        }
      }
#pragma unroll
      for (int k = 0; k < kDiagFramesPerThread; ++k) sc[fh * kDiagFramesPerThread + k][gsub] = acc[k];
    }
    __syncthreads();
    // every wave merges its frames one after the other; the trip counts and the barriers are the same for all waves
    for (int fi = 0; fi < kDiagFramesPerWave; ++fi) {
      const int f = wave * kDiagFramesPerWave + fi;
      const bool open = cnt < n;
      const uint32_t thr = open ? 0u : top_key[f][n - 1];
      if (lane < cnt) {
        cand_key[wave][lane] = top_key[f][lane];
        cand_idx[wave][lane] = top_idx[f][lane];
      }
      int c = cnt;
#pragma unroll
      for (int h = 0; h < kUbmGaussTile / 64; ++h) {
        const int gs = h * 64 + lane, gg = g0 + gs;
        const uint32_t key = score_key(sc[f][gs]);
        // a tile's indices are above every index already in the list: at equal score the newcomer loses.  The compare only spares
        // the ranking below a candidate; admitted, an equal score would rank behind the list's by its index and fall out at n.
        const bool ok = gg < a.num_gauss && (open || key > thr);
        const unsigned long long mask = __ballot(ok);
        if (ok) {
          const int pos = c + __popcll(mask & ((1ull << lane) - 1ull));
          cand_key[wave][pos] = key;
          cand_idx[wave][pos] = gg;
        }
        c += __popcll(mask);
      }
      __syncthreads();
      for (int i = lane; i < c; i += 64) {
        const uint32_t k = cand_key[wave][i];
        const int32_t id = cand_idx[wave][i];
        int rank = 0;
        for (int j = 0; j < c; ++j) {
          const uint32_t kj = cand_key[wave][j];
          rank += (kj > k || (kj == k && cand_idx[wave][j] < id)) ? 1 : 0;
        }
        if (rank < n) {
          top_key[f][rank] = k;
          top_idx[f][rank] = id;
        }
      }
      __syncthreads();
    }
    const int valid = a.num_gauss - g0 < kUbmGaussTile ? a.num_gauss - g0 : kUbmGaussTile;
    cnt = cnt + valid < n ? cnt + valid : n;
  }
  for (int e = tid; e < kUbmFrameBlock * n; e += kUbmThreads) {
    const int f = e / n, s = e - f * n;
    if (f0 + f >= a.rows) continue;
    a.out_idx[(f0 + f) * n + s] = top_idx[f][s];
    if (a.out_ll) a.out_ll[(f0 + f) * n + s] = key_score(top_key[f][s]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// NC columns per thread: the LDS image of the inverse covariance is dim rows of W = 8 NC columns, zero beyond dim.
template <int NC>
__global__ __launch_bounds__(kUbmThreads) void ubm_full_loglike_kernel(const UbmFullArgs a) {
  constexpr int W = kUbmFullGroups * NC;
  constexpr int XS = W + 1;   // odd: the 32 frames of a read land in 32 banks
  extern __shared__ float4 dyn_lds[];
  float* A = (float*)dyn_lds;   // [dim][W]
  __shared__ float xs[kUbmFullFrameTile * XS];
  __shared__ float lin_s[W];
  __shared__ float red[kUbmFullGroups][kUbmFullFrameTile];
  const int g = blockIdx.x, tid = threadIdx.x, dim = a.dim;
  const int start = a.bucket_start[g], cnt = a.bucket_start[g + 1] - start;
  if ((int)blockIdx.y * kUbmFullFrameTile >= cnt) return;
  const float* packed = a.inv_covars + (int64_t)g * (dim * (dim + 1) / 2);
  for (int e = tid; e < dim * W; e += kUbmThreads) {
    const int i = e / W, j = e - i * W;
    const int lo = i > j ? i : j, hi = i > j ? j : i;
    A[e] = j < dim ? packed[lo * (lo + 1) / 2 + hi] : 0.f;
  }
  for (int j = tid; j < W; j += kUbmThreads) lin_s[j] = j < dim ? a.lin[(int64_t)g * dim + j] : 0.f;
  const float gc = a.gconst[g];
  const int f = tid % kUbmFullFrameTile, c = tid / kUbmFullFrameTile;
  for (int k0 = blockIdx.y * kUbmFullFrameTile; k0 < cnt; k0 += gridDim.y * kUbmFullFrameTile) {
    __syncthreads();   // the image (first pass); the previous pass's reads of xs and red
    for (int e = tid; e < kUbmFullFrameTile * W; e += kUbmThreads) {
      const int ff = e / W, j = e - ff * W;
      float x = 0.f;
      if (k0 + ff < cnt && j < dim) x = a.feats[(int64_t)(a.sorted[start + k0 + ff] / a.n) * dim + j];
      xs[ff * XS + j] = x;
    }
    __syncthreads();
    float acc[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) acc[k] = 0.f;
    const float* xr = xs + f * XS;
    for (int i = 0; i < dim; ++i) {
      const float xi = xr[i];
      const float4* ar = (const float4*)(A + i * W + c * NC);
#pragma unroll
      for (int k = 0; k < NC / 4; ++k) {
        const float4 v = ar[k];
        acc[4 * k + 0] = fmaf(xi, v.x, acc[4 * k + 0]);
        acc[4 * k + 1] = fmaf(xi, v.y, acc[4 * k + 1]);
        acc[4 * k + 2] = fmaf(xi, v.z, acc[4 * k + 2]);
        acc[4 * k + 3] = fmaf(xi, v.w, acc[4 * k + 3]);
      }
    }
    float q = 0.f, l = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const float xj = xr[c * NC + k];
      q = fmaf(xj, acc[k], q);
      l = fmaf(lin_s[c * NC + k], xj, l);
    }
    red[c][f] = fmaf(-0.5f, q, l);
    __syncthreads();
    if (c == 0 && k0 + f < cnt) {
      float tot = gc;
#pragma unroll
      for (int cc = 0; cc < kUbmFullGroups; ++cc) tot = tot + red[cc][f];
      a.ll[a.sorted[start + k0 + f]] = tot;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kUbmThreads) void ubm_post_kernel(const UbmFullArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kUbmThreads + threadIdx.x;
  if (t >= a.rows) return;
  const int n = a.n;
  const float* ll = a.ll + t * n;
  const int32_t* gs = a.gselect + t * n;
  float mx = ll[0];
  int arg = 0;
  for (int i = 1; i < n; ++i)
    if (ll[i] > mx) {
      mx = ll[i];
      arg = i;
    }
  float* post = a.out_post + t * n;
  int32_t* idx = a.out_idx + t * n;
  if (!isfinite(mx)) {   // no posterior (ubm.h): every score is -inf, or the first one is a NaN, as all are for a frame that holds one
    if (a.out_logsum) a.out_logsum[t] = mx;
    a.out_count[t] = 0;
    for (int i = 0; i < n; ++i) {
      idx[i] = -1;
      post[i] = 0.f;
      if (a.out_slot_post) a.out_slot_post[t * n + i] = 0.f;
    }
    return;
  }
  float sum = 0.f;
  for (int i = 0; i < n; ++i) sum = sum + expf(ll[i] - mx);
  if (a.out_logsum) a.out_logsum[t] = mx + logf(sum);
  const float inv = 1.f / sum;
  int count = 0;
  if (a.min_post != 0.f) {
    // what survives min-post is renormalised; nothing survives: the arg-max takes everything
    float kept = 0.f;
    for (int i = 0; i < n; ++i) {
      const float p = expf(ll[i] - mx) * inv;
      if (!(p < a.min_post)) kept = kept + p;
    }
    const float rescale = 1.f / kept;
    for (int i = 0; i < n; ++i) {
      float p = expf(ll[i] - mx) * inv;
      if (p < a.min_post) p = 0.f;
      p = kept == 0.f ? (i == arg ? 1.f : 0.f) : p * rescale;
      if (a.out_slot_post) a.out_slot_post[t * n + i] = p;
      if (p != 0.f) {
        idx[count] = gs[i];
        post[count] = p;
        ++count;
      }
    }
  } else {
    for (int i = 0; i < n; ++i) {
      const float p = expf(ll[i] - mx) * inv;
      if (a.out_slot_post) a.out_slot_post[t * n + i] = p;
      if (p != 0.f) {
        idx[count] = gs[i];
        post[count] = p;
        ++count;
      }
    }
  }
  a.out_count[t] = count;
  for (int i = count; i < n; ++i) {   // the slots that are not used hold no stale memory
    idx[i] = -1;
    post[i] = 0.f;
  }
}

template <int NC>
hipError_t launch_full(const UbmFullArgs& a, hipStream_t s) {
  const size_t lds = (size_t)a.dim * kUbmFullGroups * NC * sizeof(float);
  hipLaunchKernelGGL(ubm_full_loglike_kernel<NC>, dim3((unsigned)a.num_gauss, (unsigned)a.split), dim3(kUbmThreads), lds, s, a);
  return hipGetLastError();
}

bool full_args_ok(const UbmFullArgs& a) {
  return a.rows > 0 && a.dim >= 1 && a.dim <= kUbmMaxDim && a.num_gauss >= 1 && a.n >= 1 && a.n <= kUbmMaxSelect &&
         a.rows * a.n < INT32_MAX && a.gselect && a.bucket_start && a.sorted;
}

}  // namespace

hipError_t launch_add_deltas(const DeltaArgs& a, hipStream_t s) {
  if (a.n < 1 || a.n_items < 1 || a.dim < 1 || a.in_stride < a.dim || a.order < 0 || a.order > kDeltaMaxOrder || a.window < 0 || !a.feats ||
      !a.row_off || !a.scales || !a.item_mat || !a.item_blk || !a.out)
    return hipErrorInvalidValue;
  if ((int64_t)(a.order + 1) * a.dim > (INT32_MAX - kUbmThreads) / kDeltaRowBlock) return hipErrorInvalidValue;   // a block is indexed in 32 bits
  hipLaunchKernelGGL(add_deltas_kernel, dim3((unsigned)a.n_items), dim3(kUbmThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ubm_diag_gselect(const UbmDiagArgs& a, hipStream_t s) {
  if (a.rows < 1 || a.dim < 1 || a.dim > kUbmMaxDim || a.num_gauss < 1 || a.gauss_pad < a.num_gauss || a.gauss_pad % kUbmGaussTile != 0 ||
      a.n < 1 || a.n > kUbmMaxSelect || a.n > a.num_gauss || !a.feats || !a.m_t || !a.v_t || !a.gconst || !a.out_idx)
    return hipErrorInvalidValue;
  const int64_t blocks = (a.rows + kUbmFrameBlock - 1) / kUbmFrameBlock;
  if (blocks > INT32_MAX) return hipErrorInvalidValue;
  const size_t lds = (size_t)2 * a.dim * kUbmFrameBlock * sizeof(float);
  hipLaunchKernelGGL(ubm_diag_gselect_kernel, dim3((unsigned)blocks), dim3(kUbmThreads), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_ubm_full_loglike(const UbmFullArgs& a, hipStream_t s) {
  if (!full_args_ok(a) || !a.feats || !a.inv_covars || !a.lin || !a.gconst || !a.ll || a.split < 1 || a.split > 65535)
    return hipErrorInvalidValue;
  if (a.dim <= 32) return launch_full<4>(a, s);
  if (a.dim <= 64) return launch_full<8>(a, s);
  return launch_full<12>(a, s);
}

hipError_t launch_ubm_post(const UbmFullArgs& a, hipStream_t s) {
  if (!full_args_ok(a) || !a.ll || !a.out_count || !a.out_idx || !a.out_post) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ubm_post_kernel, dim3((unsigned)((a.rows + kUbmThreads - 1) / kUbmThreads)), dim3(kUbmThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
