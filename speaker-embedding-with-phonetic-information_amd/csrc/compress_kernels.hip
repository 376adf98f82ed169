// Kernels of the feature compressor: see compress_kernels.h for the launches and compress.h for the format.
#include "compress_kernels.h"

// One rounding per operation everywhere below: a * b + c must not become a fused multiply-add (the Makefile passes
// -ffp-contract=off as well; the pragma keeps any other compile line honest).  Division is hipcc's correctly rounded one.
#pragma clang fp contract(off)

namespace xv {
namespace {

enum { kFmtCM = 0, kFmtCM2 = 1, kFmtCM3 = 2 };

__device__ __forceinline__ int cmp_format(int method, int rows) {
  if (method == 2 || (method == 1 && rows > 8)) return kFmtCM;
  return method == 5 ? kFmtCM3 : kFmtCM2;
}

// float bits <-> an unsigned integer that orders like the float (-0 below +0, NaNs at the two ends)
__device__ __forceinline__ uint32_t cmp_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ float cmp_unkey(uint32_t key) {
  return __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu));
}

// the global header's two floats from the statistics: a zero minimum is +0; max == min widens the range to 1 + |min|
__device__ __forceinline__ void cmp_min_range(const CmpStats& st, float* mn, float* range) {
  float lo = cmp_unkey(st.min_key), hi = cmp_unkey(st.max_key);
  if (lo == 0.f) lo = 0.f;
  if (hi == lo) hi = lo + (1.0f + fabsf(lo));
  *mn = lo;
  *range = hi - lo;
}

// int((x - min) / range * top + 0.499) with the fraction clamped to [0, 1]
__device__ __forceinline__ int cmp_code(float x, float mn, float range, float top) {
  float f = (x - mn) / range;
  f = fminf(fmaxf(f, 0.0f), 1.0f);
  return (int)(f * top + 0.499f);
}

// base + clamp(int((v - lo) / (hi - lo) * scale + 0.5), 0, scale), clamped before the conversion
__device__ __forceinline__ int cmp_segment(float v, float lo, float hi, float scale, int base) {
  float t = (v - lo) / (hi - lo) * scale + 0.5f;
  t = fminf(fmaxf(t, 0.0f), scale);
  return base + (int)t;
}

__global__ __launch_bounds__(kCmpMinmaxThreads) void cmp_minmax_kernel(const CmpArgs a) {
  const int u = a.item_mat[blockIdx.x];
  const int64_t total = (int64_t)(a.row_off[u + 1] - a.row_off[u]) * a.cols;
  const int64_t e0 = (int64_t)a.item_blk[blockIdx.x] * kCmpMinmaxChunk;
  const int64_t e1 = e0 + kCmpMinmaxChunk < total ? e0 + kCmpMinmaxChunk : total;
  const uint32_t* src = (const uint32_t*)a.feats + (int64_t)a.row_off[u] * a.cols;
  __shared__ uint32_t s_min, s_max, s_bad;
  if (threadIdx.x == 0) {
    s_min = 0xffffffffu;
    s_max = 0u;
    s_bad = 0u;
  }
  __syncthreads();
  uint32_t lo = 0xffffffffu, hi = 0u, bad = 0u;
  for (int64_t i = e0 + threadIdx.x; i < e1; i += kCmpMinmaxThreads) {
    const uint32_t bits = src[i];
    const uint32_t k = cmp_key(bits);
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
    bad |= (bits & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
  }
  // across the wave first: one LDS atomic per wave and value
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t l2 = __shfl_xor(lo, d), h2 = __shfl_xor(hi, d), b2 = __shfl_xor(bad, d);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
    bad |= b2;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&s_min, lo);
    atomicMax(&s_max, hi);
    if (bad) atomicOr(&s_bad, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0 && e0 < e1) {
    atomicMin(&a.stats[u].min_key, s_min);
    atomicMax(&a.stats[u].max_key, s_max);
    if (s_bad) atomicOr(&a.stats[u].nonfinite, 1u);
  }
}

// One workgroup per (matrix, group of kCmpSelectCols columns).  A thread keeps one column: the rows of the group are read
// 1024 / gc at a time, consecutive lanes on consecutive columns.  Both ranks are narrowed in the same pass: rank t keeps the
// leading bits found so far (prefix[t][c]) and what is left of its rank among the keys that share them (rank[t][c]).
__global__ __launch_bounds__(kCmpSelectThreads) void cmp_select_kernel(const CmpArgs a) {
  constexpr int CG = kCmpSelectCols, HS = 257;   // 257: the bin scans of different columns start in different banks
  const int u = a.item_mat[blockIdx.x];
  const int c0 = a.item_blk[blockIdx.x] * CG;
  const int rows = a.row_off[u + 1] - a.row_off[u];
  const int gc = a.cols - c0 < CG ? a.cols - c0 : CG;
  const int tid = threadIdx.x;
  __shared__ uint32_t hist[2 * CG * HS];
  __shared__ uint32_t prefix[2][CG], rank[2][CG], cmin[CG], cmax[CG];
  if (tid < gc) {
    const int q = rows / 4;
    rank[0][tid] = rows >= 5 ? q : (rows - 1 < 1 ? rows - 1 : 1);
    rank[1][tid] = rows >= 5 ? 3 * q : (rows - 1 < 2 ? rows - 1 : 2);
    prefix[0][tid] = prefix[1][tid] = 0u;
    cmin[tid] = 0xffffffffu;
    cmax[tid] = 0u;
  }
  const int rpi = kCmpSelectThreads / gc;   // rows per iteration
  const bool active = tid < rpi * gc;
  const int c = tid % gc, rr = tid / gc;
  const uint32_t* src = (const uint32_t*)a.feats + (int64_t)a.row_off[u] * a.cols + c0 + c;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < 2 * CG * HS; i += kCmpSelectThreads) hist[i] = 0u;
    __syncthreads();
    if (active) {
      uint32_t* h0 = hist + c * HS;
      uint32_t* h1 = hist + (CG + c) * HS;
      if (pass == 0) {
        uint32_t lo = 0xffffffffu, hi = 0u;
        for (int r = rr; r < rows; r += rpi) {
          const uint32_t k = cmp_key(src[(int64_t)r * a.cols]);
          lo = k < lo ? k : lo;
          hi = k > hi ? k : hi;
          atomicAdd(&h0[k >> 24], 1u);
          atomicAdd(&h1[k >> 24], 1u);
        }
        if (rr < rows) {
          atomicMin(&cmin[c], lo);
          atomicMax(&cmax[c], hi);
        }
      } else {
        const uint32_t p0 = prefix[0][c], p1 = prefix[1][c];
        for (int r = rr; r < rows; r += rpi) {
          const uint32_t k = cmp_key(src[(int64_t)r * a.cols]);
          const uint32_t bin = (k >> shift) & 255u;
          if (((k ^ p0) >> (shift + 8)) == 0u) atomicAdd(&h0[bin], 1u);
          if (((k ^ p1) >> (shift + 8)) == 0u) atomicAdd(&h1[bin], 1u);
        }
      }
    }
    __syncthreads();
    if (tid < 2 * gc) {
      const int t = tid / gc, cc = tid - t * gc;
      const uint32_t* h = hist + (t * CG + cc) * HS;
      const uint32_t want = rank[t][cc];
      uint32_t before = 0u;
      int b = 0;
      for (; b < 255; ++b) {   // the counts of the matching keys add up to more than the rank: bin 255 is what is left
        const uint32_t n = h[b];
        if (before + n > want) break;
        before += n;
      }
      prefix[t][cc] |= (uint32_t)b << shift;
      rank[t][cc] = want - before;
    }
    __syncthreads();
  }
  if (tid < gc) {
    float mn, range;
    cmp_min_range(a.stats[u], &mn, &range);
    const int u0 = cmp_code(cmp_unkey(cmin[tid]), mn, range, 65535.0f);
    const int u1 = cmp_code(cmp_unkey(prefix[0][tid]), mn, range, 65535.0f);
    const int u2 = cmp_code(cmp_unkey(prefix[1][tid]), mn, range, 65535.0f);
    const int u3 = cmp_code(cmp_unkey(cmax[tid]), mn, range, 65535.0f);
    // strictly increasing; a column shorter than four rows has no s[1], s[2] or s[3]: the value before, plus one
    const int p0 = min(u0, 65532);
    const int p25 = rows > 1 ? min(max(u1, p0 + 1), 65533) : p0 + 1;
    const int p75 = rows > 2 ? min(max(u2, p25 + 1), 65534) : p25 + 1;
    const int p100 = rows > 3 ? max(u3, p75 + 1) : p75 + 1;
    uint32_t* dst = (uint32_t*)(a.out + a.obj_off[u] + 16 + (int64_t)(c0 + tid) * 8);
    dst[0] = (uint32_t)p0 | ((uint32_t)p25 << 16);
    dst[1] = (uint32_t)p75 | ((uint32_t)p100 << 16);
  }
}

// One workgroup per (matrix, kCmpEncodeRows rows).
__global__ __launch_bounds__(kCmpEncodeThreads) void cmp_encode_kernel(const CmpArgs a) {
  constexpr int RB = kCmpEncodeRows, CT = kCmpEncodeCols, TS = RB + 4;   // TS: a column of the tile starts one bank further
  const int u = a.item_mat[blockIdx.x];
  const int r0 = a.item_blk[blockIdx.x] * RB;
  const int rows = a.row_off[u + 1] - a.row_off[u];
  const int cols = a.cols;
  const int nr = rows - r0 < RB ? rows - r0 : RB;
  const int tid = threadIdx.x;
  float mn, range;
  cmp_min_range(a.stats[u], &mn, &range);
  uint8_t* obj = a.out + a.obj_off[u];
  if (r0 == 0 && tid == 0) {
    uint32_t* h = (uint32_t*)obj;
    h[0] = __float_as_uint(mn);
    h[1] = __float_as_uint(range);
    h[2] = (uint32_t)rows;
    h[3] = (uint32_t)cols;
  }
  const float* src = a.feats + ((int64_t)a.row_off[u] + r0) * cols;
  const int fmt = cmp_format(a.method, rows);
  if (fmt != kFmtCM) {
    const int total = nr * cols;   // at most 128 rows
    const int64_t first = (int64_t)r0 * cols;
    if (fmt == kFmtCM2) {
      uint16_t* dst = (uint16_t*)(obj + 16) + first;
      for (int i = tid; i < total; i += kCmpEncodeThreads) dst[i] = (uint16_t)cmp_code(src[i], mn, range, 65535.0f);
    } else {
      uint8_t* dst = obj + 16 + first;
      for (int i = tid; i < total; i += kCmpEncodeThreads) dst[i] = (uint8_t)cmp_code(src[i], mn, range, 255.0f);
    }
    return;
  }
  __shared__ float pt[4][CT];
  __shared__ uint8_t tile[CT * TS];
  uint8_t* data = obj + 16 + (int64_t)cols * 8;
  for (int c0 = 0; c0 < cols; c0 += CT) {
    const int gc = cols - c0 < CT ? cols - c0 : CT;
    if (tid < gc) {
      const uint32_t* w = (const uint32_t*)(obj + 16 + (int64_t)(c0 + tid) * 8);
      const uint32_t w0 = w[0], w1 = w[1];
      // min + range * 1.52590218966964e-05f * word, left to right: what the reader computes
      const float scaled = range * 1.52590218966964e-05F;
      pt[0][tid] = mn + scaled * (float)(w0 & 0xffffu);
      pt[1][tid] = mn + scaled * (float)(w0 >> 16);
      pt[2][tid] = mn + scaled * (float)(w1 & 0xffffu);
      pt[3][tid] = mn + scaled * (float)(w1 >> 16);
    }
    __syncthreads();
    for (int i = tid; i < nr * gc; i += kCmpEncodeThreads) {
      const int r = i / gc, c = i - r * gc;
      const float v = src[(int64_t)r * cols + c0 + c];
      const float p0 = pt[0][c], p25 = pt[1][c], p75 = pt[2][c], p100 = pt[3][c];
      int b;
      if (v < p25) b = cmp_segment(v, p0, p25, 64.0f, 0);
      else if (v < p75) b = cmp_segment(v, p25, p75, 128.0f, 64);
      else b = cmp_segment(v, p75, p100, 63.0f, 192);
      tile[c * TS + r] = (uint8_t)b;
    }
    __syncthreads();
    for (int i = tid; i < nr * gc; i += kCmpEncodeThreads) {
      const int c = i / nr, r = i - c * nr;
      data[(int64_t)(c0 + c) * rows + r0 + r] = tile[c * TS + r];
    }
    __syncthreads();
  }
}

bool cmp_args_ok(const CmpArgs& a) {
  return a.n_items > 0 && a.n > 0 && a.cols > 0 && a.feats && a.row_off && a.obj_off && a.stats && a.out && a.item_mat && a.item_blk &&
         (a.method == 1 || a.method == 2 || a.method == 3 || a.method == 5);
}

}  // namespace

hipError_t launch_cmp_minmax(const CmpArgs& a, hipStream_t s) {
  if (!cmp_args_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cmp_minmax_kernel, dim3((unsigned)a.n_items), dim3(kCmpMinmaxThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cmp_select(const CmpArgs& a, hipStream_t s) {
  if (!cmp_args_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cmp_select_kernel, dim3((unsigned)a.n_items), dim3(kCmpSelectThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cmp_encode(const CmpArgs& a, hipStream_t s) {
  if (!cmp_args_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cmp_encode_kernel, dim3((unsigned)a.n_items), dim3(kCmpEncodeThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
