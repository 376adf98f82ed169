// nnet-am-compute's kernels: see nnet2_kernels.h.
#include "nnet2_kernels.h"

#include <math.h>

namespace xv {

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
  return v;
}

__device__ __forceinline__ void split_store(float y, uint16_t* hi, uint16_t* lo) {
  const _Float16 h = (_Float16)y;
  const _Float16 l = (_Float16)((y - (float)h) * kNnet2LoScale);
  *hi = __builtin_bit_cast(uint16_t, h);
  *lo = __builtin_bit_cast(uint16_t, l);
}

// ----------------------------------------------------------------------------------------------------------- prep and row kernel
// output j of the row at p: the nonlinearity alone
__device__ __forceinline__ float row_value(const float* p, int j, int group, int nonlin) {
  if (nonlin == 1) {
    float s = 0.f;
    const float* g = p + (int64_t)j * group;
    for (int i = 0; i < group; ++i) s = fmaf(g[i], g[i], s);
    return sqrtf(s);
  }
  const float v = p[j];
  return nonlin == 2 ? (v > 0.f ? v : 0.f) : v;
}

template <bool kPlain>
__global__ __launch_bounds__(kNnet2RowThreads) void nnet2_row_kernel(Nnet2RowArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (kNnet2RowThreads / 64) + (threadIdx.x >> 6);
  if (r >= a.rows) return;
  const float* p = a.pre + r * a.ldp;
  const int nonlin = kPlain ? 0 : a.nonlin;
  const int group = nonlin == 1 ? a.in_dim / a.out_dim : 1;
  float scale = 1.f;
  if (!kPlain && a.normalize) {
    float ss = 0.f;
    for (int j = lane; j < a.out_dim; j += 64) {
      const float y = row_value(p, j, group, nonlin);
      ss = fmaf(y, y, ss);
    }
    ss = wave_sum(ss);
    scale = 1.f / sqrtf(fmaxf(ss / (float)a.out_dim, 0x1p-66f));
  }
  uint16_t* hi = a.hi + r * a.ld;
  uint16_t* lo = a.lo + r * a.ld;
  for (int j = lane; j < a.ld; j += 64) {
    float y = 0.f;
    if (j < a.out_dim) y = row_value(p, j, group, nonlin) * scale;
    split_store(y, hi + j, lo + j);
  }
}

// ------------------------------------------------------------------------------------------------------------- the spliced affine
__global__ __launch_bounds__(kNnet2AffineThreads) void nnet2_affine_kernel(Nnet2AffineArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int m0 = blockIdx.x * kNnet2TileM + (wave & 1) * 32;
  const int n0 = blockIdx.y * kNnet2TileN + (wave >> 1) * 64;
  const int64_t ldw = (int64_t)a.n_ctx * a.k_pad;
  f32x4 acc[2][4], accx[2][4];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      accx[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  // n0 + 16 nt + r < n_pad always: the grid covers n_pad exactly
  const uint16_t *wh[4], *wl[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int64_t off = (int64_t)(n0 + 16 * nt + r) * ldw + 8 * q;
    wh[nt] = a.w_hi + off;
    wl[nt] = a.w_lo + off;
  }
  for (int ci = 0; ci < a.n_ctx; ++ci) {
    const int c = a.ctx[ci];
    const uint16_t *xh[2], *xl[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      int row = m0 + 16 * mt + r + c;
      row = row < a.row_lo ? a.row_lo : (row >= a.row_hi ? a.row_hi - 1 : row);
      const int64_t off = (int64_t)row * a.ldx + 8 * q;
      xh[mt] = a.x_hi + off;
      xl[mt] = a.x_lo + off;
    }
    const int wk = ci * a.k_pad;
    for (int k0 = 0; k0 < a.k_pad; k0 += kNnet2TileK) {
      f16x8 ah[2], al[2], bh[4], bl[4];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        ah[mt] = *(const f16x8*)(xh[mt] + k0);
        al[mt] = *(const f16x8*)(xl[mt] + k0);
      }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        bh[nt] = *(const f16x8*)(wh[nt] + wk + k0);
        bl[nt] = *(const f16x8*)(wl[nt] + wk + k0);
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mt], bh[nt], acc[mt][nt], 0, 0, 0);
          accx[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mt], bl[nt], accx[mt][nt], 0, 0, 0);
          accx[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[mt], bh[nt], accx[mt][nt], 0, 0, 0);
        }
    }
  }
  // C: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int n = n0 + 16 * nt + r;
    if (n >= a.n) continue;
    const float b = a.bias[n];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + 16 * mt + 4 * q + i;
        if (m < a.rows) a.out[(int64_t)m * a.ldo + n] = (acc[mt][nt][i] + accx[mt][nt][i] * (1.f / kNnet2LoScale)) * a.w_unscale + b;
      }
  }
}

// ------------------------------------------------------------------------------------------------------------------------ the head
__device__ __forceinline__ float block_fold(float v, float* red, bool is_max) {
  v = is_max ? wave_max(v) : wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = red[0];
  for (int w = 1; w < kNnet2HeadThreads / 64; ++w) t = is_max ? fmaxf(t, red[w]) : t + red[w];
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(kNnet2HeadThreads) void nnet2_head_kernel(Nnet2HeadArgs a) {
  __shared__ float row[kNnet2HeadMaxCols];
  __shared__ float red[kNnet2HeadThreads / 64];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int64_t src = a.src_row ? a.src_row[r] : r;
  const float* x = a.logits + src * a.ldl;
  float m = -INFINITY;
  for (int c = tid; c < a.n; c += kNnet2HeadThreads) {
    const float v = x[c];
    row[c] = v;
    m = fmaxf(m, v);
  }
  m = block_fold(m, red, true);
  float s = 0.f;
  for (int c = tid; c < a.n; c += kNnet2HeadThreads) {
    const float e = expf(row[c] - m);
    row[c] = e;
    s += e;
  }
  s = block_fold(s, red, false);
  for (int c = tid; c < a.n; c += kNnet2HeadThreads) row[c] = fmaxf(row[c] / s, 1e-20f);
  __syncthreads();
  float* out = a.out + (int64_t)r * a.n_out;
  for (int g = tid; g < a.n_out; g += kNnet2HeadThreads) {
    float p;
    if (a.start) {
      p = 0.f;
      for (int c = a.start[g]; c < a.start[g + 1]; ++c) p += row[c];
    } else {
      p = row[g];
    }
    if (a.inv_prior) p *= a.inv_prior[g];
    if (a.apply_log) p = logf(fmaxf(p, 1e-20f));
    out[g] = p;
  }
}

}  // namespace

hipError_t launch_nnet2_prep(const Nnet2PrepArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  Nnet2RowArgs r{};
  r.pre = a.x;
  r.rows = a.rows;
  r.ldp = a.cols;
  r.in_dim = r.out_dim = a.cols;
  r.hi = a.hi;
  r.lo = a.lo;
  r.ld = a.ld;
  const int per = kNnet2RowThreads / 64;
  hipLaunchKernelGGL(nnet2_row_kernel<true>, dim3((unsigned)((a.rows + per - 1) / per)), dim3(kNnet2RowThreads), 0, s, r);
  return hipGetLastError();
}

hipError_t launch_nnet2_row(const Nnet2RowArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  const int per = kNnet2RowThreads / 64;
  hipLaunchKernelGGL(nnet2_row_kernel<false>, dim3((unsigned)((a.rows + per - 1) / per)), dim3(kNnet2RowThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_nnet2_affine(const Nnet2AffineArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(nnet2_affine_kernel, dim3((unsigned)((a.rows + kNnet2TileM - 1) / kNnet2TileM), (unsigned)(a.n_pad / kNnet2TileN)),
                     dim3(kNnet2AffineThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_nnet2_head(const Nnet2HeadArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(nnet2_head_kernel, dim3((unsigned)a.rows), dim3(kNnet2HeadThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
