// Augmentation-stage kernels (reverb_kernels.h): partitioned overlap-save convolution of a ragged batch, power sums, noise
// mixing and the final scale / shift / trim / 16-bit conversion.  Workgroups of 256 threads; the FFT is a 4096-point radix-2
// decimation-in-time transform on two fp32 planes in LDS (bit-reversed store, natural-order result), eight butterflies per
// thread and stage.
#include "reverb_kernels.h"

namespace xv {

namespace {

// Sum over the workgroup in a fixed tree; every thread gets the result.  red: kRvThreads doubles in LDS.
__device__ inline double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();   // red may still be read from an earlier call
  red[t] = v;
  __syncthreads();
#pragma unroll
  for (int m = kRvThreads / 2; m >= 1; m >>= 1) {
    if (t < m) red[t] += red[t + m];
    __syncthreads();
  }
  return red[0];
}

__device__ inline int brev12(int i) { return (int)(__brev((unsigned)i) >> (32 - kRvLog2N)); }

// In-place FFT of re/im (bit-reversed order in, natural order out).  The planes must be complete and synchronised on entry;
// they are synchronised on return.
__device__ inline void fft_lds(float* re, float* im, const float2* __restrict__ tw) {
  const int t = threadIdx.x;
  for (int s = 0; s < kRvLog2N; ++s) {
    const int half = 1 << s;
    const int tw_shift = kRvLog2N - 1 - s;
#pragma unroll
    for (int q = 0; q < kRvN / 2 / kRvThreads; ++q) {
      const int b = t + q * kRvThreads;
      const int j = b & (half - 1);
      const int i0 = ((b >> s) << (s + 1)) + j;
      const int i1 = i0 + half;
      const float2 w = tw[j << tw_shift];
      const float xr = re[i1], xi = im[i1];
      const float tr = w.x * xr - w.y * xi;
      const float ti = w.x * xi + w.y * xr;
      const float ur = re[i0], ui = im[i0];
      re[i0] = ur + tr;
      im[i0] = ui + ti;
      re[i1] = ur - tr;
      im[i1] = ui - ti;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kRvThreads) void rv_power_kernel(const RvPowerArgs a) {
  __shared__ double red[kRvThreads];
  const int c = blockIdx.x;
  if (c >= a.n_chunks) return;
  const float* x = a.sig + a.chunk_off[c];
  const int n = a.chunk_len[c];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += kRvThreads) {
    const double v = (double)x[i];
    acc = fma(v, v, acc);
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) a.out[c] = acc;
}

__global__ __launch_bounds__(kRvThreads) void rv_rir_spectra_kernel(const RvRirSpecArgs a) {
  __shared__ float re[kRvN];
  __shared__ float im[kRvN];
  const int item = blockIdx.x;
  if (item >= a.n_items) return;
  const float* h = a.sig + a.src_off[item];
  const int n = a.src_len[item];
  for (int i = threadIdx.x; i < kRvN; i += kRvThreads) {
    const int j = brev12(i);
    re[j] = i < n ? h[i] : 0.f;
    im[j] = 0.f;
  }
  __syncthreads();
  fft_lds(re, im, a.twiddle);
  float2* out = a.hspec + (size_t)item * kRvN;
  for (int k = threadIdx.x; k < kRvN; k += kRvThreads) out[k] = make_float2(re[k], im[k]);
}

// Block b of an utterance: the spectrum of x[(b - 1) H, (b + 1) H), zeros outside the signal.
__global__ __launch_bounds__(kRvThreads) void rv_sig_spectra_kernel(const RvConvArgs a) {
  __shared__ float re[kRvN];
  __shared__ float im[kRvN];
  const int item = blockIdx.x;
  if (item >= a.n_items) return;
  const RvUtt& U = a.utts[a.item_utt[item]];
  const int b = a.item_blk[item];
  const float* x = a.sig + U.in_off;
  const int64_t base = ((int64_t)b - 1) * kRvH;
  for (int i = threadIdx.x; i < kRvN; i += kRvThreads) {
    const int64_t s = base + i;
    const int j = brev12(i);
    re[j] = (s >= 0 && s < U.n) ? x[s] : 0.f;
    im[j] = 0.f;
  }
  __syncthreads();
  fft_lds(re, im, a.twiddle);
  float2* out = a.xspec + (size_t)(U.xspec_off + b) * kRvN;
  for (int k = threadIdx.x; k < kRvN; k += kRvThreads) out[k] = make_float2(re[k], im[k]);
}

// Output block b: y[b H, (b + 1) H) = sum over partitions p of (block b - p of the signal) * (partition p of the RIR), the valid
// half of the circular product.  Both products are spectra of real sequences, so A + iE transforms back to full + i early.
__global__ __launch_bounds__(kRvThreads) void rv_conv_kernel(const RvConvArgs a) {
  __shared__ float re[kRvN];
  __shared__ float im[kRvN];
  __shared__ double red[kRvThreads];
  const int item = blockIdx.x;
  if (item >= a.n_items) return;
  const RvUtt& U = a.utts[a.item_utt[item]];
  const int b = a.item_blk[item];
  const int P = min(U.P, b + 1), Pe = min(U.Pe, b + 1);
  const float2* X = a.xspec + (size_t)(U.xspec_off + b) * kRvN;   // block b - p lies p spectra before
  const float2* Hf = a.hspec + (size_t)U.hfull * kRvN;
  const float2* He = a.hspec + (size_t)U.hearly * kRvN;
  for (int k = threadIdx.x; k < kRvN; k += kRvThreads) {
    float ar = 0.f, ai = 0.f, er = 0.f, ei = 0.f;
    for (int p = 0; p < P; ++p) {
      const float2 x = X[k - (ptrdiff_t)p * kRvN];
      const float2 h = Hf[k + (size_t)p * kRvN];
      ar += x.x * h.x - x.y * h.y;
      ai += x.x * h.y + x.y * h.x;
    }
    for (int p = 0; p < Pe; ++p) {
      const float2 x = X[k - (ptrdiff_t)p * kRvN];
      const float2 h = He[k + (size_t)p * kRvN];
      er += x.x * h.x - x.y * h.y;
      ei += x.x * h.y + x.y * h.x;
    }
    // Z = A + iE; the inverse transform is conj(FFT(conj Z)) / N
    const int j = brev12(k);
    re[j] = ar - ei;
    im[j] = -(ai + er);
  }
  __syncthreads();
  fft_lds(re, im, a.twiddle);
  const float inv = 1.0f / (float)kRvN;
  float* y = a.y + U.y_off;
  double acc = 0.0;
  for (int j = threadIdx.x; j < kRvH; j += kRvThreads) {
    const int64_t s = (int64_t)b * kRvH + j;
    if (s < U.ext_len) {
      y[s] = re[kRvH + j] * inv;
      const double e = (double)(im[kRvH + j] * inv);
      acc = fma(e, e, acc);
    }
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) a.epart[U.epart_off + b] = acc;
}

// Filters of at most kRvDirectMax taps: the sums themselves, in fp64, rounded once.
__global__ __launch_bounds__(kRvThreads) void rv_conv_direct_kernel(const RvConvArgs a) {
  __shared__ double red[kRvThreads];
  __shared__ float hs[kRvDirectMax];
  const int item = blockIdx.x;
  if (item >= a.n_items) return;
  const RvUtt& U = a.utts[a.item_utt[item]];
  const int c = a.item_blk[item];
  const float* x = a.sig + U.in_off;
  const int L = min(U.rir_len, kRvDirectMax);
  if ((int)threadIdx.x < L) hs[threadIdx.x] = a.sig[U.h_off + threadIdx.x];
  __syncthreads();
  float* y = a.y + U.y_off;
  double eacc = 0.0;
  for (int i = threadIdx.x; i < kRvDirectChunk; i += kRvThreads) {
    const int64_t s = (int64_t)c * kRvDirectChunk + i;
    if (s >= U.ext_len) break;
    double full = 0.0, early = 0.0;
    for (int j = 0; j < L; ++j) {
      const int64_t idx = s - j;
      if (idx >= 0 && idx < U.n) full = fma((double)hs[j], (double)x[idx], full);
    }
    for (int j = U.e0; j < U.e1 && j < L; ++j) {
      const int64_t idx = s - (j - U.e0);
      if (idx >= 0 && idx < U.n) early = fma((double)hs[j], (double)x[idx], early);
    }
    y[s] = (float)full;
    const double e = (double)(float)early;
    eacc = fma(e, e, eacc);
  }
  eacc = block_sum(eacc, red);
  if (threadIdx.x == 0) a.epart[U.epart_off + c] = eacc;
}

__global__ __launch_bounds__(kRvThreads) void rv_mix_kernel(const RvMixArgs a) {
  __shared__ double red[kRvThreads];
  const int item = blockIdx.x;
  if (item >= a.n_items) return;
  const RvUtt& U = a.utts[a.item_utt[item]];
  const int c = a.item_blk[item];
  float* y = a.y + U.y_off;
  const float* src = U.rir_len > 0 ? y : a.sig + U.in_off;
  const RvAdd* adds = a.adds + U.add_first;
  double acc = 0.0;
  for (int i = threadIdx.x; i < kRvChunk; i += kRvThreads) {
    const int64_t s = (int64_t)c * kRvChunk + i;
    if (s >= U.ext_len) break;
    float v = src[s];
    for (int k = 0; k < U.add_count; ++k) {
      const int64_t j = s - adds[k].start;
      if (j >= 0 && j < adds[k].len) v = __fadd_rn(v, __fmul_rn(adds[k].scale, a.sig[adds[k].off + j]));
    }
    y[s] = v;
    acc = fma((double)v, (double)v, acc);
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) a.apart[U.apart_off + c] = acc;
}

__global__ __launch_bounds__(kRvThreads) void rv_finish_kernel(const RvFinishArgs a) {
  const int item = blockIdx.x;
  if (item >= a.n_items) return;
  const RvUtt& U = a.utts[a.item_utt[item]];
  const int c = a.item_blk[item];
  const float* y = a.y + U.y_off;
  const bool repeat = U.out_len > U.n;
  unsigned clipped = 0;
  for (int i = threadIdx.x; i < kRvChunk; i += kRvThreads) {
    const int64_t o = (int64_t)c * kRvChunk + i;
    if (o >= U.out_len) break;
    const int64_t s = repeat ? o % U.ext_len : o + U.shift;
    const float v = __fmul_rn(y[s], U.scale);
    a.out_f32[U.out_off + o] = v;
    if (a.out_i16) {
      int16_t q;
      if (v >= 32768.f) {
        q = 32767;
        ++clipped;
      } else if (v <= -32769.f) {
        q = -32768;
        ++clipped;
      } else if (v != v) {
        q = 0;
      } else {
        q = (int16_t)(int)v;   // toward zero
      }
      a.out_i16[U.out_off + o] = q;
    }
  }
  if (a.clipped && clipped) atomicAdd(a.clipped + a.item_utt[item], (unsigned long long)clipped);
}

}  // namespace

hipError_t launch_rv_power(const RvPowerArgs& a, hipStream_t s) {
  if (a.n_chunks <= 0) return hipSuccess;
  hipLaunchKernelGGL(rv_power_kernel, dim3(a.n_chunks), dim3(kRvThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rv_rir_spectra(const RvRirSpecArgs& a, hipStream_t s) {
  if (a.n_items <= 0) return hipSuccess;
  hipLaunchKernelGGL(rv_rir_spectra_kernel, dim3(a.n_items), dim3(kRvThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rv_sig_spectra(const RvConvArgs& a, hipStream_t s) {
  if (a.n_items <= 0) return hipSuccess;
  hipLaunchKernelGGL(rv_sig_spectra_kernel, dim3(a.n_items), dim3(kRvThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rv_conv(const RvConvArgs& a, hipStream_t s) {
  if (a.n_items <= 0) return hipSuccess;
  hipLaunchKernelGGL(rv_conv_kernel, dim3(a.n_items), dim3(kRvThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rv_conv_direct(const RvConvArgs& a, hipStream_t s) {
  if (a.n_items <= 0) return hipSuccess;
  hipLaunchKernelGGL(rv_conv_direct_kernel, dim3(a.n_items), dim3(kRvThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rv_mix(const RvMixArgs& a, hipStream_t s) {
  if (a.n_items <= 0) return hipSuccess;
  hipLaunchKernelGGL(rv_mix_kernel, dim3(a.n_items), dim3(kRvThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rv_finish(const RvFinishArgs& a, hipStream_t s) {
  if (a.n_items <= 0) return hipSuccess;
  hipLaunchKernelGGL(rv_finish_kernel, dim3(a.n_items), dim3(kRvThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
