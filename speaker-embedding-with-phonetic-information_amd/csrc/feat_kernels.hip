// Feature-stage kernels (feat_kernels.h): MFCC of a ragged batch of waveforms and Kaldi's energy VAD.
// MFCC: one 64-lane workgroup (one wave) per frame; the frame lives in LDS (staging window, then the real and imaginary
// planes of an in-place radix-2 FFT with a bit-reversed load, then power spectrum and log mel energies).  Every sum is
// taken in an order that depends on the options only, so a frame's bytes do not depend on the batch.
#include "feat_kernels.h"

#include <float.h>

#include "counter_rng.h"

namespace xv {

namespace {

constexpr int kWave = 64;

// Sum over the wave: xor butterfly, every lane ends with the same value (fixed order).
__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

// Largest u with off[u] <= r (off non-decreasing, off[0] <= r < off[n]); empty utterances are stepped over.
__device__ inline int find_segment(const int32_t* off, int n, int r) {
  int lo = 0, hi = n;   // answer in [lo, hi)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= r) lo = mid;
    else hi = mid;
  }
  return lo;
}

// The dither: 64 bits from (utterance seed, frame, sample) of the generator in counter_rng.h, through Box-Muller.
__device__ inline float dither_gauss(uint64_t seed, int frame, int i) {
  const uint64_t r = counter_bits(seed, (uint32_t)frame, (uint32_t)i);
  const float u1 = counter_unit_open0(r);                                         // (0, 1], 24 bits
  const float u2 = (float)(uint32_t)((r >> 8) & 0xffffff) * (1.0f / 16777216.0f); // [0, 1)
  return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

template <typename T>
__global__ __launch_bounds__(kWave) void mfcc_kernel(const MfccArgs a) {
  extern __shared__ __align__(16) float lds[];
  const int P = a.padded, L = a.frame_len;
  float* stage = lds;          // [P]  the window as read, later the power spectrum
  float* re = lds + P;         // [P]
  float* im = lds + 2 * P;     // [P]
  const int lane = threadIdx.x;
  const int f = blockIdx.x;
  if (f >= a.total_frames) return;
  const int u = find_segment(a.row_off, a.n_utts, f);
  const int t = f - a.row_off[u];
  const int64_t base = a.sample_off[u];
  const int64_t n = a.sample_off[u + 1] - base;
  const T* x = (const T*)a.samples + base;
  const int64_t start = a.snip_edges ? (int64_t)t * a.frame_shift
                                     : (int64_t)t * a.frame_shift + a.frame_shift / 2 - L / 2;
  const uint64_t seed = a.dither != 0.f ? a.utt_seed[u] : 0;

  // 1-2. the window (reflected at the ends without snip-edges), dithered
  float part = 0.f;
  for (int i = lane; i < L; i += kWave) {
    int64_t s = start + i;
    if (!a.snip_edges) {
      while (s < 0 || s >= n) s = s < 0 ? -s - 1 : 2 * n - 1 - s;
    }
    float v = (float)x[s];
    if (a.dither != 0.f) v += a.dither * dither_gauss(seed, t, i);
    stage[i] = v;
    part += v;
  }
  // 3. DC offset
  if (a.remove_dc) {
    const float mean = wave_sum(part) / (float)L;
    for (int i = lane; i < L; i += kWave) stage[i] -= mean;
  }
  __syncthreads();
  // 4. raw log energy
  float log_energy = 0.f;
  if (a.use_energy && a.raw_energy) {
    float e = 0.f;
    for (int i = lane; i < L; i += kWave) e = fmaf(stage[i], stage[i], e);
    log_energy = logf(fmaxf(wave_sum(e), FLT_EPSILON));
  }
  // 5-7. pre-emphasis, window, zero padding; stored in bit-reversed order for the in-place FFT
  const int shift = 32 - a.log2_padded;
  float e_win = 0.f;
  for (int i = lane; i < P; i += kWave) {
    float v = 0.f;
    if (i < L) {
      const float cur = stage[i];
      const float prev = stage[i > 0 ? i - 1 : 0];
      v = (cur - a.preemph * prev) * a.window[i];
      e_win = fmaf(v, v, e_win);
    }
    const int j = (int)(__brev((unsigned)i) >> shift);
    re[j] = v;
    im[j] = 0.f;
  }
  if (a.use_energy && !a.raw_energy) log_energy = logf(fmaxf(wave_sum(e_win), FLT_EPSILON));
  if (a.use_energy && a.has_energy_floor && log_energy < a.log_energy_floor) log_energy = a.log_energy_floor;
  __syncthreads();
  // FFT: log2 P radix-2 decimation-in-time stages
  for (int s = 0; s < a.log2_padded; ++s) {
    const int half = 1 << s;
    const int tw_shift = a.log2_padded - 1 - s;
    for (int b = lane; b < (P >> 1); b += kWave) {
      const int j = b & (half - 1);
      const int i0 = ((b >> s) << (s + 1)) + j;
      const int i1 = i0 + half;
      const float2 w = ((const float2*)a.twiddle)[j << tw_shift];
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
  // power spectrum, bins 0 .. P/2
  for (int k = lane; k <= (P >> 1); k += kWave) stage[k] = re[k] * re[k] + im[k] * im[k];
  __syncthreads();
  // 8-9. mel energies and their logs (re[] is free now)
  for (int m = lane; m < a.num_bins; m += kWave) {
    const float* w = a.mel_w + a.mel_woff[m];
    const float* p = stage + a.mel_first[m];
    const int len = a.mel_len[m];
    float e = 0.f;
    for (int k = 0; k < len; ++k) e = fmaf(w[k], p[k], e);
    re[m] = logf(fmaxf(e, FLT_EPSILON));
  }
  __syncthreads();
  // DCT, lifter, c0
  for (int c = lane; c < a.num_ceps; c += kWave) {
    float acc = 0.f;
    for (int m = 0; m < a.num_bins; ++m) acc = fmaf(a.dct_t[m * a.num_ceps + c], re[m], acc);
    acc *= a.lifter[c];
    if (c == 0 && a.use_energy) acc = log_energy;
    a.out[(size_t)f * a.num_ceps + c] = acc;
  }
}

// thr[u]: one wave per utterance; lane l adds rows l, l + 64, ... in fp64, then the xor butterfly.
__global__ __launch_bounds__(kWave) void vad_threshold_kernel(const VadArgs a) {
  const int u = blockIdx.x;
  if (u >= a.n_utts) return;
  const int r0 = a.row_off[u], r1 = a.row_off[u + 1];
  double s = 0.0;
  for (int r = r0 + (int)threadIdx.x; r < r1; r += kWave) s += (double)a.feats[(size_t)r * a.dim];
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    double thr = (double)a.energy_threshold;
    if (r1 > r0 && a.energy_mean_scale != 0.f) thr += (double)a.energy_mean_scale * (s / (double)(r1 - r0));
    a.thr[u] = (float)thr;
  }
}

__global__ __launch_bounds__(256) void vad_decision_kernel(const VadArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.total_rows) return;
  const int u = find_segment(a.row_off, a.n_utts, r);
  const int r0 = a.row_off[u], r1 = a.row_off[u + 1];
  const float thr = a.thr[u];
  const int lo = max(r0, r - a.frames_context), hi = min(r1 - 1, r + a.frames_context);
  int num = 0;
  for (int v = lo; v <= hi; ++v) num += a.feats[(size_t)v * a.dim] > thr ? 1 : 0;
  const int den = hi - lo + 1;
  a.out[r] = (float)num >= (float)den * a.proportion_threshold ? 1.f : 0.f;
}

template <typename T>
hipError_t launch_mfcc(const MfccArgs& a, hipStream_t s) {
  if (a.total_frames <= 0) return hipSuccess;
  if (a.padded < 2 || a.padded > kMfccMaxPadded || (1 << a.log2_padded) != a.padded || a.frame_len > a.padded || a.frame_len < 1)
    return hipErrorInvalidValue;
  // the log mel energies live in re[0 .. num_bins) (one LDS plane of `padded` floats), the DCT reads num_ceps <= num_bins of them
  if (a.num_bins < 1 || a.num_bins > a.padded || a.num_ceps < 1 || a.num_ceps > a.num_bins) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mfcc_kernel<T>, dim3(a.total_frames), dim3(kWave), mfcc_lds_bytes(a.padded), s, a);
  return hipGetLastError();
}

}  // namespace

size_t mfcc_lds_bytes(int padded) { return (size_t)3 * padded * sizeof(float); }

hipError_t launch_mfcc_f32(const MfccArgs& a, hipStream_t s) { return launch_mfcc<float>(a, s); }
hipError_t launch_mfcc_i16(const MfccArgs& a, hipStream_t s) { return launch_mfcc<int16_t>(a, s); }

hipError_t launch_vad_energy(const VadArgs& a, hipStream_t s) {
  if (a.n_utts <= 0 || a.total_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(vad_threshold_kernel, dim3(a.n_utts), dim3(kWave), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(vad_decision_kernel, dim3((a.total_rows + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
