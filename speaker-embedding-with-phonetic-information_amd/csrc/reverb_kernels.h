// Device kernels of the augmentation stage (stage 2 of egs/sre/v2/run_sre10.sh: wav-reverberate).  Kept out of kernels.hip for
// the reason feat_kernels.* are: KERNELS_SHA names the extraction kernels only.
//
// A launch works on a ragged batch.  The host (reverb.cc) lays every signal - inputs, noises, impulse responses - into one fp32
// array and describes each utterance with an RvUtt; each kernel takes a list of work items (utterance, block) built by the
// host, so a workgroup never searches for its place.  Every sum is taken in an order fixed by the utterance's own lengths
// (fixed-size chunks, fp64 partial per chunk by a fixed tree, partials added in order on the host): no float atomics, and an
// utterance's bytes do not depend on what else is in the launch.
//
// Convolution: uniformly partitioned overlap-save, FFT of kRvN = 4096 points in LDS (two fp32 planes, 32 KiB), hop and partition
// kRvH = 2048.  rv_sig_spectra transforms each signal block once; rv_rir_spectra each partition of each distinct filter once;
// rv_conv multiplies and adds over the partitions in the frequency domain and does one inverse FFT per output block, which
// carries the full convolution in its real part and the "early" one (the slice of the same RIR around its peak, wanted only
// for its energy) in its imaginary part.  Filters of at most kRvDirectMax taps skip the FFT (rv_conv_direct, fp64 sums).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace xv {

constexpr int kRvN = 4096;         // FFT size
constexpr int kRvLog2N = 12;
constexpr int kRvH = 2048;         // hop = partition size = kRvN / 2
constexpr int kRvThreads = 256;
constexpr int kRvDirectMax = 64;   // longest filter convolved in the time domain
constexpr int kRvDirectChunk = 4096;   // outputs per workgroup of rv_conv_direct
constexpr int kRvChunk = 16384;    // samples per workgroup (and per fp64 partial) of the power, mix and finish kernels

struct RvUtt {
  int64_t in_off, n;          // the input in sig[]
  int64_t ext_len;            // n + rir_len - 1 with a RIR, else n: length of y
  int64_t y_off;              // the utterance's part of y[]
  int64_t out_off, out_len;   // its part of the outputs
  int64_t h_off;              // the RIR in sig[] (already scaled by 1/32768)
  int64_t xspec_off;          // first block spectrum of the utterance in xspec (in units of kRvN complex values)
  int64_t epart_off;          // first partial of the early energy
  int64_t apart_off;          // first partial of the power after mixing
  int32_t rir_len;            // 0: no RIR
  int32_t e0, e1;             // the early slice [e0, e1) of the RIR
  int32_t hfull, P;           // first partition spectrum of the RIR in hspec, and how many
  int32_t hearly, Pe;         // the same for the early slice
  int32_t shift;              // samples dropped in front when the output is not longer than the input
  int32_t add_first, add_count;   // its additive signals in the RvAdd list
  float scale;                // final factor (volume or normalisation)
};

struct RvAdd {
  int64_t off, len;           // the noise in sig[]
  int64_t start;              // sample offset in the (extended) signal; may lie beyond its end
  float scale;
  int32_t pad;
};

// out[c] = sum of squares of sig[chunk_off[c] .. + chunk_len[c]) in fp64
struct RvPowerArgs {
  const float* sig;
  const int64_t* chunk_off;
  const int32_t* chunk_len;
  int n_chunks;
  double* out;
};
hipError_t launch_rv_power(const RvPowerArgs& a, hipStream_t s);

// hspec[item] = FFT of sig[src_off[item] .. + src_len[item]) zero-padded to kRvN (src_len <= kRvH)
struct RvRirSpecArgs {
  const float* sig;
  const int64_t* src_off;
  const int32_t* src_len;
  int n_items;
  const float2* twiddle;      // [kRvN / 2]: cos, -sin of 2 pi j / kRvN
  float2* hspec;
};
hipError_t launch_rv_rir_spectra(const RvRirSpecArgs& a, hipStream_t s);

struct RvConvArgs {
  const float* sig;
  const RvUtt* utts;
  const int32_t* item_utt;    // work items: (utterance, block)
  const int32_t* item_blk;
  int n_items;
  const float2* twiddle;
  const float2* hspec;
  float2* xspec;
  float* y;
  double* epart;
};
hipError_t launch_rv_sig_spectra(const RvConvArgs& a, hipStream_t s);
hipError_t launch_rv_conv(const RvConvArgs& a, hipStream_t s);
hipError_t launch_rv_conv_direct(const RvConvArgs& a, hipStream_t s);

// y = (convolved signal, or the input without a RIR) + the scaled additive signals; apart = partial powers of the result
struct RvMixArgs {
  const float* sig;
  const RvUtt* utts;
  const RvAdd* adds;
  const int32_t* item_utt;
  const int32_t* item_blk;    // chunk of kRvChunk samples of y
  int n_items;
  float* y;
  double* apart;
};
hipError_t launch_rv_mix(const RvMixArgs& a, hipStream_t s);

// out_f32 = scale * y shifted, trimmed or repeated; out_i16 (optional) = that truncated toward zero and saturated,
// clipped[u] (optional with it) += samples that were saturated
struct RvFinishArgs {
  const RvUtt* utts;
  const int32_t* item_utt;
  const int32_t* item_blk;    // chunk of kRvChunk output samples
  int n_items;
  const float* y;
  float* out_f32;
  int16_t* out_i16;
  unsigned long long* clipped;
};
hipError_t launch_rv_finish(const RvFinishArgs& a, hipStream_t s);

}  // namespace xv
