// Device kernels of the feature stage (stage 1 of egs/sre/v2/run_sre10.sh: compute-mfcc-feats, compute-vad).
// Kept out of kernels.hip/kernels.h for the reason plda_kernels.* are: KERNELS_SHA names the extraction kernels only.
// fp32 arithmetic like Kaldi's float build; every frame is computed by one wave in a fixed order, every utterance mean by
// one wave in a fixed order: a result depends on the utterance and the options, never on the batch it sits in.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace xv {

constexpr int kMfccMaxPadded = 4096;   // largest FFT size (power of two) the kernel is launched with

// MFCC of a ragged batch: utterance u holds samples [sample_off[u], sample_off[u+1]) and frames
// [row_off[u], row_off[u+1]) of out.  One wave per frame.  The tables come from the host (feat.cc), so the kernel has one
// code path whatever the window type or the mel scale options.
struct MfccArgs {
  const void* samples;          // float or int16_t, Kaldi's unscaled range
  const int64_t* sample_off;    // [n_utts + 1]
  const int32_t* row_off;       // [n_utts + 1]
  const uint64_t* utt_seed;     // [n_utts]; read only when dither != 0
  int n_utts, total_frames;
  int frame_len, frame_shift;   // L, S in samples
  int padded, log2_padded;      // P and log2 P
  int snip_edges;
  float dither, preemph;
  int remove_dc, raw_energy, use_energy;
  float log_energy_floor;       // log(energy_floor); applied when has_energy_floor
  int has_energy_floor;
  const float* window;          // [L]
  const float* twiddle;         // [P/2][2]: cos, -sin of 2 pi j / P
  int num_bins, num_ceps;
  const int32_t* mel_first;     // [num_bins] first FFT bin of each filter
  const int32_t* mel_len;       // [num_bins]
  const int32_t* mel_woff;      // [num_bins] offset of the filter's weights in mel_w
  const float* mel_w;
  const float* dct_t;           // [num_bins][num_ceps]: the DCT matrix, transposed (lanes read consecutive addresses)
  const float* lifter;          // [num_ceps] (all ones when the lifter is off)
  float* out;                   // [total_frames][num_ceps]
};
size_t mfcc_lds_bytes(int padded);
hipError_t launch_mfcc_f32(const MfccArgs& a, hipStream_t s);
hipError_t launch_mfcc_i16(const MfccArgs& a, hipStream_t s);

// Energy VAD (Kaldi's ComputeVadEnergy) of a ragged batch of feature matrices; c0 is column 0.
//   thr[u] = energy_threshold + energy_mean_scale * mean_t c0[u][t]      (one wave per utterance, fp64 sum, fixed order)
//   out[t] = count{v in [t-ctx, t+ctx] inside u : c0[v] > thr[u]} >= den * proportion_threshold ? 1 : 0
struct VadArgs {
  const float* feats;           // [total_rows][dim]
  const int32_t* row_off;       // [n_utts + 1]
  int n_utts, total_rows, dim;
  float energy_threshold, energy_mean_scale, proportion_threshold;
  int frames_context;
  float* thr;                   // [n_utts] workspace
  float* out;                   // [total_rows]
};
hipError_t launch_vad_energy(const VadArgs& a, hipStream_t s);

}  // namespace xv
