// Host layer of the augmentation stage (wav-reverberate, stage 2 of egs/sre/v2/run_sre10.sh:92-159): options, the plan of a
// ragged batch and the device calls.  Semantics are upstream Kaldi's (featbin/wav-reverberate.cc, feat/signal.cc,
// feat/wave-reader.cc) [UPSTREAM, recalled], restated in tests/reverb_ref.py; parity with Kaldi is unpinned.  For one utterance:
//   1. input = the chosen channel as float (int16 values, not scaled); power_before = sum(input^2) / len.
//   2. with a RIR (scaled by 1/32768): the signal becomes the linear convolution, length len + rir_len - 1; early_energy is the
//      mean square, over that length, of the convolution with the RIR's slice [peak - 0.001 rate, peak + 0.05 rate) (peak = first
//      maximum of the signed values).  Without a RIR early_energy = power_before.
//   3. additive signal i is scaled by sqrt(10^(-snr_i / 10) * early_energy / its own mean square) and added once at sample
//      int(start_i * rate), cut at the signal's end.
//   4. power_after = mean square of the result; the final factor is --volume if > 0, else sqrt(power_before / power_after)
//      with --normalize-output, else 1.
//   5. output length: int(rate * duration) if duration > 0, else len with --shift-output, else len + rir_len - 1.  Not longer
//      than the input: out[i] = signal[i + shift] (shift = the RIR's peak with --shift-output, else 0); longer: the signal
//      repeated from its start, without shift.
//   6. 16-bit samples: truncated toward zero, saturated.
// No CPU path: Reverberate throws EngineError without a GPU.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/xvec_hip.h"

namespace xv {

xv_reverb_options ReverbDefaults();

// Point 5's length for an input of n samples and a RIR of rir_len taps (0: none).
int64_t ReverbOutputLength(const xv_reverb_options& o, float rate, int64_t n, int64_t rir_len);

// A ragged batch.  samples: float or int16, utterance u = [sample_off[u], sample_off[u + 1]).  rirs / noises: fp32 in the
// 16-bit range as read from their files, ragged by rir_off / noise_off.  utt_rir[u]: index of the utterance's RIR or -1 (the
// array may be null: no RIR anywhere).  Utterance u's additive signals are entries [utt_add_off[u], utt_add_off[u + 1]) of
// add_noise (index into the noises) / add_snr (dB) / add_start (seconds); utt_add_off may be null: none.
struct ReverbBatch {
  float rate = 0.f;
  const void* samples = nullptr;
  bool is_i16 = false;
  const int64_t* sample_off = nullptr;
  int n_utts = 0;
  const float* rirs = nullptr;
  const int64_t* rir_off = nullptr;
  int n_rirs = 0;
  const int32_t* utt_rir = nullptr;
  const float* noises = nullptr;
  const int64_t* noise_off = nullptr;
  int n_noises = 0;
  const int32_t* utt_add_off = nullptr;
  const int32_t* add_noise = nullptr;
  const float* add_snr = nullptr;
  const float* add_start = nullptr;
};

// out_off [n_utts + 1] is filled (ReverbOutputLength of each utterance, cumulated); out_f32 receives out_off[n_utts] floats
// (before quantisation); out_i16 (may be null) the 16-bit samples; clipped (may be null) [n_utts] how many were saturated.
// device_ms (optional): time of the kernels.  Throws KioError for bad arguments, EngineError for the device.
void Reverberate(int device, const xv_reverb_options& o, const ReverbBatch& b, int64_t* out_off, float* out_f32, int16_t* out_i16,
                 int64_t* clipped, float* device_ms = nullptr);

}  // namespace xv
