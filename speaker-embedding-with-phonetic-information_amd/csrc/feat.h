// Host layer of the feature stage (compute-mfcc-feats, compute-vad): options, the window / mel / DCT tables the MFCC kernel
// reads, and the device calls.  Semantics are upstream Kaldi's (feat/feature-window.cc, feat/mel-computations.cc,
// feat/feature-mfcc.cc, ivector/voice-activity-detection.cc) [UPSTREAM, recalled], restated in tests/mfcc_ref.py; parity with
// Kaldi is unpinned.  No CPU path: the device entries throw EngineError without a GPU.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/xvec_hip.h"

namespace xv {

// Kaldi's defaults (MfccOptions / FrameExtractionOptions / MelBanksOptions).
xv_mfcc_options MfccDefaults();
xv_vad_options VadDefaults();

// Derived sizes; throws KioError for options the kernels do not implement or that make no sense.
struct MfccGeometry {
  int frame_len = 0, frame_shift = 0, padded = 0, log2_padded = 0;
};
MfccGeometry MfccGeometryOf(const xv_mfcc_options& o);
// Kaldi's NumFrames (flush = true)
int64_t MfccNumFrames(const xv_mfcc_options& o, int64_t n_samples);

// The tables (exposed for the host tests).
struct MfccTables {
  MfccGeometry g;
  std::vector<float> window, twiddle, mel_w, dct_t, lifter;
  std::vector<int32_t> mel_first, mel_len, mel_woff;
};
MfccTables BuildMfccTables(const xv_mfcc_options& o);

// FNV-1a of the utterance key: what keys the dither generator (the same key gives the same noise in any job).
uint64_t UttSeed(const char* key);

// One device, one set of options: tables uploaded once, buffers reused between batches.
class MfccComputer {
 public:
  MfccComputer(int device, const xv_mfcc_options& o);
  ~MfccComputer();
  MfccComputer(const MfccComputer&) = delete;
  MfccComputer& operator=(const MfccComputer&) = delete;
  // samples: float or int16 (is_i16), packed; sample_off [n_utts + 1]; seeds [n_utts] (may be null when dither == 0).
  // row_off [n_utts + 1] is filled; out is resized to row_off[n_utts] * num_ceps.  device_ms (optional): kernel time.
  void Compute(const void* samples, bool is_i16, const int64_t* sample_off, int n_utts, const uint64_t* seeds,
               std::vector<float>* out, int32_t* row_off, float* device_ms = nullptr);
  const xv_mfcc_options& options() const { return o_; }

 private:
  struct Impl;
  Impl* p_;
  xv_mfcc_options o_;
};

// Kaldi's ComputeVadEnergy on a ragged batch (feats [row_off[n_utts]][dim], out [row_off[n_utts]]).
void VadEnergy(int device, const xv_vad_options& o, const float* feats, const int32_t* row_off, int n_utts, int dim, float* out);

// ---- command-line options (the tools; --config files are read by cli.h)
// Applies one option; returns false for a name this option set does not know; throws KioError for a bad value and for
// options that are refused (they would change the numbers and are not built).
struct MfccToolOptions {
  xv_mfcc_options mfcc;
  int channel = -1;
  float min_duration = 0.f;
  bool subtract_mean = false;
  int verbose = 0;
  int device = -1;
};
bool SetMfccOption(const std::string& name, const std::string& value, MfccToolOptions* o);
bool SetVadOption(const std::string& name, const std::string& value, xv_vad_options* o);

}  // namespace xv
