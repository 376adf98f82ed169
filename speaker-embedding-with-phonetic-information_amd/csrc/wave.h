// RIFF/WAVE reader on xv::Input: what compute-mfcc-feats reads from wav.scp entries (files and "cmd |" pipes such as
// `sph2pipe -f wav ... |`) and from `ark:` tables of "key RIFF..." objects.  PCM 16-bit, any channel count.
#pragma once
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "kio.h"

namespace xv {

struct WaveData {
  int rate = 0;
  int channels = 0;
  std::vector<int16_t> samples;   // interleaved, frames() * channels
  size_t frames() const { return channels > 0 ? samples.size() / (size_t)channels : 0; }
};

// Reads one WAVE object from the current position of `in`.  Chunks other than "fmt " and "data" are skipped.  A "data" size
// of 0 or 0xFFFFFFFF (what a writer that cannot seek leaves), or one larger than what follows, means "until the end of the
// input"; with until_end_ok == false (objects inside an archive, where another key follows) such a size is an error.
// Throws KioError: not RIFF/WAVE, not 16-bit PCM, truncated header.
void ReadWave(Input& in, WaveData* w, bool until_end_ok = true);

// Kaldi's --channel: -1 = mono as is, otherwise channel 0 (*warn is set to say so); c >= 0 picks channel c (KioError when the
// file has fewer).  out receives one channel.
void SelectChannel(const WaveData& w, int channel, std::vector<int16_t>* out, std::string* warn);

// Writes one channel as RIFF/WAVE, 16-bit PCM, to a wxfilename (file, "-", "| cmd"): each value truncated toward zero and
// saturated to [-32768, 32767] (what Kaldi's WaveData::Write does); returns how many were saturated.  The int16 form writes the
// samples as they are.
int64_t WriteWave(const std::string& wxfilename, int rate, const float* samples, int64_t n);
void WriteWaveI16(const std::string& wxfilename, int rate, const int16_t* samples, int64_t n);

// Sequential reader of a wave table: "scp:" / "scp,p:" of rxfilenames, "ark:" of "key RIFF..." objects.  Per-entry problems
// are reported through *error (non-empty) with the key set and reading continues (scp); a corrupt archive is a KioError.
class SequentialWaveReader {
 public:
  explicit SequentialWaveReader(const std::string& rspecifier);
  bool Next(std::string* key, WaveData* w, std::string* error);
  bool permissive() const { return opts_.permissive; }
  // scp tables: called with each entry's rxfilename before it is opened; true = the hook filled *w or *error itself
  // (compute-mfcc-feats takes wav-reverberate lines over this way, fuse_wav.h)
  void SetEntryHook(std::function<bool(const std::string& rx, WaveData* w, std::string* error)> h) { hook_ = std::move(h); }

 private:
  RspecifierOptions opts_;
  Input in_;
  std::function<bool(const std::string&, WaveData*, std::string*)> hook_;
};

}  // namespace xv
