// What select-voiced-frames makes of one utterance: its VAD decisions, or which of the tool's three warnings applies.  The one
// place that knows the checks and the texts; callers log, count and Forget() in their own way (the calibration sample skips
// silently, the table loop's consumers share one reader behind a lock, the fused reader of nnet3-compute counts per tool).
#pragma once
#include <string>
#include <vector>

#include "kio.h"

namespace xv {

struct VadVerdict {
  enum Kind { kOk, kNoEntry, kWrongLength, kNoneVoiced } kind = kOk;
  const std::vector<float>* decisions = nullptr;   // every kind but kNoEntry; stays valid until the key is forgotten
  int kept = 0;                                    // kOk: frames judged as voiced
  bool ok() const { return kind == kOk; }
  // the warning of the tool, for what is not kOk
  std::string Warning(const std::string& key, int rows) const {
    if (kind == kNoEntry) return "No VAD input found for utterance " + key;
    if (kind == kNoneVoiced) return "No features were judged as voiced for utterance " + key;
    return "Mismatch in number of frames " + std::to_string(rows) + " for features and VAD " + std::to_string(decisions->size()) +
           ", for utterance " + key;
  }
};

// An utterance without rows and with an empty entry passes (kept = 0): the extractor reports it in its own words.
inline VadVerdict JudgeVad(RandomAccessVectorReader* vad, const std::string& key, int rows) {
  VadVerdict r;
  if (!vad->HasKey(key)) {
    r.kind = VadVerdict::kNoEntry;
    return r;
  }
  r.decisions = &vad->Value(key);
  if ((int)r.decisions->size() != rows) {
    r.kind = VadVerdict::kWrongLength;
    return r;
  }
  for (int t = 0; t < rows; ++t) r.kept += (*r.decisions)[t] != 0.f;
  if (rows > 0 && r.kept == 0) r.kind = VadVerdict::kNoneVoiced;
  return r;
}

}  // namespace xv
