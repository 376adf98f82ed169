// Shared by the tools that join the utterances of a feature table with a Gaussian selection or a posterior by key and pack what
// survived into the flat arrays of a device call (ubm_tools_main.cc, gmm_classify_tools_main.cc, gmm_acc_tool.h,
// post_tools_main.cc, ivex_tools_main.cc, ivex_train_tools_main.cc).  Each tool family follows the wording of another Kaldi
// program, so FindFrames / FindGselect only say what they found and the caller words the warning.  Host only.
#pragma once
#include <stdint.h>

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "cli.h"
#include "feat_batch.h"
#include "keyed_lookup.h"
#include "kio.h"

namespace xv {

struct Joined {
  enum Outcome { kOk, kNotFound, kWrongSize, kRagged } outcome;
  size_t size;   // kOk, kWrongSize, kRagged: the frames the table has for the key
  int width;     // FindGselect, kOk: the indices per frame
};

// The value of `key`, which has to have one element per frame.
template <class T>
Joined FindFrames(KeyedLookup<T>* table, const std::string& key, int rows, T* value) {
  if (!table->Find(key, value)) return Joined{Joined::kNotFound, 0, 0};
  return Joined{(int)value->size() == rows ? Joined::kOk : Joined::kWrongSize, value->size(), 0};
}

// The same for a Gaussian selection, which also has to have one width >= 1 on every frame (rows >= 1).
inline Joined FindGselect(GselectLookup* table, const std::string& key, int rows, IntVecVec* sel) {
  Joined j = FindFrames(table, key, rows, sel);
  if (j.outcome != Joined::kOk) return j;
  const size_t width = (*sel)[0].size();
  bool same = width >= 1;
  for (const auto& l : *sel) same = same && l.size() == width;
  j.outcome = same ? Joined::kOk : Joined::kRagged;
  j.width = same ? (int)width : 0;
  return j;
}

// The rows of utterance u of a batch of floats, appended to *feats.
inline void AppendRows(const FeatBatchReader::Batch& b, size_t u, std::vector<float>* feats) {
  feats->insert(feats->end(), b.feats.begin() + (size_t)b.row_off[u] * b.cols, b.feats.begin() + (size_t)b.row_off[u + 1] * b.cols);
}

inline void Append(const IntVecVec& sel, std::vector<int32_t>* gs) {
  for (const auto& l : sel) gs->insert(gs->end(), l.begin(), l.end());
}

// A posterior as the device calls take it: the pairs of all frames back to back, frame t of the pending ones at
// [post_off[t], post_off[t + 1]).  post_off starts as {0}.
inline void Append(const Posterior& post, std::vector<int32_t>* post_off, std::vector<int32_t>* post_idx, std::vector<float>* post_w) {
  for (const auto& frame : post) {
    for (const auto& e : frame) {
      post_idx->push_back(e.first);
      post_w->push_back(e.second);
    }
    if (post_idx->size() > (size_t)INT32_MAX) throw KioError("more than 2^31 posterior pairs are pending in one block of frames");
    post_off->push_back((int32_t)post_idx->size());
  }
}

// The utterances of a feature table that have a usable selection, in groups of one selection width: what the device tools that
// score selected Gaussians walk.
struct GselectGroup {
  std::vector<std::string> keys;
  std::vector<float> feats;
  std::vector<int32_t> off, gs;   // off: [keys.size() + 1] rows; gs: [rows][n]
  int n = 0;
  void Clear() {
    keys.clear();
    feats.clear();
    gs.clear();
    off.assign(1, 0);
  }
};

// The walk over those groups; the constructor opens the two tables.  Run calls `flush` for every group, a batch of the feature
// table at a time, and returns the number of utterances skipped with a warning.  gselect_rspecifier empty: every utterance gets
// the identity selection 0 .. num_gauss - 1.
class GselectGroupWalk {
 public:
  GselectGroupWalk(int dim, int num_gauss, const std::string& feats_rspecifier, const std::string& gselect_rspecifier,
                   int64_t batch_frames = kBatchFrames)
      : dim_(dim), num_gauss_(num_gauss), feats_(feats_rspecifier, batch_frames, false, FeatProblems::kCount) {
    if (!gselect_rspecifier.empty()) gselect_.reset(new GselectLookup(gselect_rspecifier));
  }
  long Run(const std::function<void(const GselectGroup&)>& flush);

 private:
  const int dim_, num_gauss_;
  FeatBatchWalk feats_;
  std::unique_ptr<GselectLookup> gselect_;
};

inline long GselectGroupWalk::Run(const std::function<void(const GselectGroup&)>& flush) {
  long num_err = 0;
  GselectGroup g;
  const long unread = feats_.Run([&](const FeatBatchReader::Batch& b) {
    g.Clear();
    g.n = 0;
    for (size_t u = 0; u < b.keys.size(); ++u) {
      const int rows = b.row_off[u + 1] - b.row_off[u];
      if (b.cols != dim_) {
        XWARN("Dimension mismatch for utterance " << b.keys[u] << ": the features have " << b.cols << " columns, the model " << dim_);
        ++num_err;
        continue;
      }
      int width = num_gauss_;
      IntVecVec sel;
      if (gselect_) {
        const Joined j = FindGselect(gselect_.get(), b.keys[u], rows, &sel);
        if (j.outcome == Joined::kNotFound)
          XWARN("No Gaussian-selection info available for utterance " << b.keys[u] << " (skipping utterance)");
        else if (j.outcome == Joined::kWrongSize)
          XWARN("Mismatch in number of frames " << rows << " for features and Gaussian selection " << j.size << ", for utterance " << b.keys[u]);
        else if (j.outcome == Joined::kRagged)
          XWARN("The Gaussian selection of utterance " << b.keys[u] << " does not have one length for every frame (skipping utterance)");
        if (j.outcome != Joined::kOk) {
          ++num_err;
          continue;
        }
        width = j.width;
      }
      if (width != g.n && !g.keys.empty()) {
        flush(g);
        g.Clear();
      }
      g.n = width;
      g.keys.push_back(b.keys[u]);
      AppendRows(b, u, &g.feats);
      if (gselect_) {
        Append(sel, &g.gs);
      } else {
        for (int t = 0; t < rows; ++t)
          for (int k = 0; k < width; ++k) g.gs.push_back(k);
      }
      g.off.push_back(g.off.back() + rows);
    }
    if (!g.keys.empty()) flush(g);
  });
  return unread + num_err;
}

}  // namespace xv
