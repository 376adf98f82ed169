// Shared by fgmm-global-acc-stats / fgmm-global-sum-accs (ubm_train_tools_main.cc) and gmm-global-acc-stats / gmm-global-sum-accs
// (dubm_train_tools_main.cc): the options, the reader loop that cuts the accepted frames into blocks, and the sum of stats files.
// Semantics: ubm_train.h.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "cli.h"
#include "feat_join.h"
#include "gmm_train.h"
#include "kio.h"
#include "ubm_kernels.h"

namespace xv {

struct GmmAccOptions {
  bool binary = true;
  std::string update_flags = "mvw", gselect;
  int device = -1, verbose = 0;
};

// Appends the options of the two *-global-acc-stats tools but --weights, whose refusal each words itself.
inline void AppendGmmAccOptions(GmmAccOptions* o, std::vector<CliOption>* to) {
  to->insert(to->end(), {Int("verbose", &o->verbose), Bool("binary", &o->binary), String("update-flags", &o->update_flags),
                         String("gselect", &o->gselect), Int("device", &o->device)});
}

// pos: <model-in> <feature-rspecifier> <stats-out>, the model already read and on the device.  host: initialised with the kind,
// the model's shape and the flags.  accumulate(feats, rows, gselect, n, logsum): one block of at most frame_block frames through
// the device, logsum [rows] coming back.  get(): the device's sums into *host, once at the end.  Returns the exit status.
template <class Accumulate, class Get>
int GmmAccStats(const GmmAccOptions& o, const std::vector<std::string>& pos, GmmAccs* host, int frame_block, Accumulate accumulate, Get get) {
  // (the accumulate calls do not depend on the frames read ahead; a matrix without rows is skipped, not an error)
  FeatBatchWalk walk(pos[1], kBatchFrames, false, FeatProblems::kCountUnreadable);
  GselectLookup gselect(o.gselect);
  long num_done = 0, num_err = 0;
  double tot_like = 0.0;
  int64_t tot_t = 0;
  // the stream of accepted frames, cut into blocks of exactly frame_block: what is pending is less than one block
  std::vector<float> feats, logsum;
  std::vector<int32_t> gs;
  int n = 0;
  const int D = host->dim;
  size_t head = 0;   // frames at the front of the pending buffers that have been through the device
  auto block = [&](size_t rows) {   // the next `rows` pending frames
    logsum.resize(rows);
    accumulate(feats.data() + head * D, (int64_t)rows, gs.data() + head * n, n, logsum.data());
    for (size_t t = 0; t < rows; ++t) tot_like += logsum[t];
    tot_t += (int64_t)rows;
    head += rows;
  };
  const long unread = walk.Run([&](const FeatBatchReader::Batch& b) {
    for (size_t u = 0; u < b.keys.size(); ++u) {
      const int rows = b.row_off[u + 1] - b.row_off[u];
      if (b.cols != D) {
        XWARN("Dimension mismatch for utterance " << b.keys[u] << ": the features have " << b.cols << " columns, the model " << D);
        ++num_err;
        continue;
      }
      IntVecVec sel;
      const Joined j = FindGselect(&gselect, b.keys[u], rows, &sel);
      const bool usable = j.outcome == Joined::kOk && (n == 0 || j.width == n);   // one width for the whole run
      if (j.outcome == Joined::kNotFound)
        XWARN("No gselect information for utterance " << b.keys[u]);
      else if (j.outcome == Joined::kWrongSize)
        XWARN("gselect information for utterance " << b.keys[u] << " has wrong size " << j.size << " vs. " << rows);
      else if (!usable)
        XWARN("The Gaussian selection of utterance " << b.keys[u] << " does not have " << (n ? "the " + std::to_string(n) + " indices per frame of the utterances before it" : "one length for every frame")
                                                    << " (skipping utterance)");
      if (!usable) {
        ++num_err;
        continue;
      }
      if (j.width > kUbmMaxSelect)
        throw KioError("the Gaussian selection has " + std::to_string(j.width) + " indices per frame; the device kernels take at most " + std::to_string(kUbmMaxSelect));
      n = j.width;
      AppendRows(b, u, &feats);
      Append(sel, &gs);
      while (feats.size() / D - head >= (size_t)frame_block) block((size_t)frame_block);
      if (head) {   // drop what was consumed, once per utterance that filled a block
        feats.erase(feats.begin(), feats.begin() + head * D);
        gs.erase(gs.begin(), gs.begin() + head * n);
        head = 0;
      }
      ++num_done;
      if (o.verbose >= 1 && num_done % 10 == 0)   // over the frames that have been through the device: whole blocks
        XLOG("Avg like per frame so far is " << (tot_t ? tot_like / (double)tot_t : 0.0));
    }
  });
  if (!feats.empty()) block(feats.size() / D);
  XLOG("Done " << num_done << " files; " << unread + num_err << " with errors.");
  XLOG("Overall likelihood per frame = " << (tot_t ? tot_like / (double)tot_t : 0.0) << " over " << tot_t << " (weighted) frames.");
  get();
  WriteGmmAccsFile(pos[2], o.binary, *host);
  XLOG("Written accs to " << pos[2]);
  return num_done != 0 ? 0 : 1;
}

// pos: <stats-out> <stats-in1> ...
inline int GmmSumAccs(bool full, bool binary, const std::vector<std::string>& pos) {
  GmmAccs sum;
  sum.full = full;
  for (size_t i = 1; i < pos.size(); ++i) ReadGmmAccsFile(pos[i], i > 1, &sum);
  WriteGmmAccsFile(pos[0], binary, sum);
  XLOG("Summed " << pos.size() - 1 << " stats");
  XLOG("Written stats to " << pos[0]);
  return 0;
}

}  // namespace xv
