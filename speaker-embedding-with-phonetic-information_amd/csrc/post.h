// The phonetic i-vector path: what logprob-to-post, fgmm-global-acc-stats-post, fgmm-global-init-from-accs and nnet3-info do in
// sid/extract_post_nnet3.sh:85-91 and sid/init_full_ubm_from_nnet3.sh:91-136, where the frame posteriors come from the senone
// network and the UBM has one Gaussian per senone.  A restatement of Kaldi's bin/logprob-to-post.cc, fgmmbin/fgmm-global-acc-stats-post.cc,
// fgmmbin/fgmm-global-init-from-accs.cc and nnet3bin/nnet3-info.cc of early 2018, written from their documented behaviour: as in
// ubm.h, parity with a Kaldi binary is not pinned by any test here.  tests/logprob_post_ref.py is logprob-to-post in numpy;
// tests/ubm_train_ref.py is the accumulation.
//
// logprob-to-post [--min-post=0.01] [--random-prune=true] <logprob-matrix-rspecifier> <posterior-wspecifier>  (device)
//   Per utterance the rows x columns matrix of log-probabilities (a compressed matrix is expanded first) becomes a Posterior with
//   one entry per row; a matrix without rows gives an empty Posterior.  Within a row the columns are ascending.  For column j:
//     a NaN is dropped and counted;  p = expf(x[j]) in fp32;
//     min_post <= 0: keep (j, p), -infinity included (it gives 0);
//     p >= min_post: keep (j, p);
//     else with --random-prune and p / min_post >= u: keep (j, min_post);  else drop.
//   A row may come out empty and is still written; nothing is renormalised.
//   u is not a stream.  It is a function of (utterance key, row index within the utterance as this tool reads it, column) through
//   the counter-based generator of the MFCC dither (counter_rng.h): seed = FNV-1a of the key, the counter (row << 32) | column,
//   u = ((r >> 40) + 1) / 2^24 in (0, 1].  A frame's posterior is therefore the same bits alone, in any batch and in any job
//   split.  Kaldi draws from rand() instead (RandPrune), one more reason parity is not pinned; what is kept is the expectation,
//   E[weight] = p for a pruned entry.
//   Log: "Done N utterances", "F frames in, P pairs out, P / F pairs per frame"; a warning with the number of NaN values.
//   Limits: the number of columns is limited by memory alone; a launch takes rows * columns < 2^31 (its pairs fit an int32), which
//   the frame budget of a launch is cut to.
// fgmm-global-acc-stats-post [--binary=true] [--update-flags=mvw] <posterior-rspecifier> <num-components> <feats-rspecifier> <stats-out>  (device)
//   The posterior of every feature key comes through PosteriorLookup (a merge when the keys are sorted, loaded otherwise).  No
//   posterior for a key: warn, count an error, skip.  A posterior whose length is not the number of rows: the same.  An index
//   outside [0, num-components) is an error that names it.  The accepted frames with their (Gaussian, weight) pairs are
//   concatenated, cut into blocks of exactly kFgmmAccFrameBlock frames (an utterance may straddle a block) and go through
//   FgmmAccAdd, one call per block, the last one possibly short: the statistics are a function of the ordered sequence of
//   (frame, pairs) alone, exactly as fgmm-global-acc-stats'.  (kFgmmAccFrameBlock is kept: with one Gaussian per senone a block of
//   16384 frames at about 10 pairs per frame leaves buckets of some tens of pairs, which FgmmAccAdd's work items, one per started
//   chunk of a bucket, take as they are; nothing was measured that asks for another size.)  A Gaussian named twice in one frame adds
//   twice, as FgmmAccAdd does; logprob-to-post never produces that.  A pair whose weight is 0 adds nothing.
//   The output is the accumulator file of gmm_train.h, which fgmm-global-sum-accs reads.
//   Log: "Done N files; M with errors."  Exit status 0 iff N > 0.
// fgmm-global-init-from-accs [--binary=true] [fgmm-global-est's options] <stats-in> <num-components> <model-out>  (host, fp64)
//   The accumulator must carry m, v and w and have <num-components> Gaussians.  For every Gaussian g:
//     weight = occ_g / sum occ;  mu = mean_g / occ_g;  C = cov_g / occ_g - mu mu';  the model stores C^-1 and C^-1 mu (plda.h's
//     InvertSymmetric; there is no eigenvalue flooring here, Kaldi's tool does none); the gconsts are ComputeGconsts'.
//   A Gaussian whose occupancy is 0, whose C cannot be inverted or whose gconst is not finite is bad.  With
//   --remove-low-count-gaussians (default true) it is removed with a warning and the weights become occ_g / (sum of occ over the
//   Gaussians kept); without, it is an error that names the Gaussian.  Of fgmm-global-est's options only that one has a meaning
//   here; the others are accepted and ignored, as in Kaldi.  Log: the number of bad gconsts, "Written model to <out>".
// nnet3-info <raw-nnet-rxfilename>  (host)
//   Reads a raw network (nnet3_raw.h; "nnet3-am-copy --raw=true final.mdl - |" is an rxfilename, and so are its words given one by
//   one, which is what the unquoted $nnet_raw of sid/init_full_ubm_from_nnet3.sh:91 makes of it) and prints to stdout:
//   "num-parameters: N" (the linear and bias parameters), one "input-node name=... dim=..." line per input, one "component-node
//   name=... component=... input=... input-dim=... output-dim=..." line per component node, one "output-node name=... input=...
//   dim=... objective=linear" line per output and one "component name=... type=..." line per component; then, as "# " lines, the
//   lowered program of every output the extractor can run (xv_model_describe).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "gmm_train.h"
#include "kio.h"

namespace xv {

// rows per launch when the caller names no budget: what keeps a launch's input within kPostLaunchBytes, at least 1.  The size is
// chosen for the grid, one wave per row: at 6000 columns, 2048 rows (49 MB) leave the chip short of waves and ran at 3.7 to 5.3 times
// the floor of profiles/logprob_post_bench.md, 8192 rows (197 MB) at 1.5 to 2.5 times, 16384 rows at 1.3 to 2.3 times.  The second
// pass gains little from the memory-side cache (4 % at 197 MB, which it holds), so nothing is given up by launches beyond it.
constexpr size_t kPostLaunchBytes = (size_t)256 << 20;
int64_t LogprobPostDefaultBudget(int cols);

struct LogprobPostResult {
  std::vector<int64_t> off;   // [rows + 1]: row r has the pairs off[r] .. off[r + 1]
  std::vector<int32_t> idx;   // ascending within a row
  std::vector<float> w;
  int64_t num_nan = 0;
  float ms[3] = {0.f, 0.f, 0.f};   // {count, scan, write}, summed over the launches; only with timed
};
// logprobs [row_off[n_utts]][cols] packed; utt_seed [n_utts] (UttSeed of the keys; may be null without pruning).  frame_budget:
// rows per launch, <= 0 for the default; whatever it is, it is cut to rows * cols < 2^31.  Blocking.
void LogprobToPost(int device, const float* logprobs, const int32_t* row_off, int n_utts, int cols, const uint64_t* utt_seed, float min_post,
                   bool random_prune, int64_t frame_budget, bool timed, LogprobPostResult* out);

// ms of one device-to-device copy of `bytes` bytes, the best of reps after one that warms up (the floor tools/bench_post.py quotes)
float DeviceCopyMs(int device, size_t bytes, int reps);

// fgmm-global-init-from-accs.  removed: ascending; bad_gconsts: how many of the bad Gaussians were bad by their gconst alone.
struct FgmmInitResult {
  std::vector<int32_t> removed;
  int bad_gconsts = 0;
  std::vector<std::string> warnings;
  std::vector<double> inv_covars64;   // [G as given][D (D + 1) / 2]: C^-1 before it is rounded to float; zeros for a bad Gaussian
};
void FgmmInitFromAccs(const FgmmAccs& accs, bool remove_low_count_gaussians, FullGmmData* model, FgmmInitResult* res);

}  // namespace xv
