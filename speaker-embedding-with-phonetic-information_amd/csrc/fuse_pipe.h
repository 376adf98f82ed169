// The feature pipeline every extraction script of the reference builds, recognised as text.
//
// egs/sre/v2/sid/nnet3/xvector/extract_xvectors_new.sh:79 (and extract_xvectors.sh:73, extract_output_new.sh:75, the
// nnet3_cvector copies, extract_cvectors_with_am.sh:92, extract_cvectors_with_embedding.sh:81, extract_log_post.sh:68-70) hand
// the binary its features as ONE rspecifier string:
//   ark:apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 scp:$sdata/feats.scp ark:- |
//       select-voiced-frames ark:- scp,s,cs:$sdata/vad.scp ark:- |
// Run as written, that is two CPU tools and two pipes per job in front of a GPU that could take fifty times what they deliver.
// The tool therefore reads the string before it starts the commands: when it is EXACTLY this pipeline - these two programs, only
// the options the device front-end implements with the values it implements them for, "ark:-" in the plumbing positions - the job
// reads the inner feature table itself and runs sliding CMN + voiced-frame selection on the device (engine.h FrontEndJob; the
// stored features, compressed as make_mfcc.sh leaves them, go up as they are).  Anything else - another option, another
// program, a third stage, quotes, redirections - is not this pipeline and is run as a command, as before.  nnet3-compute, which
// extract_log_post.sh:77-84 hands the same string, does the same in front of its frame-level forward pass.
//
// The acoustic-model scripts (sid/nnet3_cvector/am/extract_bn.sh:59, extract_am_embedding.sh:67,
// steps/nnet3/make_bottleneck_features_new.sh) hand nnet3-compute the PER-SPEAKER normalisation instead:
//   ark,s,cs:apply-cmvn $cmvn_opts --utt2spk=ark:$sdata/JOB/utt2spk scp:$sdata/JOB/cmvn.scp scp:$sdata/JOB/feats.scp ark:- |
// - a child process that opens the GPU itself, expands the stored features on a core and writes four bytes per value into a
// pipe.  RecognizeCmvnPipeline reads that string the same way: apply-cmvn by base name, only --norm-means, --norm-vars and
// --utt2spk=ark:<file>, the statistics as a table in a file or as the file of one global matrix, the features as a table in a
// file, "ark:-" as the output, and at most the select-voiced-frames stage behind it.  nnet3-compute then reads the tables
// itself, computes every speaker's norm once and runs the affine map behind the row selection as one kernel in front of the
// network (cmvn_kernels.h cmvn_apply_select).  --skip-dims, --reverse, --config, --verbose, a pipe or "-" where a table is
// expected: run as commands.
#pragma once
#include <string>

namespace xv {

struct FusedPipeline {
  std::string feats_rspecifier;   // what apply-cmvn-sliding reads: "scp:..." or "ark:..."
  std::string vad_rspecifier;     // what select-voiced-frames takes its decisions from; empty: no selection stage
  int cmn_window = 600;           // apply-cmvn-sliding's defaults (sliding-window-cmn options)
  int min_cmn_window = 100;
  bool center = false;
};

// true: `rspecifier` is the pipeline above and *out describes it.  false: it is something else (out untouched).
bool RecognizeFeaturePipeline(const std::string& rspecifier, FusedPipeline* out);

struct FusedCmvnPipeline {
  std::string stats_rxfilename;     // the first argument of apply-cmvn as typed: a table ("scp:..." / "ark:...") or a file
  bool stats_is_table = true;       // false: the file of ONE statistics matrix, applied to every utterance
  std::string feats_rspecifier;     // "scp:..." or "ark:..."
  std::string vad_rspecifier;       // empty: no selection stage
  std::string utt2spk_rspecifier;   // "ark:<file>"; empty: the statistics are looked up by utterance key
  bool norm_means = true;           // apply-cmvn's defaults
  bool norm_vars = false;
};

// The same for the per-speaker pipeline.  The two recognisers accept disjoint sets of strings (they name different programs).
bool RecognizeCmvnPipeline(const std::string& rspecifier, FusedCmvnPipeline* out);
// "name=value" lines: stats, stats-is-table, feats, vad, utt2spk, norm-means, norm-vars (what the C ABI returns)
std::string DescribeFusedCmvn(const FusedCmvnPipeline& p);

}  // namespace xv
