// ivector-extract / ivector-extractor-copy - drop-in command lines for the last step of the GMM-UBM i-vector baseline
// (egs/sre/v1: sid/extract_ivectors.sh:69).  One executable, dispatching on its name:
//   ivector-extract [--compute-objf-change=true --acoustic-weight=1.0 --max-count=0 --num-threads=N] <model-rxfilename>
//                   <feature-rspecifier> <posterior-rspecifier> <ivector-wspecifier>
//   ivector-extractor-copy [--binary=true] <model-in> <model-out>
// ivector-extract runs on the device (ivex.h) and fails without a GPU (exit 255); the copy is host code and opens no device.
// --num-threads is accepted and ignored; --spk2utt is refused by name, and so is a model with i-vector-dependent weights.
// Features are read ahead in batches, so the recipes' "ark,s,cs:add-deltas ... | select-voiced-frames ... |" is a child pipeline read
// front to back; a posterior table that promised sorted keys (s) is merged against the feature keys, any other is loaded.
// Per utterance, warned, counted and skipped: no posterior, a posterior of another length than the features, no rows, a Q that
// is not positive definite.  Fatal (exit 255): a feature width that is not the model's, a Gaussian index outside the model, no GPU.
#include <math.h>
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "cli.h"
#include "feat_join.h"
#include "ivex.h"
#include "kio.h"

namespace {

struct ExtractOptions {
  bool compute_objf_change = true;
  double acoustic_weight = 1.0, max_count = 0.0;
  int verbose = 0, device = -1;
};

int IvectorExtract(const ExtractOptions& o, const std::vector<std::string>& pos) {
  xv::IvexData data;
  xv::ReadIvexFile(pos[0], &data);
  const int dev = xv::PickDevice(o.device);
  std::unique_ptr<xv::IvexModel> model(xv::IvexCreate(dev, data));
  const int D = data.D, S = data.S;
  xv::FeatBatchWalk walk(pos[1], xv::kBatchFrames, false, xv::FeatProblems::kCount);
  xv::PosteriorLookup posts(pos[2]);
  xv::TableWriter writer(pos[3]);
  long num_done = 0, num_err = 0;
  double tot_t = 0.0, tot_auxf = 0.0;
  std::vector<std::string> keys;
  std::vector<float> feats, post_w, ivectors;
  std::vector<int32_t> off, post_off, post_idx, status;
  std::vector<double> auxf, weighted;
  const long unread = walk.Run([&](const xv::FeatBatchReader::Batch& b) {
    if (b.cols != D)
      throw xv::KioError("Feature dimension mismatch: the features of " + b.keys[0] + " have " + std::to_string(b.cols) + " columns, the model " + std::to_string(D));
    keys.clear();
    feats.clear();
    post_w.clear();
    post_idx.clear();
    weighted.clear();
    off.assign(1, 0);
    post_off.assign(1, 0);
    for (size_t u = 0; u < b.keys.size(); ++u) {
      const int rows = b.row_off[u + 1] - b.row_off[u];
      xv::Posterior p;
      const xv::Joined j = xv::FindFrames(&posts, b.keys[u], rows, &p);
      if (j.outcome == xv::Joined::kNotFound) XWARN("No posteriors for utterance " << b.keys[u]);
      else if (j.outcome != xv::Joined::kOk) XWARN("Size mismatch between posterior " << j.size << " and features " << rows << " for utterance " << b.keys[u]);
      if (j.outcome != xv::Joined::kOk) {
        ++num_err;
        continue;
      }
      const size_t first = post_w.size();
      xv::Append(p, &post_off, &post_idx, &post_w);
      bool clipped = false;
      const float scale = xv::IvexPosteriorScale(post_w.data() + first, post_w.size() - first, o.acoustic_weight, o.max_count, &clipped);
      if (clipped) XLOG("Scaling stats for utterance " << b.keys[u] << " by scale " << scale << " due to --max-count=" << o.max_count);
      double t = 0.0;
      for (size_t i = first; i < post_w.size(); ++i) t += (double)(post_w[i] * scale);
      weighted.push_back(t);
      keys.push_back(b.keys[u]);
      xv::AppendRows(b, u, &feats);
      off.push_back(off.back() + rows);
    }
    if (keys.empty()) return;
    const int n = (int)keys.size();
    ivectors.resize((size_t)n * S);
    status.resize((size_t)n);
    auxf.assign((size_t)n, 0.0);
    xv::IvexOutputs out;
    out.ivectors = ivectors.data();
    out.status = status.data();
    out.auxf_change = o.compute_objf_change ? auxf.data() : nullptr;
    xv::IvexExtract(*model, feats.data(), off.data(), n, post_off.data(), post_idx.data(), post_w.data(), o.acoustic_weight, o.max_count, out);
    for (int u = 0; u < n; ++u) {
      if (status[u] != 0) {
        XWARN("The quadratic term of utterance " << keys[u] << " is not positive definite: no i-vector (skipping utterance)");
        ++num_err;
        continue;
      }
      const float* v = ivectors.data() + (size_t)u * S;
      const double T = weighted[u];
      if (o.compute_objf_change) {
        tot_auxf += auxf[u];
        if (o.verbose >= 2)
          XLOG("Auxf change for utterance " << keys[u] << " was " << (T != 0.0 ? auxf[u] / T : 0.0) << " per frame over " << T << " frames (weighted)");
      }
      if (o.verbose >= 2) {
        double norm = 0.0;
        for (int s = 0; s < S; ++s) norm += (double)v[s] * (double)v[s];
        XLOG("Ivector norm for utterance " << keys[u] << " was " << sqrt(norm));
      }
      tot_t += T;
      writer.WriteVec(keys[u], v, S);
      ++num_done;
    }
  });
  writer.Close();
  XLOG("Done " << num_done << " files, " << unread + num_err << " with errors.  Total (weighted) frames " << tot_t);
  if (o.compute_objf_change)
    XLOG("Overall average objective-function change from estimating ivector was " << (tot_t != 0.0 ? tot_auxf / tot_t : 0.0) << " per frame  over "
                                                                                    << tot_t << " (weighted) frames.");
  return num_done != 0 ? 0 : 1;
}

int ExtractorCopy(bool binary, const std::vector<std::string>& pos) {
  xv::IvexData m;
  xv::ReadIvexFile(pos[0], &m);
  xv::WriteIvexFile(pos[1], binary, m);
  XLOG("Copied the i-vector extractor to " << pos[1]);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  using Pos = std::vector<std::string>;
  bool binary = true;
  ExtractOptions o;
  const std::vector<xv::CliTool> tools = {
      {"ivector-extractor-copy",
       "Copy the i-vector extractor to a different file (possibly changing binary/text format).\n"
       "Usage: ivector-extractor-copy [options] <ivector-extractor-in> <ivector-extractor-out>\nOptions: --binary (true)\n",
       {xv::Bool("binary", &binary)}, 2, 2, [&](const Pos& pos) { return ExtractorCopy(binary, pos); }},
      {"ivector-extract",
       "Extract iVectors for utterances, using a trained iVector extractor, and features and Gaussian-level posteriors.\n"
       "Usage: ivector-extract [options] <model-in> <feature-rspecifier> <posterior-rspecifier> <ivector-wspecifier>\n"
       "e.g.: fgmm-global-gselect-to-post 1.ubm '$feats' 'ark:gunzip -c gselect.1.gz|' ark:- | ivector-extract final.ie '$feats' ark,s,cs:- ark,t:ivectors.1.ark\n"
       "Options: --compute-objf-change (true) --acoustic-weight (1.0) --max-count (0) --num-threads (accepted, ignored) --verbose --device=<gpu>\n"
       "Limits: i-vector dimension <= 1024, feature dimension <= 96.  Not built (refused): --spk2utt, models with i-vector-dependent weights.\n",
       {xv::Ignored("num-threads"), xv::Int("verbose", &o.verbose), xv::Bool("compute-objf-change", &o.compute_objf_change),
        xv::Double("acoustic-weight", &o.acoustic_weight), xv::Double("max-count", &o.max_count), xv::Int("device", &o.device),
        xv::Refused("spk2utt", "--spk2utt is not built: no script of the recipes passes it (they average per speaker with ivector-mean)")},
       4, 4, [&](const Pos& pos) { return IvectorExtract(o, pos); }},
  };
  return xv::ToolsMain(argc, argv, tools, xv::NameRule::kContains, "ivector-extract");
}
