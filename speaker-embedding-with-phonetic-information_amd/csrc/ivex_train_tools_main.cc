// ivector-extractor-init / -acc-stats / -sum-accs / -est - drop-in command lines for i-vector extractor training
// (egs/sre/v1: sid/train_ivector_extractor.sh:97-160).  One executable, dispatching on its exact base name:
//   ivector-extractor-init [--binary=true] [--ivector-dim=400] [--use-weights=false] [--seed=0] <fgmm-in> <ie-out>
//   ivector-extractor-acc-stats [--binary=true] [--update-variances=true] [--compute-auxf=true] [--verbose=N] [--device=N]
//                               <ie-in> <feature-rspecifier> <posterior-rspecifier> <stats-out>
//   ivector-extractor-sum-accs [--binary=true] [--parallel=false] <stats-in1> ... <stats-inN> <stats-out>
//   ivector-extractor-est [--binary=true] [--num-threads=1] [--variance-floor-factor=0.1] [--gaussian-min-count=100]
//                         [--diagonalize=true] <ie-in> <stats-in> <ie-out>
// Semantics: ivex_train.h.  Only ivector-extractor-acc-stats opens a device, and it fails without a GPU (exit 255).  --num-threads,
// --num-samples-for-weights and --cache-size of acc-stats are accepted and ignored.  --seed is an option of ours (upstream draws from
// rand()).  --use-weights=true is refused by name.  --parallel=true is accepted; the inputs are still opened and read one after
// another, so one sum-accs never has more than one child pipeline, and with it one device process, alive.
#include <math.h>
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "cli.h"
#include "feat_join.h"
#include "ivex.h"
#include "ivex_train.h"
#include "kio.h"

namespace {

struct AccOptions {
  bool binary = true, update_variances = true, compute_auxf = true;
  int verbose = 0, device = -1;
};

int AccStats(const AccOptions& o, const std::vector<std::string>& pos) {
  xv::IvexData data;
  xv::ReadIvexFile(pos[0], &data);
  const int dev = xv::PickDevice(o.device);
  std::unique_ptr<xv::IvexModel> model(xv::IvexCreate(dev, data));
  std::unique_ptr<xv::IvexAccumulator> acc(xv::IvexAccCreate(model.get(), o.update_variances, o.compute_auxf));
  const int D = data.D;
  xv::FeatBatchWalk walk(pos[1], xv::kBatchFrames, false, xv::FeatProblems::kCount);
  xv::PosteriorLookup posts(pos[2]);
  long num_done = 0, num_err = 0;
  std::vector<std::string> keys;
  std::vector<float> feats, post_w;
  std::vector<int32_t> off, post_off, post_idx, status;
  const long unread = walk.Run([&](const xv::FeatBatchReader::Batch& b) {
    if (b.cols != D)
      throw xv::KioError("Feature dimension mismatch: the features of " + b.keys[0] + " have " + std::to_string(b.cols) + " columns, the model " + std::to_string(D));
    keys.clear();
    feats.clear();
    post_w.clear();
    post_idx.clear();
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
      xv::Append(p, &post_off, &post_idx, &post_w);
      keys.push_back(b.keys[u]);
      xv::AppendRows(b, u, &feats);
      off.push_back(off.back() + rows);
    }
    if (keys.empty()) return;
    const int n = (int)keys.size();
    status.assign((size_t)n, 0);
    xv::IvexAccAdd(acc.get(), feats.data(), off.data(), n, post_off.data(), post_idx.data(), post_w.data(), status.data());
    for (int u = 0; u < n; ++u) {
      if (status[u] != 0) {
        XWARN("The quadratic term of utterance " << keys[u] << " is not positive definite: no statistics (skipping utterance)");
        ++num_err;
      } else {
        ++num_done;
      }
    }
  });
  xv::IvexStats st;
  xv::IvexAccGet(acc.get(), &st);
  XLOG("Done " << num_done << " files, " << unread + num_err << " with errors.");
  if (o.compute_auxf)
    XLOG("Overall auxf/frame on training data was " << (st.frames != 0.0 ? st.auxf / st.frames : 0.0) << " per frame over " << st.frames << " frames.");
  xv::WriteIvexStatsFile(pos[3], o.binary, st);
  XLOG("Wrote stats to " << pos[3]);
  return num_done != 0 ? 0 : 1;
}

int Init(bool binary, int ivector_dim, uint64_t seed, const std::vector<std::string>& pos) {
  xv::FullGmmData ubm;
  {
    xv::Input in;
    in.Open(pos[0]);
    const bool b = xv::ReadBinaryHeader(in);
    xv::ReadFullGmm(in, b, &ubm);
    if (in.Close() != 0) throw xv::KioError("the command of " + pos[0] + " failed");
  }
  xv::IvexData m;
  xv::IvexInit(ubm, ivector_dim, seed, &m);
  xv::WriteIvexFile(pos[1], binary, m);
  XLOG("Initialized iVector extractor with iVector dimension " << ivector_dim << " and wrote it to " << pos[1]);
  return 0;
}

int SumAccs(bool binary, const std::vector<std::string>& pos) {
  xv::IvexStats sum, one;
  for (size_t i = 0; i + 1 < pos.size(); ++i) {   // one after another: never two child pipelines at a time
    XLOG("Reading stats from " << pos[i]);
    xv::ReadIvexStatsFile(pos[i], i == 0 ? &sum : &one);
    if (i > 0) sum.Add(one);
  }
  xv::WriteIvexStatsFile(pos.back(), binary, sum);
  XLOG("Wrote summed stats to " << pos.back());
  return 0;
}

int Est(bool binary, const xv::IvexEstOptions& o, const std::vector<std::string>& pos) {
  xv::IvexData m;
  xv::ReadIvexFile(pos[0], &m);
  xv::IvexStats st;
  xv::ReadIvexStatsFile(pos[1], &st);
  xv::IvexEstResult r;
  xv::IvexEst(st, o, &m, &r);
  for (const std::string& w : r.warnings) XWARN(w);
  XLOG("Updated " << r.gauss_updated << " projections, skipped " << r.gauss_skipped << "; floored " << r.eig_floored << " eigenvalues of the quadratic statistics.");
  XLOG("Overall objective function improvement for M (mean projections) was " << r.impr_proj << " per frame.");
  if (st.has_variances) {
    XLOG(r.var_floored << " variances floored in " << r.var_floored_gauss << " Gaussians");
    XLOG("Overall objective function improvement for variances was " << r.impr_var << " per frame.");
  }
  if (r.prior_floored) XLOG("Floored " << r.prior_floored << " eigenvalues of the covariance of the iVectors.");
  XLOG("Overall auxf improvement from prior is " << r.impr_prior << " per frame; the new prior offset is " << m.prior_offset);
  XLOG("Overall objective-function improvement per frame was " << r.impr_proj + r.impr_var + r.impr_prior);
  xv::WriteIvexFile(pos[2], binary, m);
  XLOG("Wrote iVector extractor to " << pos[2]);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  using Pos = std::vector<std::string>;
  bool binary = true;
  int ivector_dim = 400;
  uint64_t seed = 0;
  xv::IvexEstOptions e;
  AccOptions o;
  const std::vector<xv::CliTool> tools = {
      {"ivector-extractor-init",
       "Initialize an iVector extractor from a full-covariance UBM.\n"
       "Usage: ivector-extractor-init [options] <fgmm-in> <ivector-extractor-out>\n"
       "Options: --binary (true) --ivector-dim (400) --seed (0: the generator of the projections; not an upstream option)\n"
       "Limits: i-vector dimension <= 1024, feature dimension <= 96.  Not built (refused): --use-weights=true.\n",
       {xv::Bool("binary", &binary), xv::Int("ivector-dim", &ivector_dim),
        xv::Custom("seed", [&](const std::string& n, const std::string& val) {   // an int, negative ones included
          seed = (uint64_t)(int64_t)xv::ToInt(n, val);
          return true;
        }),
        xv::RefusedIfTrue("use-weights", "--use-weights=true is not built: no recipe trains a model with i-vector-dependent weights, and ivector-extract refuses one")},
       2, 2, [&](const Pos& pos) { return Init(binary, ivector_dim, seed, pos); }},
      {"ivector-extractor-sum-accs",
       "Sum statistics for iVector extractor training; the output is the last argument.\n"
       "Usage: ivector-extractor-sum-accs [options] <stats-in1> <stats-in2> ... <stats-inN> <stats-out>\n"
       "Options: --binary (true) --parallel (accepted; the inputs are read one after another either way)\n",
       {xv::Bool("binary", &binary), xv::Bool("parallel", nullptr)}, 2, -1, [&](const Pos& pos) { return SumAccs(binary, pos); }},
      {"ivector-extractor-est",
       "Do model re-estimation of an iVector extractor.\n"
       "Usage: ivector-extractor-est [options] <model-in> <stats-in> <model-out>\n"
       "Options: --binary (true) --num-threads (1) --variance-floor-factor (0.1) --gaussian-min-count (100) --diagonalize (true)\n",
       {xv::Bool("binary", &binary), xv::Int("num-threads", &e.num_threads), xv::Double("variance-floor-factor", &e.variance_floor_factor),
        xv::Double("gaussian-min-count", &e.gaussian_min_count), xv::Bool("diagonalize", &e.diagonalize)},
       3, 3, [&](const Pos& pos) { return Est(binary, e, pos); }},
      {"ivector-extractor-acc-stats",
       "Accumulate stats for iVector extractor training, from features and Gaussian-level posteriors.\n"
       "Usage: ivector-extractor-acc-stats [options] <model-in> <feature-rspecifier> <posterior-rspecifier> <stats-out>\n"
       "Options: --binary (true) --update-variances (true) --compute-auxf (true) --verbose --device=<gpu>; --num-threads,\n"
       "--num-samples-for-weights and --cache-size are accepted and ignored.\n"
       "Limits: i-vector dimension <= 1024, feature dimension <= 96.\n",
       {xv::Ignored("num-threads"), xv::Ignored("num-samples-for-weights"), xv::Ignored("cache-size"), xv::Int("verbose", &o.verbose),
        xv::Bool("binary", &o.binary), xv::Bool("update-variances", &o.update_variances), xv::Bool("compute-auxf", &o.compute_auxf),
        xv::Int("device", &o.device)},
       4, 4, [&](const Pos& pos) { return AccStats(o, pos); }},
  };
  return xv::ToolsMain(argc, argv, tools, xv::NameRule::kExact, "ivector-extractor-acc-stats");
}
