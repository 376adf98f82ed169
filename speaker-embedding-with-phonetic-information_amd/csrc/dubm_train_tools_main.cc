// gmm-global-acc-stats / gmm-global-init-from-feats / gmm-global-sum-accs / gmm-global-est - drop-in command lines for diagonal UBM
// training (egs/sre/v1: sid/train_diag_ubm.sh:105-137).  One executable, dispatching on its exact base name:
//   gmm-global-init-from-feats [--binary=true --num-gauss=100 --num-gauss-init=0 --num-iters=50 --num-frames=200000 --num-threads=4
//                               --min-gaussian-weight=1e-5 --min-gaussian-occupancy=10 --min-variance=0.001
//                               --remove-low-count-gaussians=true --seed=0] <feature-rspecifier> <model-out>
//   gmm-global-acc-stats [--binary=true --update-flags=mvw] --gselect=<rspecifier> <model-in> <feature-rspecifier> <stats-out>
//   gmm-global-sum-accs [--binary=true] <stats-out> <stats-in1> <stats-in2> ...
//   gmm-global-est [--binary=true --update-flags=mvw --min-gaussian-weight=1e-5 --min-gaussian-occupancy=10 --min-variance=0.001
//                   --remove-low-count-gaussians=true --mix-up=0 --perturb-factor=0.01 --seed=0] <model-in> <stats-in> <model-out>
// Semantics: dubm_train.h.  The first two run on the device and fail without a GPU (exit 255); the others are host code and open no
// device.  Refused by name: gmm-global-acc-stats without --gselect and with --weights.
#include <math.h>
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "cli.h"
#include "feat_batch.h"
#include "dubm_train.h"
#include "dubm_train_kernels.h"
#include "gmm_acc_tool.h"
#include "kio.h"
#include "ubm.h"
#include "ubm_kernels.h"

namespace {

std::unique_ptr<xv::UbmModel> Upload(int dev, const xv::DiagGmmData& gmm) {
  return std::unique_ptr<xv::UbmModel>(xv::UbmDiagCreate(dev, gmm.num_gauss, gmm.dim, gmm.gconsts.data(), gmm.means_invvars.data(), gmm.inv_vars.data()));
}

int AccStats(const xv::GmmAccOptions& o, const std::vector<std::string>& pos) {
  if (o.gselect.empty())
    throw xv::KioError("gmm-global-acc-stats without --gselect is not built: sid/train_diag_ubm.sh always passes the Gaussian selection");
  const int flags = xv::ParseGmmFlags(o.update_flags);
  xv::DiagGmmData gmm;
  xv::ReadDiagGmmFile(pos[0], &gmm);
  const int dev = xv::PickDevice(o.device);
  std::unique_ptr<xv::DgmmAccumulator> acc(xv::DgmmAccCreate(dev, gmm.num_gauss, gmm.dim, flags));
  std::unique_ptr<xv::UbmModel> model = Upload(dev, gmm);
  xv::DgmmAccs host;
  host.Init(gmm.num_gauss, gmm.dim, flags);
  return xv::GmmAccStats(
      o, pos, &host, xv::kDgmmAccFrameBlock,
      [&](const float* feats, int64_t rows, const int32_t* gselect, int n, float* logsum) {
        xv::DgmmAccAddGselect(acc.get(), *model, feats, rows, gselect, n, nullptr, logsum);
      },
      [&] { xv::DgmmAccGet(*acc, host.occ.data(), host.mean.data(), host.second.data()); });
}

struct EstOptions {
  bool binary = true;
  std::string update_flags = "mvw";
  xv::DgmmEstOptions est;
  int mix_up = 0;
  double perturb_factor = 0.01;
  uint64_t seed = 0;
};

int Est(const EstOptions& o, const std::vector<std::string>& pos) {
  const int flags = xv::ParseGmmFlags(o.update_flags);
  xv::DiagGmmData gmm;
  xv::ReadDiagGmmFile(pos[0], &gmm);
  xv::DgmmAccs accs;
  xv::ReadGmmAccsFile(pos[1], false, &accs);
  xv::DgmmEstResult r;
  xv::DgmmEst(accs, flags, o.est, &gmm, &r);
  for (const std::string& w : r.warnings) XWARN(w);
  XLOG("Overall objective function improvement is " << (r.objf_after - r.objf_before) / r.count << " per frame over " << r.count << " frames");
  if (r.floored_elements) XWARN(r.floored_elements << " variances floored in " << r.floored_gauss << " Gaussians.");
  if (o.mix_up > gmm.num_gauss) {
    XLOG("Splitting to " << o.mix_up << " Gaussians.");
    xv::DgmmSplit(&gmm, o.mix_up, o.perturb_factor, o.seed, 0);
  }
  xv::WriteDiagGmmFile(pos[2], o.binary, gmm);
  XLOG("Written model to " << pos[2]);
  return 0;
}

struct InitOptions {
  bool binary = true;
  int num_gauss = 100, num_gauss_init = 0, num_iters = 50, num_frames = 200000, device = -1;
  xv::DgmmEstOptions est;
  uint64_t seed = 0;
};

int InitFromFeats(const InitOptions& o, const std::vector<std::string>& pos) {
  if (o.num_gauss < 1 || o.num_iters < 0 || o.num_frames < 1) throw xv::KioError("--num-gauss and --num-frames must be at least 1, --num-iters not negative");
  // (no result depends on the frames read ahead)
  xv::FeatBatchWalk walk(pos[0], xv::kBatchFrames, false, xv::FeatProblems::kThrowUnreadable);
  xv::DgmmFrameSampler sampler;
  sampler.num_frames = o.num_frames;
  sampler.seed = o.seed;
  walk.Run([&](const xv::FeatBatchReader::Batch& b) {
    if (sampler.dim == 0) sampler.dim = b.cols;
    if (b.cols != sampler.dim)
      throw xv::KioError("Features have inconsistent dims " + std::to_string(b.cols) + " vs. " + std::to_string(sampler.dim) + " (current utt is) " + b.keys[0]);
    const int64_t rows = b.row_off[b.keys.size()];
    for (int64_t t = 0; t < rows; ++t) sampler.Add(b.feats.data() + (size_t)t * b.cols);
  });
  const int64_t T = sampler.rows();
  if (T == 0) throw xv::KioError("No frames were read from " + pos[0]);
  if (sampler.num_read < o.num_frames) {
    XWARN("Number of frames read " << sampler.num_read << " was less than target number " << o.num_frames << ", using all we read.");
  } else {
    XLOG("Kept " << T << " out of " << sampler.num_read << " input frames = " << 100.0 * (double)T / (double)sampler.num_read << "%.");
  }
  const int D = sampler.dim;
  if (D > xv::kDgmmMaxDim)
    throw xv::KioError("the dimension " + std::to_string(D) + " is above the accumulation kernels' limit of " + std::to_string(xv::kDgmmMaxDim));
  int num_gauss_init = o.num_gauss_init;
  if (num_gauss_init <= 0 || num_gauss_init > o.num_gauss) num_gauss_init = o.num_gauss;
  xv::DiagGmmData gmm;
  xv::DgmmInitFromFrames(sampler.kept.data(), T, D, num_gauss_init, o.seed, &gmm);
  const int dev = xv::PickDevice(o.device);
  std::unique_ptr<xv::DgmmAccumulator> acc(xv::DgmmAccCreate(dev, gmm.num_gauss, D, 7));
  xv::DgmmAccSetFrames(acc.get(), sampler.kept.data(), T);   // once: the iterations upload the model alone
  const int half = o.num_iters / 2;
  const int gauss_inc = half > 0 ? (o.num_gauss - num_gauss_init) / half : o.num_gauss - num_gauss_init;
  int cur_num_gauss = num_gauss_init;
  std::vector<float> logsum((size_t)T);
  xv::DgmmAccs host;
  for (int iter = 0; iter < o.num_iters; ++iter) {
    xv::DgmmAccReset(acc.get(), gmm.num_gauss);
    std::unique_ptr<xv::UbmModel> model = Upload(dev, gmm);
    xv::DgmmAccAddDense(acc.get(), *model, nullptr, T, logsum.data());
    double tot_like = 0.0;
    for (int64_t t = 0; t < T; ++t) tot_like += logsum[t];
    XLOG("Likelihood per frame on iteration " << iter << " was " << tot_like / (double)T << " over " << T << " frames.");
    host.Init(gmm.num_gauss, D, 7);
    xv::DgmmAccGet(*acc, host.occ.data(), host.mean.data(), host.second.data());
    xv::DgmmEstResult r;
    xv::DgmmEst(host, 7, o.est, &gmm, &r);
    for (const std::string& w : r.warnings) XWARN(w);
    XLOG("Objective-function change on iteration " << iter << " was " << (r.objf_after - r.objf_before) / r.count << " over " << r.count << " frames.");
    const int next_num_gauss = std::min(o.num_gauss, cur_num_gauss + gauss_inc);
    if (next_num_gauss > gmm.num_gauss) {
      XLOG("Splitting to " << next_num_gauss << " Gaussians.");
      xv::DgmmSplit(&gmm, next_num_gauss, 0.1, o.seed, (uint64_t)iter + 1);
      cur_num_gauss = next_num_gauss;
    }
  }
  xv::WriteDiagGmmFile(pos[1], o.binary, gmm);
  XLOG("Wrote model to " << pos[1]);
  return 0;
}

// appends the four options of the M-step that gmm-global-est and gmm-global-init-from-feats share
void AppendEstOptions(xv::DgmmEstOptions* est, std::vector<xv::CliOption>* to) {
  to->insert(to->end(), {xv::Double("min-gaussian-weight", &est->min_gaussian_weight), xv::Double("min-gaussian-occupancy", &est->min_gaussian_occupancy),
                         xv::Double("min-variance", &est->min_variance), xv::Bool("remove-low-count-gaussians", &est->remove_low_count_gaussians)});
}

}  // namespace

int main(int argc, char** argv) {
  using Pos = std::vector<std::string>;
  bool binary = true;
  EstOptions e;
  InitOptions io;
  xv::GmmAccOptions o;
  std::vector<xv::CliTool> tools = {
      {"gmm-global-acc-stats",
       "Accumulate stats for training a diagonal-covariance GMM.\n"
       "Usage: gmm-global-acc-stats [options] --gselect=<gselect-rspecifier> <model-in> <feature-rspecifier> <stats-out>\n"
       "Options: --binary (true) --update-flags (mvw) --gselect (required) --verbose --device=<gpu>\n"
       "Not built (refused): running without --gselect, --weights.\n",
       {xv::Refused("weights", "--weights is not built: sid/train_diag_ubm.sh passes no per-frame weights")},
       3, 3, [&](const Pos& pos) { return AccStats(o, pos); }},
      {"gmm-global-init-from-feats",
       "This program initializes a single diagonal GMM and does multiple iterations of training from features held in memory.\n"
       "Usage: gmm-global-init-from-feats [options] <feature-rspecifier> <model-out>\n"
       "Options: --binary (true) --num-gauss (100) --num-gauss-init (0) --num-iters (50) --num-frames (200000)\n"
       "         --num-threads (4; accepted and ignored) --min-gaussian-weight (1e-5) --min-gaussian-occupancy (10)\n"
       "         --min-variance (0.001) --remove-low-count-gaussians (true) --seed (0) --verbose --device=<gpu>\n",
       {xv::Bool("binary", &io.binary), xv::Int("num-gauss", &io.num_gauss), xv::Int("num-gauss-init", &io.num_gauss_init),
        xv::Int("num-iters", &io.num_iters), xv::Int("num-frames", &io.num_frames), xv::Int("num-threads", nullptr),
        xv::Seed("seed", &io.seed), xv::Int("device", &io.device)},
       2, 2, [&](const Pos& pos) { return InitFromFeats(io, pos); }},
      {"gmm-global-sum-accs",
       "Sum multiple accumulated stats files for diagonal-covariance GMM training.\n"
       "Usage: gmm-global-sum-accs [options] <stats-out> <stats-in1> <stats-in2> ...\n"
       "Options: --binary (true)\n",
       {xv::Bool("binary", &binary)}, 2, -1, [&](const Pos& pos) { return xv::GmmSumAccs(false, binary, pos); }},
      {"gmm-global-est",
       "Estimate a diagonal-covariance GMM from the accumulated stats.\n"
       "Usage: gmm-global-est [options] <model-in> <stats-in> <model-out>\n"
       "Options: --binary (true) --update-flags (mvw) --min-gaussian-weight (1e-5) --min-gaussian-occupancy (10)\n"
       "         --min-variance (0.001) --remove-low-count-gaussians (true) --mix-up (0) --perturb-factor (0.01) --seed (0)\n",
       {xv::Bool("binary", &e.binary), xv::String("update-flags", &e.update_flags), xv::Int("mix-up", &e.mix_up),
        xv::Double("perturb-factor", &e.perturb_factor), xv::Seed("seed", &e.seed)},
       3, 3, [&](const Pos& pos) { return Est(e, pos); }},
  };
  xv::AppendGmmAccOptions(&o, &tools[0].options);
  AppendEstOptions(&io.est, &tools[1].options);
  AppendEstOptions(&e.est, &tools[3].options);
  return xv::ToolsMain(argc, argv, tools, xv::NameRule::kExactOrRefuse);
}
