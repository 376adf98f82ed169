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

// the four options of the M-step that gmm-global-est and gmm-global-init-from-feats share
bool SetEstOption(const std::string& n, const std::string& val, xv::DgmmEstOptions* est) {
  if (n == "min-gaussian-weight") est->min_gaussian_weight = xv::ToDouble(n, val);
  else if (n == "min-gaussian-occupancy") est->min_gaussian_occupancy = xv::ToDouble(n, val);
  else if (n == "min-variance") est->min_variance = xv::ToDouble(n, val);
  else if (n == "remove-low-count-gaussians") est->remove_low_count_gaussians = xv::ToBool(n, val);
  else return false;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string prog = xv::ProgramName(argv[0]);
  xv::CliTool t;
  t.config_file = false;
  if (prog == "gmm-global-sum-accs") {
    bool binary = true;
    t.usage = "Sum multiple accumulated stats files for diagonal-covariance GMM training.\n"
              "Usage: gmm-global-sum-accs [options] <stats-out> <stats-in1> <stats-in2> ...\n"
              "Options: --binary (true)\n";
    t.set = [&](const std::string& name, const std::string& val) {
      const std::string n = xv::Dashes(name);
      if (xv::CommonOption(n)) return xv::OptionResult::kOk;
      if (n == "binary") binary = xv::ToBool(n, val);
      else return xv::OptionResult::kUnknown;
      return xv::OptionResult::kOk;
    };
    t.run = [&](const std::vector<std::string>& pos) { return pos.size() < 2 ? xv::kUsageError : xv::GmmSumAccs(false, binary, pos); };
    return xv::CliMain(argc, argv, t);
  }
  if (prog == "gmm-global-est") {
    EstOptions o;
    t.usage = "Estimate a diagonal-covariance GMM from the accumulated stats.\n"
              "Usage: gmm-global-est [options] <model-in> <stats-in> <model-out>\n"
              "Options: --binary (true) --update-flags (mvw) --min-gaussian-weight (1e-5) --min-gaussian-occupancy (10)\n"
              "         --min-variance (0.001) --remove-low-count-gaussians (true) --mix-up (0) --perturb-factor (0.01) --seed (0)\n";
    t.set = [&](const std::string& name, const std::string& val) {
      const std::string n = xv::Dashes(name);
      if (xv::CommonOption(n)) return xv::OptionResult::kOk;
      if (n == "binary") o.binary = xv::ToBool(n, val);
      else if (n == "update-flags") o.update_flags = val;
      else if (SetEstOption(n, val, &o.est)) return xv::OptionResult::kOk;
      else if (n == "mix-up") o.mix_up = xv::ToInt(n, val);
      else if (n == "perturb-factor") o.perturb_factor = xv::ToDouble(n, val);
      else if (n == "seed") o.seed = xv::ToSeed(n, val);
      else return xv::OptionResult::kUnknown;
      return xv::OptionResult::kOk;
    };
    t.run = [&](const std::vector<std::string>& pos) { return pos.size() != 3 ? xv::kUsageError : Est(o, pos); };
    return xv::CliMain(argc, argv, t);
  }
  if (prog == "gmm-global-init-from-feats") {
    InitOptions o;
    t.usage = "This program initializes a single diagonal GMM and does multiple iterations of training from features held in memory.\n"
              "Usage: gmm-global-init-from-feats [options] <feature-rspecifier> <model-out>\n"
              "Options: --binary (true) --num-gauss (100) --num-gauss-init (0) --num-iters (50) --num-frames (200000)\n"
              "         --num-threads (4; accepted and ignored) --min-gaussian-weight (1e-5) --min-gaussian-occupancy (10)\n"
              "         --min-variance (0.001) --remove-low-count-gaussians (true) --seed (0) --verbose --device=<gpu>\n";
    t.set = [&](const std::string& name, const std::string& val) {
      const std::string n = xv::Dashes(name);
      if (xv::CommonOption(n)) return xv::OptionResult::kOk;
      if (n == "binary") o.binary = xv::ToBool(n, val);
      else if (n == "num-gauss") o.num_gauss = xv::ToInt(n, val);
      else if (n == "num-gauss-init") o.num_gauss_init = xv::ToInt(n, val);
      else if (n == "num-iters") o.num_iters = xv::ToInt(n, val);
      else if (n == "num-frames") o.num_frames = xv::ToInt(n, val);
      else if (n == "num-threads") (void)xv::ToInt(n, val);
      else if (SetEstOption(n, val, &o.est)) return xv::OptionResult::kOk;
      else if (n == "seed") o.seed = xv::ToSeed(n, val);
      else if (n == "device") o.device = xv::ToInt(n, val);
      else return xv::OptionResult::kUnknown;
      return xv::OptionResult::kOk;
    };
    t.run = [&](const std::vector<std::string>& pos) { return pos.size() != 2 ? xv::kUsageError : InitFromFeats(o, pos); };
    return xv::CliMain(argc, argv, t);
  }
  if (prog != "gmm-global-acc-stats") {
    fprintf(stderr, "%s: not one of gmm-global-acc-stats, gmm-global-init-from-feats, gmm-global-sum-accs, gmm-global-est\n", prog.c_str());
    return 255;
  }
  xv::GmmAccOptions o;
  t.usage = "Accumulate stats for training a diagonal-covariance GMM.\n"
            "Usage: gmm-global-acc-stats [options] --gselect=<gselect-rspecifier> <model-in> <feature-rspecifier> <stats-out>\n"
            "Options: --binary (true) --update-flags (mvw) --gselect (required) --verbose --device=<gpu>\n"
            "Not built (refused): running without --gselect, --weights.\n";
  t.set = [&](const std::string& name, const std::string& val) {
    const std::string n = xv::Dashes(name);
    if (n == "weights") throw xv::KioError("--weights is not built: sid/train_diag_ubm.sh passes no per-frame weights");
    return xv::SetGmmAccOption(n, val, &o);
  };
  t.run = [&](const std::vector<std::string>& pos) { return pos.size() != 3 ? xv::kUsageError : AccStats(o, pos); };
  return xv::CliMain(argc, argv, t);
}
