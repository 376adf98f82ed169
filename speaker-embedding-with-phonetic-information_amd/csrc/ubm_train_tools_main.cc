// fgmm-global-acc-stats / gmm-global-to-fgmm / subsample-feats / fgmm-global-sum-accs / fgmm-global-est - drop-in command lines for
// full-covariance UBM training (egs/sre/v1: sid/train_full_ubm.sh:69-118).  One executable, dispatching on its exact base name:
//   gmm-global-to-fgmm [--binary=true] <diag-gmm-in> <full-gmm-out>
//   subsample-feats [--n=1 --offset=0] <feats-rspecifier> <feats-wspecifier>
//   fgmm-global-acc-stats [--binary=true --update-flags=mvw] --gselect=<rspecifier> <model-in> <feats-rspecifier> <stats-out>
//   fgmm-global-sum-accs [--binary=true] <stats-out> <stats-in1> <stats-in2> ...
//   fgmm-global-est [--binary=true --update-flags=mvw --min-gaussian-weight=1e-5 --min-gaussian-occupancy=100 --variance-floor=0.001
//                    --max-condition=1e5 --remove-low-count-gaussians=true] <model-in> <stats-in> <model-out>
// Semantics: ubm_train.h.  fgmm-global-acc-stats runs on the device and fails without a GPU (exit 255); the others are host code and
// open no device.  Models and statistics are rxfilenames / wxfilenames ("0.ubm", "-", "fgmm-global-sum-accs - a.1.acc a.2.acc |").
// Refused by name: fgmm-global-acc-stats without --gselect and with --weights, fgmm-global-est --mix-up other than 0.
#include <math.h>
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "cli.h"
#include "gmm_acc_tool.h"
#include "kio.h"
#include "ubm.h"
#include "ubm_kernels.h"
#include "ubm_train.h"
#include "ubm_train_kernels.h"

namespace {

int GmmToFgmm(bool binary, const std::vector<std::string>& pos) {
  xv::DiagGmmData diag;
  xv::ReadDiagGmmFile(pos[0], &diag);
  xv::FullGmmData full;
  xv::DiagGmmToFull(diag, &full);
  xv::WriteFullGmmFile(pos[1], binary, full);
  XLOG("Written full GMM to " << pos[1]);
  return 0;
}

int SubsampleFeats(int n, int offset, const std::vector<std::string>& pos) {
  if (offset < 0) throw xv::KioError("Invalid option --offset=" + std::to_string(offset) + ": it must not be negative");
  if (n < 0 && offset != 0) throw xv::KioError("--offset=" + std::to_string(offset) + " cannot be used with a negative --n: frames are then repeated");
  xv::SequentialMatrixReader reader(pos[0]);
  xv::TableWriter writer(pos[1]);
  long num_done = 0, num_err = 0;
  int64_t frames_in = 0, frames_out = 0;
  std::string key, err;
  xv::Matrix m, out;
  while (reader.Next(&key, &m, &err)) {
    if (!err.empty()) {
      XWARN("Failed to read features for key " << key << ": " << err);
      ++num_err;
      continue;
    }
    if (m.cm) {
      xv::Matrix full;
      xv::ExpandCompressedView(m, &full);
      m = full;
    }
    out.cols = m.cols;
    out.data.clear();
    if (n > 0) {
      out.rows = m.rows > offset ? (m.rows - offset + n - 1) / n : 0;
      frames_in += m.rows;
      frames_out += out.rows;
      if (out.rows == 0) {
        XWARN("For utterance " << key << ", output would have no rows, producing no output.");
        ++num_err;
        continue;
      }
      for (int r = offset; r < m.rows; r += n) out.data.insert(out.data.end(), m.Row(r), m.Row(r) + m.cols);
    } else {
      const int rep = -n;
      out.rows = m.rows * rep;
      frames_in += m.rows;
      frames_out += out.rows;
      if (out.rows == 0) {
        XWARN("For utterance " << key << ", output would have no rows, producing no output.");
        ++num_err;
        continue;
      }
      for (int r = 0; r < m.rows; ++r)
        for (int k = 0; k < rep; ++k) out.data.insert(out.data.end(), m.Row(r), m.Row(r) + m.cols);
    }
    writer.WriteMat(key, out);
    ++num_done;
  }
  writer.Close();
  XLOG("Processed " << num_done << " feature matrices; " << num_err << " with errors.");
  XLOG("Processed " << frames_in << " input frames and " << frames_out << " output frames.");
  return num_done != 0 ? 0 : 1;
}

int AccStats(const xv::GmmAccOptions& o, const std::vector<std::string>& pos) {
  if (o.gselect.empty())
    throw xv::KioError("fgmm-global-acc-stats without --gselect is not built: every script of the recipes passes the Gaussian selection");
  const int flags = xv::ParseGmmFlags(o.update_flags);
  xv::FullGmmData gmm;
  xv::ReadFullGmmFile(pos[0], &gmm);
  const int dev = xv::PickDevice(o.device);
  std::unique_ptr<xv::FgmmAccumulator> acc(xv::FgmmAccCreate(dev, gmm.num_gauss, gmm.dim, flags));
  std::unique_ptr<xv::UbmModel> model(xv::UbmFullCreate(dev, gmm.num_gauss, gmm.dim, gmm.gconsts.data(), gmm.means_invcovars.data(), gmm.inv_covars.data()));
  xv::FgmmAccs host;
  host.Init(gmm.num_gauss, gmm.dim, flags);
  return xv::GmmAccStats(
      o, pos, &host, xv::kFgmmAccFrameBlock,
      [&](const float* feats, int64_t rows, const int32_t* gselect, int n, float* logsum) {
        xv::FgmmAccAddGselect(acc.get(), *model, feats, rows, gselect, n, logsum);
      },
      [&] { xv::FgmmAccGet(*acc, host.occ.data(), host.mean.data(), host.second.data()); });
}

struct EstOptions {
  bool binary = true;
  std::string update_flags = "mvw";
  xv::FgmmEstOptions est;
};

int Est(const EstOptions& o, const std::vector<std::string>& pos) {
  const int flags = xv::ParseGmmFlags(o.update_flags);
  xv::FullGmmData gmm;
  xv::ReadFullGmmFile(pos[0], &gmm);
  xv::FgmmAccs accs;
  xv::ReadGmmAccsFile(pos[1], false, &accs);
  xv::FgmmEstResult r;
  xv::FgmmEst(accs, flags, o.est, &gmm, &r);
  for (const std::string& w : r.warnings) XWARN(w);
  XLOG("Overall objective function improvement is " << (r.objf_after - r.objf_before) / r.count << " per frame over " << r.count << " frames");
  if (r.floored_elements) XWARN(r.floored_elements << " variances floored in " << r.floored_gauss << " Gaussians.");
  xv::WriteFullGmmFile(pos[2], o.binary, gmm);
  XLOG("Written model to " << pos[2]);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  using Pos = std::vector<std::string>;
  bool binary = true;
  int n = 1, offset = 0;
  EstOptions e;
  xv::GmmAccOptions o;
  std::vector<xv::CliTool> tools = {
      {"fgmm-global-acc-stats",
       "Accumulate stats for training a full-covariance GMM.\n"
       "Usage: fgmm-global-acc-stats [options] --gselect=<gselect-rspecifier> <model-in> <feature-rspecifier> <stats-out>\n"
       "Options: --binary (true) --update-flags (mvw) --gselect (required) --verbose --device=<gpu>\n"
       "Not built (refused): running without --gselect, --weights.\n",
       {xv::Refused("weights", "--weights is not built: no script of the recipes passes per-frame weights")},
       3, 3, [&](const Pos& pos) { return AccStats(o, pos); }},
      {"gmm-global-to-fgmm",
       "Convert single diagonal-covariance GMM to single full-covariance GMM.\n"
       "Usage: gmm-global-to-fgmm [options] <diag-gmm-in> <full-gmm-out>\n"
       "Options: --binary (true)\n",
       {xv::Bool("binary", &binary)}, 2, 2, [&](const Pos& pos) { return GmmToFgmm(binary, pos); }},
      {"subsample-feats",
       "Sub-samples features by taking every n'th frame.  With negative values of n, will repeat each frame n times\n"
       "(e.g. --n=-2 will repeat each frame twice)\n"
       "Usage: subsample-feats [options] <in-rspecifier> <out-wspecifier>\n"
       "Options: --n (1) --offset (0; must be 0 with a negative --n)\n",
       {xv::Int("n", &n), xv::Int("offset", &offset)}, 2, 2,
       [&](const Pos& pos) { return n == 0 ? xv::kUsageError : SubsampleFeats(n, offset, pos); }},
      {"fgmm-global-sum-accs",
       "Sum multiple accumulated stats files for full-covariance GMM training.\n"
       "Usage: fgmm-global-sum-accs [options] <stats-out> <stats-in1> <stats-in2> ...\n"
       "Options: --binary (true)\n",
       {xv::Bool("binary", &binary)}, 2, -1, [&](const Pos& pos) { return xv::GmmSumAccs(true, binary, pos); }},
      {"fgmm-global-est",
       "Estimate a full-covariance GMM from the accumulated stats.\n"
       "Usage: fgmm-global-est [options] <model-in> <stats-in> <model-out>\n"
       "Options: --binary (true) --update-flags (mvw) --min-gaussian-weight (1e-5) --min-gaussian-occupancy (100)\n"
       "         --variance-floor (0.001) --max-condition (1e5) --remove-low-count-gaussians (true)\n"
       "Not built (refused): --mix-up other than 0.\n",
       {xv::Bool("binary", &e.binary), xv::String("update-flags", &e.update_flags), xv::Double("min-gaussian-weight", &e.est.min_gaussian_weight),
        xv::Double("min-gaussian-occupancy", &e.est.min_gaussian_occupancy), xv::Double("variance-floor", &e.est.variance_floor),
        xv::Double("max-condition", &e.est.max_condition), xv::Bool("remove-low-count-gaussians", &e.est.remove_low_count_gaussians),
        xv::RefusedIfNonZero("mix-up", "--mix-up is not built: no script of the recipes increases the number of Gaussians here")},
       3, 3, [&](const Pos& pos) { return Est(e, pos); }},
  };
  xv::AppendGmmAccOptions(&o, &tools[0].options);
  return xv::ToolsMain(argc, argv, tools, xv::NameRule::kExactOrRefuse);
}
