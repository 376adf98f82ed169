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
  const std::string prog = xv::ProgramName(argv[0]);
  xv::CliTool t;
  t.config_file = false;
  if (prog == "gmm-global-to-fgmm") {
    bool binary = true;
    t.usage = "Convert single diagonal-covariance GMM to single full-covariance GMM.\n"
              "Usage: gmm-global-to-fgmm [options] <diag-gmm-in> <full-gmm-out>\n"
              "Options: --binary (true)\n";
    t.set = [&](const std::string& name, const std::string& val) {
      const std::string n = xv::Dashes(name);
      if (xv::CommonOption(n)) return xv::OptionResult::kOk;
      if (n == "binary") binary = xv::ToBool(n, val);
      else return xv::OptionResult::kUnknown;
      return xv::OptionResult::kOk;
    };
    t.run = [&](const std::vector<std::string>& pos) { return pos.size() != 2 ? xv::kUsageError : GmmToFgmm(binary, pos); };
    return xv::CliMain(argc, argv, t);
  }
  if (prog == "subsample-feats") {
    int n = 1, offset = 0;
    t.usage = "Sub-samples features by taking every n'th frame.  With negative values of n, will repeat each frame n times\n"
              "(e.g. --n=-2 will repeat each frame twice)\n"
              "Usage: subsample-feats [options] <in-rspecifier> <out-wspecifier>\n"
              "Options: --n (1) --offset (0; must be 0 with a negative --n)\n";
    t.set = [&](const std::string& name, const std::string& val) {
      const std::string nm = xv::Dashes(name);
      if (xv::CommonOption(nm)) return xv::OptionResult::kOk;
      if (nm == "n") n = xv::ToInt(nm, val);
      else if (nm == "offset") offset = xv::ToInt(nm, val);
      else return xv::OptionResult::kUnknown;
      return xv::OptionResult::kOk;
    };
    t.run = [&](const std::vector<std::string>& pos) { return pos.size() != 2 || n == 0 ? xv::kUsageError : SubsampleFeats(n, offset, pos); };
    return xv::CliMain(argc, argv, t);
  }
  if (prog == "fgmm-global-sum-accs") {
    bool binary = true;
    t.usage = "Sum multiple accumulated stats files for full-covariance GMM training.\n"
              "Usage: fgmm-global-sum-accs [options] <stats-out> <stats-in1> <stats-in2> ...\n"
              "Options: --binary (true)\n";
    t.set = [&](const std::string& name, const std::string& val) {
      const std::string n = xv::Dashes(name);
      if (xv::CommonOption(n)) return xv::OptionResult::kOk;
      if (n == "binary") binary = xv::ToBool(n, val);
      else return xv::OptionResult::kUnknown;
      return xv::OptionResult::kOk;
    };
    t.run = [&](const std::vector<std::string>& pos) { return pos.size() < 2 ? xv::kUsageError : xv::GmmSumAccs(true, binary, pos); };
    return xv::CliMain(argc, argv, t);
  }
  if (prog == "fgmm-global-est") {
    EstOptions o;
    t.usage = "Estimate a full-covariance GMM from the accumulated stats.\n"
              "Usage: fgmm-global-est [options] <model-in> <stats-in> <model-out>\n"
              "Options: --binary (true) --update-flags (mvw) --min-gaussian-weight (1e-5) --min-gaussian-occupancy (100)\n"
              "         --variance-floor (0.001) --max-condition (1e5) --remove-low-count-gaussians (true)\n"
              "Not built (refused): --mix-up other than 0.\n";
    t.set = [&](const std::string& name, const std::string& val) {
      const std::string n = xv::Dashes(name);
      if (xv::CommonOption(n)) return xv::OptionResult::kOk;
      if (n == "binary") o.binary = xv::ToBool(n, val);
      else if (n == "update-flags") o.update_flags = val;
      else if (n == "min-gaussian-weight") o.est.min_gaussian_weight = xv::ToDouble(n, val);
      else if (n == "min-gaussian-occupancy") o.est.min_gaussian_occupancy = xv::ToDouble(n, val);
      else if (n == "variance-floor") o.est.variance_floor = xv::ToDouble(n, val);
      else if (n == "max-condition") o.est.max_condition = xv::ToDouble(n, val);
      else if (n == "remove-low-count-gaussians") o.est.remove_low_count_gaussians = xv::ToBool(n, val);
      else if (n == "mix-up") {
        if (xv::ToInt(n, val) != 0) throw xv::KioError("--mix-up is not built: no script of the recipes increases the number of Gaussians here");
      } else return xv::OptionResult::kUnknown;
      return xv::OptionResult::kOk;
    };
    t.run = [&](const std::vector<std::string>& pos) { return pos.size() != 3 ? xv::kUsageError : Est(o, pos); };
    return xv::CliMain(argc, argv, t);
  }
  if (prog != "fgmm-global-acc-stats") {
    fprintf(stderr, "%s: not one of fgmm-global-acc-stats, gmm-global-to-fgmm, subsample-feats, fgmm-global-sum-accs, fgmm-global-est\n", prog.c_str());
    return 255;
  }
  xv::GmmAccOptions o;
  t.usage = "Accumulate stats for training a full-covariance GMM.\n"
            "Usage: fgmm-global-acc-stats [options] --gselect=<gselect-rspecifier> <model-in> <feature-rspecifier> <stats-out>\n"
            "Options: --binary (true) --update-flags (mvw) --gselect (required) --verbose --device=<gpu>\n"
            "Not built (refused): running without --gselect, --weights.\n";
  t.set = [&](const std::string& name, const std::string& val) {
    const std::string n = xv::Dashes(name);
    if (n == "weights") throw xv::KioError("--weights is not built: no script of the recipes passes per-frame weights");
    return xv::SetGmmAccOption(n, val, &o);
  };
  t.run = [&](const std::vector<std::string>& pos) { return pos.size() != 3 ? xv::kUsageError : AccStats(o, pos); };
  return xv::CliMain(argc, argv, t);
}
