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
#include "cmvn.h"
#include "gselect_lookup.h"
#include "kio.h"
#include "ubm.h"
#include "ubm_kernels.h"
#include "ubm_train.h"
#include "ubm_train_kernels.h"

namespace {

constexpr int64_t kBatchFrames = 1 << 16;   // frames read ahead; the accumulate calls do not depend on it

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

struct AccOptions {
  bool binary = true;
  std::string update_flags = "mvw", gselect;
  int device = -1, verbose = 0;
};

int AccStats(const AccOptions& o, const std::vector<std::string>& pos) {
  if (o.gselect.empty())
    throw xv::KioError("fgmm-global-acc-stats without --gselect is not built: every script of the recipes passes the Gaussian selection");
  const int flags = xv::ParseGmmFlags(o.update_flags);
  xv::FullGmmData gmm;
  xv::ReadFullGmmFile(pos[0], &gmm);
  const int dev = xv::PickDevice(o.device);
  std::unique_ptr<xv::FgmmAccumulator> acc(xv::FgmmAccCreate(dev, gmm.num_gauss, gmm.dim, flags));
  std::unique_ptr<xv::UbmModel> model(xv::UbmFullCreate(dev, gmm.num_gauss, gmm.dim, gmm.gconsts.data(), gmm.means_invcovars.data(), gmm.inv_covars.data()));
  xv::FeatBatchReader reader(pos[1], kBatchFrames, false);
  xv::GselectLookup gselect(o.gselect);
  long num_done = 0, num_err = 0;
  double tot_like = 0.0;
  int64_t tot_t = 0;
  // the stream of accepted frames, cut into blocks of exactly kFgmmAccFrameBlock: what is pending is less than one block
  std::vector<float> feats, logsum;
  std::vector<int32_t> gs;
  int n = 0;
  const int D = gmm.dim;
  size_t head = 0;   // frames at the front of the pending buffers that have been through the device
  auto accumulate = [&](size_t rows) {   // the next `rows` pending frames
    logsum.resize(rows);
    xv::FgmmAccAddGselect(acc.get(), *model, feats.data() + head * D, (int64_t)rows, gs.data() + head * n, n, logsum.data());
    for (size_t t = 0; t < rows; ++t) tot_like += logsum[t];
    tot_t += (int64_t)rows;
    head += rows;
  };
  xv::FeatBatchReader::Batch b;
  std::vector<xv::FeatBatchReader::Problem> problems;
  for (bool more = true; more;) {
    problems.clear();
    more = reader.Next(&b, &problems);
    for (const auto& p : problems) {
      if (p.what.empty()) {
        XWARN("Empty feature matrix for utterance " << p.key);   // no frames: skipped, not an error
      } else {
        XWARN("Failed to read features for key " << p.key << ": " << p.what);
        ++num_err;
      }
    }
    if (!more) break;
    for (size_t u = 0; u < b.keys.size(); ++u) {
      const int rows = b.row_off[u + 1] - b.row_off[u];
      if (b.cols != D) {
        XWARN("Dimension mismatch for utterance " << b.keys[u] << ": the features have " << b.cols << " columns, the model " << D);
        ++num_err;
        continue;
      }
      xv::IntVecVec sel;
      if (!gselect.Find(b.keys[u], &sel)) {
        XWARN("No gselect information for utterance " << b.keys[u]);
        ++num_err;
        continue;
      }
      if ((int)sel.size() != rows) {
        XWARN("gselect information for utterance " << b.keys[u] << " has wrong size " << sel.size() << " vs. " << rows);
        ++num_err;
        continue;
      }
      const size_t width = sel[0].size();
      bool same = width >= 1;
      for (const auto& l : sel) same = same && l.size() == width;
      if (!same || (n != 0 && (int)width != n)) {
        XWARN("The Gaussian selection of utterance " << b.keys[u] << " does not have " << (n ? "the " + std::to_string(n) + " indices per frame of the utterances before it" : "one length for every frame")
                                                    << " (skipping utterance)");
        ++num_err;
        continue;
      }
      if (width > (size_t)xv::kUbmMaxSelect)
        throw xv::KioError("the Gaussian selection has " + std::to_string(width) + " indices per frame; the device kernels take at most " + std::to_string(xv::kUbmMaxSelect));
      n = (int)width;
      feats.insert(feats.end(), b.feats.begin() + (size_t)b.row_off[u] * D, b.feats.begin() + (size_t)b.row_off[u + 1] * D);
      for (const auto& l : sel) gs.insert(gs.end(), l.begin(), l.end());
      while (feats.size() / D - head >= (size_t)xv::kFgmmAccFrameBlock) accumulate((size_t)xv::kFgmmAccFrameBlock);
      if (head) {   // drop what was consumed, once per utterance that filled a block
        feats.erase(feats.begin(), feats.begin() + head * D);
        gs.erase(gs.begin(), gs.begin() + head * n);
        head = 0;
      }
      ++num_done;
      if (o.verbose >= 1 && num_done % 10 == 0)   // over the frames that have been through the device: whole blocks
        XLOG("Avg like per frame so far is " << (tot_t ? tot_like / (double)tot_t : 0.0));
    }
  }
  if (!feats.empty()) accumulate(feats.size() / D);
  XLOG("Done " << num_done << " files; " << num_err << " with errors.");
  XLOG("Overall likelihood per frame = " << (tot_t ? tot_like / (double)tot_t : 0.0) << " over " << tot_t << " (weighted) frames.");
  xv::FgmmAccs host;
  host.Init(gmm.num_gauss, gmm.dim, flags);
  xv::FgmmAccGet(*acc, host.occ.data(), host.mean.data(), host.cov.data());
  xv::WriteFgmmAccsFile(pos[2], o.binary, host);
  XLOG("Written accs to " << pos[2]);
  return num_done != 0 ? 0 : 1;
}

int SumAccs(bool binary, const std::vector<std::string>& pos) {
  xv::FgmmAccs sum;
  for (size_t i = 1; i < pos.size(); ++i) xv::ReadFgmmAccsFile(pos[i], i > 1, &sum);
  xv::WriteFgmmAccsFile(pos[0], binary, sum);
  XLOG("Summed " << pos.size() - 1 << " stats");
  XLOG("Written stats to " << pos[0]);
  return 0;
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
  xv::ReadFgmmAccsFile(pos[1], false, &accs);
  xv::FgmmEstResult r;
  xv::FgmmEst(accs, flags, o.est, &gmm, &r);
  for (const std::string& w : r.warnings) XWARN(w);
  XLOG("Overall objective function improvement is " << (r.objf_after - r.objf_before) / r.count << " per frame over " << r.count << " frames");
  if (r.floored_elements) XWARN(r.floored_elements << " variances floored in " << r.floored_gauss << " Gaussians.");
  xv::WriteFullGmmFile(pos[2], o.binary, gmm);
  XLOG("Written model to " << pos[2]);
  return 0;
}

std::string Dashes(std::string n) {
  for (char& c : n)
    if (c == '_') c = '-';
  return n;
}

bool Common(const std::string& n) { return n == "verbose" || n == "print-args" || n == "config"; }

double ToDouble(const std::string& name, const std::string& v) {
  double d = 0.0;
  if (!xv::ParseDouble(v, &d)) throw xv::KioError("Invalid floating-point option --" + name + "=" + v);
  return d;
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
      const std::string n = Dashes(name);
      if (Common(n)) return xv::OptionResult::kOk;
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
      const std::string nm = Dashes(name);
      if (Common(nm)) return xv::OptionResult::kOk;
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
      const std::string n = Dashes(name);
      if (Common(n)) return xv::OptionResult::kOk;
      if (n == "binary") binary = xv::ToBool(n, val);
      else return xv::OptionResult::kUnknown;
      return xv::OptionResult::kOk;
    };
    t.run = [&](const std::vector<std::string>& pos) { return pos.size() < 2 ? xv::kUsageError : SumAccs(binary, pos); };
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
      const std::string n = Dashes(name);
      if (Common(n)) return xv::OptionResult::kOk;
      if (n == "binary") o.binary = xv::ToBool(n, val);
      else if (n == "update-flags") o.update_flags = val;
      else if (n == "min-gaussian-weight") o.est.min_gaussian_weight = ToDouble(n, val);
      else if (n == "min-gaussian-occupancy") o.est.min_gaussian_occupancy = ToDouble(n, val);
      else if (n == "variance-floor") o.est.variance_floor = ToDouble(n, val);
      else if (n == "max-condition") o.est.max_condition = ToDouble(n, val);
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
  AccOptions o;
  t.usage = "Accumulate stats for training a full-covariance GMM.\n"
            "Usage: fgmm-global-acc-stats [options] --gselect=<gselect-rspecifier> <model-in> <feature-rspecifier> <stats-out>\n"
            "Options: --binary (true) --update-flags (mvw) --gselect (required) --verbose --device=<gpu>\n"
            "Not built (refused): running without --gselect, --weights.\n";
  t.set = [&](const std::string& name, const std::string& val) {
    const std::string n = Dashes(name);
    if (n == "verbose") o.verbose = xv::ToInt(n, val);
    else if (Common(n)) return xv::OptionResult::kOk;
    else if (n == "binary") o.binary = xv::ToBool(n, val);
    else if (n == "update-flags") o.update_flags = val;
    else if (n == "gselect") o.gselect = val;
    else if (n == "device") o.device = xv::ToInt(n, val);
    else if (n == "weights") throw xv::KioError("--weights is not built: no script of the recipes passes per-frame weights");
    else return xv::OptionResult::kUnknown;
    return xv::OptionResult::kOk;
  };
  t.run = [&](const std::vector<std::string>& pos) { return pos.size() != 3 ? xv::kUsageError : AccStats(o, pos); };
  return xv::CliMain(argc, argv, t);
}
