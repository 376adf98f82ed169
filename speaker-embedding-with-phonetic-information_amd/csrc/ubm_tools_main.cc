// add-deltas / fgmm-global-to-gmm / gmm-gselect / fgmm-global-gselect-to-post / scale-post - drop-in command lines for the
// frame-rate half of the GMM-UBM i-vector baseline (egs/sre/v1: sid/extract_ivectors.sh:58-68; the same three commands open
// sid/train_full_ubm.sh and sid/train_ivector_extractor.sh).  One executable, dispatching on its name:
//   add-deltas [--delta-order=2 --delta-window=2 --truncate=0] <feats-rspecifier> <feats-wspecifier>
//   fgmm-global-to-gmm [--binary=true] <full-gmm-in> <diag-gmm-out>
//   gmm-gselect [--n=50] <diag-gmm-in> <feats-rspecifier> <gselect-wspecifier>
//   fgmm-global-gselect-to-post [--min-post=0.0] <full-gmm-in> <feats-rspecifier> <gselect-rspecifier> <post-wspecifier>
//   scale-post <post-rspecifier> (<scale>|<scale-rspecifier>) <post-wspecifier>
//   fgmm-global-copy [--binary=true] <full-gmm-in> <full-gmm-out>;  gmm-global-copy [--binary=true] <diag-gmm-in> <diag-gmm-out>
//   copy-gselect [--n=-1] <gselect-rspecifier> <gselect-wspecifier>
// add-deltas, gmm-gselect and fgmm-global-gselect-to-post run on the device (ubm.h) and fail without a GPU (exit 255); the others
// are host code and open no device (the three copies rewrite a model or a table, recomputing a model's gconsts on the way).  Models are rxfilenames ("final.ubm", "-", "fgmm-global-to-gmm final.ubm -|"); features
// are read ahead in batches, so the recipes' "ark,s,cs:add-deltas ... | apply-cmvn-sliding ... | select-voiced-frames ... |" is
// a child pipeline read front to back.  Refused by name: gmm-gselect --write-likes and --gselect.
// ivector-extract, line 69 of that script, takes the posteriors from here: ivex_tools_main.cc.
#include <stdlib.h>

#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "cli.h"
#include "feat_batch.h"
#include "feat_join.h"
#include "kio.h"
#include "ubm.h"
#include "ubm_kernels.h"

namespace {

struct DeltaOptions {
  int order = 2, window = 2, truncate = 0, device = -1;
};

int AddDeltas(const DeltaOptions& o, const std::vector<std::string>& pos) {
  const int dev = xv::PickDevice(o.device);
  xv::FeatBatchWalk feats(pos[0], xv::kBatchFrames, false, xv::FeatProblems::kCount);
  xv::TableWriter writer(pos[1]);
  long num_done = 0;
  std::vector<float> out;
  const long num_err = feats.Run([&](const xv::FeatBatchReader::Batch& b) {
    const int n = (int)b.keys.size();
    const int oc = (o.order + 1) * (o.truncate > 0 ? o.truncate : b.cols);
    out.resize((size_t)b.row_off[n] * oc);
    xv::AddDeltas(dev, b.feats.data(), b.row_off.data(), n, b.cols, o.order, o.window, o.truncate, out.data());
    for (int u = 0; u < n; ++u) {
      xv::Matrix m;
      m.rows = b.row_off[u + 1] - b.row_off[u];
      m.cols = oc;
      m.data.assign(out.begin() + (size_t)b.row_off[u] * oc, out.begin() + (size_t)b.row_off[u + 1] * oc);
      writer.WriteMat(b.keys[u], m);
      ++num_done;
    }
  });
  writer.Close();
  XLOG("Done " << num_done << " files, " << num_err << " with errors.");
  return num_done != 0 ? 0 : 1;
}

int FgmmToGmm(bool binary, const std::vector<std::string>& pos) {
  xv::FullGmmData full;
  xv::ReadFullGmmFile(pos[0], &full);
  xv::DiagGmmData diag;
  xv::FullGmmToDiag(full, &diag);
  xv::WriteDiagGmmFile(pos[1], binary, diag);
  XLOG("Written diagonal GMM to " << pos[1]);
  return 0;
}

int GmmGselect(int n_opt, int device, const std::vector<std::string>& pos) {
  if (n_opt < 1) throw xv::KioError("--n must be at least 1");
  xv::DiagGmmData gmm;
  xv::ReadDiagGmmFile(pos[0], &gmm);
  int n = n_opt;
  if (n > gmm.num_gauss) {
    XWARN("You asked for " << n << " Gaussians but GMM only has " << gmm.num_gauss << ", returning this many. Note: this means the Gaussian selection is pointless.");
    n = gmm.num_gauss;
  }
  if (n > xv::kUbmMaxSelect)
    throw xv::KioError("--n=" + std::to_string(n) + " is above the limit of " + std::to_string(xv::kUbmMaxSelect) + " selected Gaussians per frame of the device kernel");
  const int dev = xv::PickDevice(device);
  std::unique_ptr<xv::UbmModel> model(xv::UbmDiagCreate(dev, gmm.num_gauss, gmm.dim, gmm.gconsts.data(), gmm.means_invvars.data(), gmm.inv_vars.data()));
  xv::FeatBatchWalk feats(pos[1], xv::kBatchFrames, false, xv::FeatProblems::kCount);
  xv::TableWriter writer(pos[2]);
  long num_done = 0, num_err = 0;
  double tot_like = 0.0;
  int64_t tot_t = 0;
  std::vector<int32_t> idx;
  std::vector<float> ll;
  const long unread = feats.Run([&](const xv::FeatBatchReader::Batch& b) {
    if (b.cols != gmm.dim) {
      for (const std::string& key : b.keys) {
        XWARN("Dimension mismatch for utterance " << key << ": the features have " << b.cols << " columns, the model " << gmm.dim);
        ++num_err;
      }
      return;
    }
    const int nu = (int)b.keys.size();
    const size_t rows = (size_t)b.row_off[nu];
    idx.resize(rows * n);
    ll.resize(rows * n);
    xv::UbmGselect(*model, b.feats.data(), b.row_off.data(), nu, n, idx.data(), ll.data());
    for (int u = 0; u < nu; ++u) {
      xv::IntVecVec gs;
      for (int t = b.row_off[u]; t < b.row_off[u + 1]; ++t) {
        gs.emplace_back(idx.begin() + (size_t)t * n, idx.begin() + (size_t)(t + 1) * n);
        tot_like += xv::LogSumExp(ll.data() + (size_t)t * n, n);
      }
      tot_t += b.row_off[u + 1] - b.row_off[u];
      writer.WriteIntVecVec(b.keys[u], gs);
      ++num_done;
    }
  });
  writer.Close();
  XLOG("Done " << num_done << " files, " << unread + num_err << " with errors, average UBM log-likelihood is " << (tot_t ? tot_like / (double)tot_t : 0.0)
               << " over " << tot_t << " frames.");
  return num_done != 0 ? 0 : 1;
}

int GselectToPost(float min_post, int device, const std::vector<std::string>& pos) {
  xv::FullGmmData gmm;
  xv::ReadFullGmmFile(pos[0], &gmm);
  const int dev = xv::PickDevice(device);
  std::unique_ptr<xv::UbmModel> model(xv::UbmFullCreate(dev, gmm.num_gauss, gmm.dim, gmm.gconsts.data(), gmm.means_invcovars.data(), gmm.inv_covars.data()));
  xv::GselectGroupWalk groups(gmm.dim, gmm.num_gauss, pos[1], pos[2]);
  xv::TableWriter writer(pos[3]);
  long num_done = 0;
  double tot_like = 0.0;
  int64_t tot_t = 0;
  std::vector<float> post, logsum;
  std::vector<int32_t> count, idx;
  const long num_err = groups.Run([&](const xv::GselectGroup& g) {
    const int nu = (int)g.keys.size(), n = g.n;
    const size_t rows = (size_t)g.off[nu];
    count.resize(rows);
    idx.resize(rows * n);
    post.resize(rows * n);
    logsum.resize(rows);
    xv::UbmPost(*model, g.feats.data(), g.off.data(), nu, g.gs.data(), n, min_post, count.data(), idx.data(), post.data(), nullptr, logsum.data());
    for (int u = 0; u < nu; ++u) {
      xv::Posterior p;
      for (int t = g.off[u]; t < g.off[u + 1]; ++t) {
        p.emplace_back();
        for (int k = 0; k < count[t]; ++k) p.back().emplace_back(idx[(size_t)t * n + k], post[(size_t)t * n + k]);
        tot_like += logsum[t];
      }
      tot_t += g.off[u + 1] - g.off[u];
      writer.WritePosterior(g.keys[u], p);
      ++num_done;
    }
  });
  writer.Close();
  XLOG("Done " << num_done << " files, " << num_err << " with errors, average log-likelihood per frame is " << (tot_t ? tot_like / (double)tot_t : 0.0)
               << " over " << tot_t << " frames.");
  return num_done != 0 ? 0 : 1;
}

int ScalePost(const std::vector<std::string>& pos) {
  const bool table = xv::IsTable(pos[1]);
  std::unordered_map<std::string, float> scales;
  double global = 1.0;
  if (table) scales = xv::ReadFloatTable(pos[1]);
  else if (!xv::ParseDouble(pos[1], &global)) throw xv::KioError("Bad scale '" + pos[1] + "': expected a number or a table of scales (ark:...)");
  xv::SequentialPosteriorReader reader(pos[0]);
  xv::TableWriter writer(pos[2]);
  long num_done = 0, num_no_scale = 0;
  std::string key, err;
  xv::Posterior p;
  while (reader.Next(&key, &p, &err)) {
    if (!err.empty()) {
      XWARN("Failed to read the posterior of " << key << ": " << err);
      ++num_no_scale;
      continue;
    }
    float scale = (float)global;
    if (table) {
      auto it = scales.find(key);
      if (it == scales.end()) {
        XWARN("No scale available for key " << key);
        ++num_no_scale;
        continue;
      }
      scale = it->second;
    }
    if (scale == 0.f) {
      for (auto& frame : p) frame.clear();
    } else if (scale != 1.f) {
      for (auto& frame : p)
        for (auto& e : frame) e.second *= scale;
    }
    writer.WritePosterior(key, p);
    ++num_done;
  }
  writer.Close();
  XLOG("Done " << num_done << " posteriors;  " << num_no_scale << " had no scales.");
  return num_done != 0 ? 0 : 1;
}

int GmmCopy(bool full, bool binary, const std::vector<std::string>& pos) {
  if (full) {
    xv::FullGmmData m;
    xv::ReadFullGmmFile(pos[0], &m);
    xv::WriteFullGmmFile(pos[1], binary, m);
  } else {
    xv::DiagGmmData m;
    xv::ReadDiagGmmFile(pos[0], &m);
    xv::WriteDiagGmmFile(pos[1], binary, m);
  }
  XLOG("Written model to " << pos[1]);
  return 0;
}

int CopyGselect(int n, const std::vector<std::string>& pos) {
  if (n == 0 || n < -1) throw xv::KioError("--n must be positive, or -1 to keep every index");
  xv::SequentialGselectReader reader(pos[0]);
  xv::TableWriter writer(pos[1]);
  long num_done = 0, num_err = 0;
  std::string key, err;
  xv::IntVecVec v;
  while (reader.Next(&key, &v, &err)) {
    if (!err.empty()) {
      XWARN("Failed to read the Gaussian selection of " << key << ": " << err);
      ++num_err;
      continue;
    }
    if (n > 0)
      for (auto& l : v)
        if ((int)l.size() > n) l.resize((size_t)n);
    writer.WriteIntVecVec(key, v);
    ++num_done;
  }
  writer.Close();
  XLOG("Copied " << num_done << " gselect entries, " << num_err << " had errors.");
  return num_done != 0 ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
  using Pos = std::vector<std::string>;
  DeltaOptions d;
  bool binary = true;
  int copy_n = -1, select_n = 50, device = -1;
  float min_post = 0.f;
  const std::vector<xv::CliTool> tools = {
      {"add-deltas",
       "Add deltas (typically to raw mfcc or plp features).\n"
       "Usage: add-deltas [options] <feats-rspecifier> <feats-wspecifier>\n"
       "Options: --delta-order (2) --delta-window (2) --truncate (0) --device=<gpu>\n",
       {xv::Int("delta-order", &d.order), xv::Int("delta-window", &d.window), xv::Int("truncate", &d.truncate), xv::Int("device", &d.device)},
       2, 2, [&](const Pos& pos) { return AddDeltas(d, pos); }},
      {"fgmm-global-to-gmm",
       "Convert single full-covariance GMM to single diagonal-covariance GMM.\n"
       "Usage: fgmm-global-to-gmm [options] <full-gmm-in> <diag-gmm-out>\n"
       "Options: --binary (true)\n",
       {xv::Bool("binary", &binary)}, 2, 2, [&](const Pos& pos) { return FgmmToGmm(binary, pos); }},
      {"fgmm-global-copy", "Copy a full-covariance GMM.\nUsage: fgmm-global-copy [options] <model-in> <model-out>\nOptions: --binary (true)\n",
       {xv::Bool("binary", &binary)}, 2, 2, [&](const Pos& pos) { return GmmCopy(true, binary, pos); }},
      {"gmm-global-copy", "Copy a diagonal-covariance GMM.\nUsage: gmm-global-copy [options] <model-in> <model-out>\nOptions: --binary (true)\n",
       {xv::Bool("binary", &binary)}, 2, 2, [&](const Pos& pos) { return GmmCopy(false, binary, pos); }},
      {"copy-gselect",
       "Copy Gaussian indices for pruning, possibly making the lists shorter.\n"
       "Usage: copy-gselect [options] <gselect-rspecifier> <gselect-wspecifier>\nOptions: --n (-1)\n",
       {xv::Int("n", &copy_n)}, 2, 2, [&](const Pos& pos) { return CopyGselect(copy_n, pos); }},
      {"fgmm-global-gselect-to-post",
       "Given features and Gaussian-selection (gselect) information for a full-covariance GMM, output per-frame posteriors\n"
       "for the selected indices.\n"
       "Usage: fgmm-global-gselect-to-post [options] <full-gmm-in> <feats-rspecifier> <gselect-rspecifier> <post-wspecifier>\n"
       "Options: --min-post (0.0) --device=<gpu>\n",
       {xv::Float("min-post", &min_post), xv::Int("device", &device)}, 4, 4, [&](const Pos& pos) { return GselectToPost(min_post, device, pos); },
       "gselect-to-post"},
      {"gmm-gselect",
       "Precompute Gaussian indices for pruning (e.g. in training UBMs, SGMMs, tied-mixture systems).\n"
       "For each frame, gives a list of the n best Gaussian indices, sorted from best to worst.\n"
       "Usage: gmm-gselect [options] <model-in> <feature-rspecifier> <gselect-wspecifier>\n"
       "Options: --n (50; at most 64) --device=<gpu>\n"
       "Not built (refused): --write-likes, --gselect.\n",
       {xv::Int("n", &select_n), xv::Int("device", &device), xv::Refused("write-likes", "--write-likes is not built: no script of the recipes passes it"),
        xv::Refused("gselect", "--gselect is not built: no script of the recipes passes it")},
       3, 3, [&](const Pos& pos) { return GmmGselect(select_n, device, pos); }},
      {"scale-post",
       "Scale all the posteriors of a table, by one scale or by a scale per utterance.\n"
       "Usage: scale-post <post-rspecifier> (<scale-rspecifier>|<scale>) <post-wspecifier>\n",
       {}, 3, 3, [&](const Pos& pos) { return ScalePost(pos); }},
  };
  // in this order: a name that holds "fgmm-global-gselect-to-post" holds "gmm-gselect" too
  return xv::ToolsMain(argc, argv, tools, xv::NameRule::kContains, "scale-post");
}
