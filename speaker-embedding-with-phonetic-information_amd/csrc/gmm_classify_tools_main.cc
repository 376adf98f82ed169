// fgmm-gselect / fgmm-global-get-frame-likes / compute-vad-from-frame-likes / merge-vads / fgmm-global-info - drop-in command lines
// for the GMM classifiers of the i-vector baseline (egs/sre/v1: sid/gender_id.sh:68-118, sid/music_id.sh:73-104,
// sid/compute_vad_decision_gmm.sh:91-127).  One executable, dispatching on its name:
//   fgmm-gselect [--n=50 --gselect=<rspecifier>] <full-gmm-in> <feats-rspecifier> <gselect-wspecifier>
//   fgmm-global-get-frame-likes [--gselect=<rspecifier> --average=false] <full-gmm-in> <feats-rspecifier> <likes-wspecifier>
//   compute-vad-from-frame-likes [--map=<file> --priors=<p0,p1,...>] <likes-rspecifier-1> ... <likes-rspecifier-n> <vad-wspecifier>
//   merge-vads [--map=<file>] <vad-rspecifier-1> <vad-rspecifier-2> <vad-wspecifier>
//   fgmm-global-info <full-gmm-in>
// The first two run on the device (gmm_classify.h) and fail without a GPU (exit 255); the others are host code and open no device.
// Without --gselect the first two score every component, which the device kernels do for models of at most 64: a larger model is
// refused by name (no script of the recipes omits --gselect).
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "cli.h"
#include "feat_join.h"
#include "gmm_classify.h"
#include "kio.h"
#include "ubm.h"
#include "ubm_kernels.h"

namespace {

void RefuseDense(const char* prog, const xv::FullGmmData& gmm) {
  if (gmm.num_gauss > xv::kUbmMaxSelect)
    throw xv::KioError(std::string(prog) + " without --gselect scores every component, and the model's " + std::to_string(gmm.num_gauss) +
                       " are above the device kernels' limit of " + std::to_string(xv::kUbmMaxSelect) + ": pass --gselect=<rspecifier>");
}

int FgmmGselect(int n_opt, const std::string& gselect_rspecifier, int device, const std::vector<std::string>& pos) {
  if (n_opt < 1) throw xv::KioError("--n must be at least 1");
  xv::FullGmmData gmm;
  xv::ReadFullGmmFile(pos[0], &gmm);
  if (gselect_rspecifier.empty()) RefuseDense("fgmm-gselect", gmm);
  const int dev = xv::PickDevice(device);
  std::unique_ptr<xv::UbmModel> model(xv::UbmFullCreate(dev, gmm.num_gauss, gmm.dim, gmm.gconsts.data(), gmm.means_invcovars.data(), gmm.inv_covars.data()));
  xv::TableWriter writer(pos[2]);
  xv::GselectGroupWalk groups(gmm.dim, gmm.num_gauss, pos[1], gselect_rspecifier);
  long num_done = 0;
  double tot_like = 0.0;
  int64_t tot_t = 0;
  bool warned = false;
  std::vector<int32_t> idx;
  std::vector<float> ll;
  const long num_err = groups.Run([&](const xv::GselectGroup& g) {
    if (n_opt >= g.n && !warned) {
      XWARN("You asked for " << n_opt << " Gaussians but the preselection only has " << g.n
                             << ", returning this many. Note: this means the Gaussian selection is pointless.");
      warned = true;
    }
    const int nu = (int)g.keys.size(), keep = n_opt < g.n ? n_opt : g.n;
    const size_t rows = (size_t)g.off[nu];
    idx.resize(rows * keep);
    ll.resize(rows * keep);
    xv::UbmFullGselect(*model, g.feats.data(), g.off.data(), nu, g.gs.data(), g.n, n_opt, idx.data(), ll.data());
    for (int u = 0; u < nu; ++u) {
      xv::IntVecVec out;
      for (int t = g.off[u]; t < g.off[u + 1]; ++t) {
        out.emplace_back(idx.begin() + (size_t)t * keep, idx.begin() + (size_t)(t + 1) * keep);
        tot_like += xv::LogSumExp(ll.data() + (size_t)t * keep, keep);
      }
      tot_t += g.off[u + 1] - g.off[u];
      writer.WriteIntVecVec(g.keys[u], out);
      ++num_done;
    }
  });
  writer.Close();
  XLOG("Done " << num_done << " files, " << num_err << " with errors, average UBM log-likelihood is " << (tot_t ? tot_like / (double)tot_t : 0.0)
               << " over " << tot_t << " frames.");
  return num_done != 0 ? 0 : 1;
}

int GetFrameLikes(bool average, const std::string& gselect_rspecifier, int device, const std::vector<std::string>& pos) {
  xv::FullGmmData gmm;
  xv::ReadFullGmmFile(pos[0], &gmm);
  if (gselect_rspecifier.empty()) RefuseDense("fgmm-global-get-frame-likes", gmm);
  const int dev = xv::PickDevice(device);
  std::unique_ptr<xv::UbmModel> model(xv::UbmFullCreate(dev, gmm.num_gauss, gmm.dim, gmm.gconsts.data(), gmm.means_invcovars.data(), gmm.inv_covars.data()));
  xv::TableWriter writer(pos[2]);
  xv::GselectGroupWalk groups(gmm.dim, gmm.num_gauss, pos[1], gselect_rspecifier);
  long num_done = 0;
  double tot_like = 0.0;
  int64_t tot_t = 0;
  std::vector<float> likes;
  const long num_err = groups.Run([&](const xv::GselectGroup& g) {
    const int nu = (int)g.keys.size();
    likes.resize((size_t)g.off[nu]);
    xv::UbmFrameLikes(*model, g.feats.data(), g.off.data(), nu, g.gs.data(), g.n, likes.data());
    for (int u = 0; u < nu; ++u) {
      const int rows = g.off[u + 1] - g.off[u];
      double sum = 0.0;   // in frame order: the average does not depend on the batch the utterance was in
      for (int t = g.off[u]; t < g.off[u + 1]; ++t) sum += (double)likes[t];
      tot_like += sum;
      tot_t += rows;
      if (average) writer.WriteFloat(g.keys[u], (float)(sum / (double)rows));
      else writer.WriteVec(g.keys[u], likes.data() + g.off[u], rows);
      ++num_done;
    }
  });
  writer.Close();
  XLOG("Done " << num_done << " files; " << num_err << " with errors.");
  XLOG("Overall likelihood per frame = " << (tot_t ? tot_like / (double)tot_t : 0.0) << " over " << tot_t << " frames.");
  return num_done != 0 ? 0 : 1;
}

// the words of a text file's lines, as integers: `per_line` of them on every line that is not blank
std::vector<int32_t> ReadIntLines(const std::string& path, int per_line, const char* what) {
  FILE* f = fopen(path.c_str(), "r");
  if (!f) throw xv::KioError(std::string("cannot open the ") + what + " " + path);
  std::vector<int32_t> out;
  char line[1024];
  while (fgets(line, sizeof line, f)) {
    std::vector<int32_t> row;
    char* p = line;
    for (;;) {
      while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') ++p;
      if (!*p) break;
      char* end = nullptr;
      const long v = strtol(p, &end, 10);
      if (end == p || (*end && !isspace((unsigned char)*end))) {
        fclose(f);
        throw xv::KioError(std::string("bad line in the ") + what + " " + path + ": " + line);
      }
      row.push_back((int32_t)v);
      p = end;
    }
    if (row.empty()) continue;
    if ((int)row.size() != per_line) {
      fclose(f);
      throw xv::KioError(std::string("a line of the ") + what + " " + path + " does not have " + std::to_string(per_line) + " integers: " + line);
    }
    out.insert(out.end(), row.begin(), row.end());
  }
  fclose(f);
  return out;
}

int VadFromFrameLikes(const std::string& map_file, const std::string& priors_str, const std::vector<std::string>& pos) {
  const int n = (int)pos.size() - 1;
  std::vector<float> priors;
  for (size_t a = 0; a < priors_str.size();) {
    size_t e = priors_str.find(',', a);
    if (e == std::string::npos) e = priors_str.size();
    double v;
    if (!xv::ParseDouble(priors_str.substr(a, e - a), &v)) throw xv::KioError("Invalid --priors=" + priors_str + ": a comma-separated list of numbers");
    priors.push_back((float)v);
    a = e + 1;
  }
  if (!priors.empty() && (int)priors.size() != n)
    throw xv::KioError("--priors has " + std::to_string(priors.size()) + " entries for " + std::to_string(n) + " tables of frame likelihoods");
  for (float p : priors)
    if (!(p > 0.f)) throw xv::KioError("--priors=" + priors_str + ": every prior must be positive");
  std::vector<int32_t> map;
  if (!map_file.empty()) {
    const std::vector<int32_t> lines = ReadIntLines(map_file, 2, "map");
    std::vector<bool> have((size_t)n, false);
    map.assign((size_t)n, 0);
    for (size_t i = 0; i + 1 < lines.size(); i += 2) {
      if (lines[i] < 0 || lines[i] >= n) continue;   // a line for a class nobody passed
      map[lines[i]] = lines[i + 1];
      have[lines[i]] = true;
    }
    for (int j = 0; j < n; ++j)
      if (!have[j]) throw xv::KioError("the map " + map_file + " has no line for index " + std::to_string(j));
  }
  xv::SequentialVectorReader first(pos[0]);
  std::vector<std::unique_ptr<xv::RandomAccessVectorReader>> others;
  for (int j = 1; j < n; ++j) others.emplace_back(new xv::RandomAccessVectorReader(pos[j]));
  xv::TableWriter writer(pos[n]);
  long num_done = 0, num_err = 0;
  std::string key, err;
  std::vector<float> v0, out;
  std::vector<const float*> likes((size_t)n);
  while (first.Next(&key, &v0, &err)) {
    if (!err.empty()) {
      XWARN("Failed to read the frame likelihoods of " << key << ": " << err);
      ++num_err;
      continue;
    }
    likes[0] = v0.data();
    bool ok = true;
    for (int j = 1; j < n && ok; ++j) {
      if (!others[j - 1]->HasKey(key)) {
        XWARN("No frame likelihoods for utterance " << key << " in " << pos[j] << " (skipping utterance)");
        ok = false;
        break;
      }
      const std::vector<float>& vj = others[j - 1]->Value(key);
      if (vj.size() != v0.size()) {
        XWARN("Mismatch in the number of frames for utterance " << key << ": " << v0.size() << " in " << pos[0] << ", " << vj.size() << " in " << pos[j]);
        ok = false;
        break;
      }
      likes[j] = vj.data();
    }
    if (!ok) {
      ++num_err;
      continue;
    }
    out.resize(v0.size());
    xv::VadFromFrameLikes(n, likes.data(), (int64_t)v0.size(), priors.empty() ? nullptr : priors.data(), map.empty() ? nullptr : map.data(), out.data());
    writer.WriteVec(key, out.data(), (int)out.size());
    ++num_done;
  }
  writer.Close();
  XLOG("Done " << num_done << " files; " << num_err << " with errors.");
  return num_done != 0 ? 0 : 1;
}

int MergeVads(const std::string& map_file, const std::vector<std::string>& pos) {
  std::vector<int32_t> triples;
  if (!map_file.empty()) {
    triples = ReadIntLines(map_file, 3, "map");
    if (triples.empty()) throw xv::KioError("the map " + map_file + " has no lines");
  }
  xv::SequentialVectorReader first(pos[0]);
  xv::RandomAccessVectorReader second(pos[1]);
  xv::TableWriter writer(pos[2]);
  long num_done = 0, num_err = 0;
  std::string key, err;
  std::vector<float> a, out;
  while (first.Next(&key, &a, &err)) {
    if (!err.empty()) {
      XWARN("Failed to read the VAD decisions of " << key << ": " << err);
      ++num_err;
      continue;
    }
    if (!second.HasKey(key)) {
      XWARN("No VAD decisions for utterance " << key << " in " << pos[1] << " (skipping utterance)");
      ++num_err;
      continue;
    }
    const std::vector<float>& b = second.Value(key);
    if (b.size() != a.size()) {
      XWARN("Mismatch in the number of frames for utterance " << key << ": " << a.size() << " versus " << b.size());
      ++num_err;
      continue;
    }
    out.resize(a.size());
    xv::MergeVads(a.data(), b.data(), (int64_t)a.size(), triples.empty() ? nullptr : triples.data(), (int)(triples.size() / 3), out.data());
    writer.WriteVec(key, out.data(), (int)out.size());
    ++num_done;
  }
  writer.Close();
  XLOG("Done " << num_done << " files; " << num_err << " with errors.");
  return num_done != 0 ? 0 : 1;
}

int FgmmInfo(const std::vector<std::string>& pos) {
  xv::FullGmmData gmm;
  xv::ReadFullGmmFile(pos[0], &gmm);
  printf("number of gaussians %d\nfeature dimension %d\n", gmm.num_gauss, gmm.dim);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  using Pos = std::vector<std::string>;
  std::string map_file, priors, gselect;
  bool average = false;
  int n_opt = 50, device = -1;
  const std::vector<xv::CliTool> tools = {
      {"compute-vad-from-frame-likes",
       "Compute per-frame class decisions from the frame log-likelihoods of several models.\n"
       "Usage: compute-vad-from-frame-likes [options] <likes-rspecifier-1> ... <likes-rspecifier-n> <vad-wspecifier>\n"
       "Options: --map=<file of 'index label' lines> --priors=<p0,p1,...>\n",
       {xv::String("map", &map_file), xv::String("priors", &priors)}, 2, -1, [&](const Pos& pos) { return VadFromFrameLikes(map_file, priors, pos); }},
      {"merge-vads",
       "Merge two tables of per-frame decisions: 1 where both are 1, or by a map of 'a b c' lines (the pair (a, b) gives c).\n"
       "Usage: merge-vads [options] <vad-rspecifier-1> <vad-rspecifier-2> <vad-wspecifier>\n"
       "Options: --map=<file>\n",
       {xv::String("map", &map_file)}, 3, 3, [&](const Pos& pos) { return MergeVads(map_file, pos); }},
      {"fgmm-global-info", "Write to standard output various properties of a full-covariance GMM.\nUsage: fgmm-global-info <model-in>\n",
       {}, 1, 1, [&](const Pos& pos) { return FgmmInfo(pos); }},
      {"fgmm-global-get-frame-likes",
       "Print out per-frame log-likelihoods for each utterance, as an archive of vectors of floats.  If --average=true, prints\n"
       "out the average per-frame log-likelihood for each utterance, as a single float.\n"
       "Usage: fgmm-global-get-frame-likes [options] <model-in> <feature-rspecifier> <likes-out-wspecifier>\n"
       "Options: --gselect=<rspecifier> (without it: models of at most 64 components) --average (false) --device=<gpu>\n",
       {xv::Bool("average", &average), xv::String("gselect", &gselect), xv::Int("device", &device)},
       3, 3, [&](const Pos& pos) { return GetFrameLikes(average, gselect, device, pos); }, "get-frame-likes"},
      {"fgmm-gselect",
       "Precompute Gaussian indices for pruning, by the full-covariance model, usually on top of a first selection by its\n"
       "diagonal form (--gselect).  For each frame, gives a list of the n best Gaussian indices, sorted from best to worst.\n"
       "Usage: fgmm-gselect [options] <model-in> <feature-rspecifier> <gselect-wspecifier>\n"
       "Options: --n (50) --gselect=<rspecifier> (at most 64 per frame; without it: models of at most 64 components) --device=<gpu>\n",
       {xv::Int("n", &n_opt), xv::String("gselect", &gselect), xv::Int("device", &device)},
       3, 3, [&](const Pos& pos) { return FgmmGselect(n_opt, gselect, device, pos); }},
  };
  return xv::ToolsMain(argc, argv, tools, xv::NameRule::kContains, "fgmm-gselect");
}
