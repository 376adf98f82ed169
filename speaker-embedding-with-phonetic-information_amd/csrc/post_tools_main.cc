// logprob-to-post / fgmm-global-acc-stats-post / fgmm-global-init-from-accs / nnet3-info - drop-in command lines for the phonetic
// i-vector path (egs/sre/v1: sid/extract_post_nnet3.sh:85-91, sid/init_full_ubm_from_nnet3.sh:91-136).  One executable,
// dispatching on its exact base name:
//   logprob-to-post [--min-post=0.01 --random-prune=true] <logprob-matrix-rspecifier> <posterior-wspecifier>
//   fgmm-global-acc-stats-post [--binary=true --update-flags=mvw] <posterior-rspecifier> <num-components> <feats-rspecifier> <stats-out>
//   fgmm-global-init-from-accs [--binary=true --remove-low-count-gaussians=true ...] <stats-in> <num-components> <model-out>
//   nnet3-info <raw-nnet-rxfilename>
// Semantics: post.h.  The first two run on the device and fail without a GPU (exit 255); the others are host code and open no
// device.  Refused by name: fgmm-global-acc-stats-post --weights, fgmm-global-init-from-accs --mix-up other than 0.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "cli.h"
#include "feat.h"
#include "feat_join.h"
#include "gmm_train.h"
#include "kio.h"
#include "nnet3_raw.h"
#include "post.h"
#include "program.h"
#include "ubm.h"
#include "ubm_train.h"
#include "ubm_train_kernels.h"

namespace {

// ------------------------------------------------------------------------------------------------------------ logprob-to-post
struct PostOptions {
  float min_post = 0.01f;
  bool random_prune = true;
  int device = -1;
};

int LogprobToPost(const PostOptions& o, const std::vector<std::string>& pos) {
  const int dev = xv::PickDevice(o.device);
  xv::SequentialMatrixReader reader(pos[0]);
  xv::TableWriter writer(pos[1]);
  long num_done = 0, num_err = 0;
  int64_t frames = 0, pairs = 0, num_nan = 0;
  // the utterances of the next device call: one width, up to the frame budget of a launch
  std::vector<std::string> keys;
  std::vector<int32_t> row_off(1, 0);
  std::vector<float> x;
  int cols = 0;
  auto flush = [&] {
    if (keys.empty()) return;
    std::vector<uint64_t> seeds;
    for (const std::string& k : keys) seeds.push_back(xv::UttSeed(k.c_str()));
    xv::LogprobPostResult r;
    xv::LogprobToPost(dev, x.data(), row_off.data(), (int)keys.size(), cols, seeds.data(), o.min_post, o.random_prune, 0, false, &r);
    for (size_t u = 0; u < keys.size(); ++u) {
      xv::Posterior post((size_t)(row_off[u + 1] - row_off[u]));
      for (int32_t t = row_off[u]; t < row_off[u + 1]; ++t) {
        auto& frame = post[(size_t)(t - row_off[u])];
        for (int64_t i = r.off[(size_t)t]; i < r.off[(size_t)t + 1]; ++i) frame.emplace_back(r.idx[(size_t)i], r.w[(size_t)i]);
      }
      writer.WritePosterior(keys[u], post);
      ++num_done;
    }
    frames += row_off.back();
    pairs += r.off.back();
    num_nan += r.num_nan;
    keys.clear();
    row_off.assign(1, 0);
    x.clear();
  };
  std::string key, err;
  xv::Matrix m;
  while (reader.Next(&key, &m, &err)) {
    if (!err.empty()) {
      XWARN("Failed to read the matrix of " << key << ": " << err);
      ++num_err;
      continue;
    }
    if (m.cm) {
      xv::Matrix full;
      xv::ExpandCompressedView(m, &full);
      m = full;
    }
    if (m.rows == 0 || m.cols == 0) {   // nothing for the device: an empty posterior, in its place among the others
      if (keys.empty()) {
        writer.WritePosterior(key, xv::Posterior());
        ++num_done;
      } else {
        keys.push_back(key);
        row_off.push_back(row_off.back());
      }
      continue;
    }
    if (!keys.empty() && (m.cols != cols || row_off.back() + (int64_t)m.rows > INT32_MAX)) flush();
    cols = m.cols;
    keys.push_back(key);
    x.insert(x.end(), m.Data(), m.Data() + (size_t)m.rows * m.cols);
    row_off.push_back(row_off.back() + m.rows);
    if (row_off.back() >= xv::LogprobPostDefaultBudget(cols)) flush();
  }
  flush();
  writer.Close();
  if (num_nan) XWARN(num_nan << " log-probabilities were NaN and were dropped");
  XLOG("Done " << num_done << " utterances; " << num_err << " with errors.");
  XLOG(frames << " frames in, " << pairs << " pairs out, " << (frames ? (double)pairs / (double)frames : 0.0) << " pairs per frame.");
  return num_done != 0 ? 0 : 1;
}

// ------------------------------------------------------------------------------------------------- fgmm-global-acc-stats-post
struct AccOptions {
  bool binary = true;
  std::string update_flags = "mvw";
  int device = -1;
};

int ParseNumComponents(const std::string& s) {
  int g = 0;
  if (!xv::ParseInt(s, &g) || g < 1) throw xv::KioError("<num-components> must be a positive integer, not '" + s + "'");
  return g;
}

int AccStatsPost(const AccOptions& o, const std::vector<std::string>& pos) {
  const int flags = xv::ParseGmmFlags(o.update_flags);
  const int G = ParseNumComponents(pos[1]);
  xv::PosteriorLookup posts(pos[0]);
  // (the accumulate calls do not depend on the frames read ahead; a matrix without rows is skipped, not an error)
  xv::FeatBatchWalk walk(pos[2], xv::kBatchFrames, false, xv::FeatProblems::kCountUnreadable);
  std::unique_ptr<xv::FgmmAccumulator> acc;
  xv::FgmmAccs host;
  int D = 0;
  long num_done = 0, num_err = 0;
  // the stream of accepted frames, cut into blocks of exactly kFgmmAccFrameBlock: what is pending is less than one block
  std::vector<float> feats, w;
  std::vector<int32_t> idx, off(1, 0);
  auto block = [&](size_t rows) {   // the first `rows` pending frames
    std::vector<int32_t> o2(off.begin(), off.begin() + rows + 1);
    xv::FgmmAccAdd(acc.get(), feats.data(), (int64_t)rows, o2.data(), idx.data(), w.data());
    const int32_t used = off[rows];
    feats.erase(feats.begin(), feats.begin() + rows * D);
    idx.erase(idx.begin(), idx.begin() + used);
    w.erase(w.begin(), w.begin() + used);
    off.erase(off.begin(), off.begin() + rows);
    for (int32_t& v : off) v -= used;
  };
  const long unread = walk.Run([&](const xv::FeatBatchReader::Batch& b) {
    for (size_t u = 0; u < b.keys.size(); ++u) {
      const int rows = b.row_off[u + 1] - b.row_off[u];
      if (!acc) {   // the first utterance gives the dimension
        D = b.cols;
        acc.reset(xv::FgmmAccCreate(xv::PickDevice(o.device), G, D, flags));
        host.Init(G, D, flags);
      }
      if (b.cols != D) {
        XWARN("Dimension mismatch for utterance " << b.keys[u] << ": the features have " << b.cols << " columns, the utterances before it " << D);
        ++num_err;
        continue;
      }
      xv::Posterior post;
      const xv::Joined j = xv::FindFrames(&posts, b.keys[u], rows, &post);
      if (j.outcome == xv::Joined::kNotFound) XWARN("No posterior for utterance " << b.keys[u]);
      else if (j.outcome != xv::Joined::kOk) XWARN("The posterior of utterance " << b.keys[u] << " has wrong size " << j.size << " vs. " << rows);
      if (j.outcome != xv::Joined::kOk) {
        ++num_err;
        continue;
      }
      for (size_t t = 0; t < post.size(); ++t)
        for (const auto& pr : post[t])
          if (pr.first < 0 || pr.first >= G)
            throw xv::KioError("the posterior of utterance " + b.keys[u] + " names Gaussian " + std::to_string(pr.first) + " at frame " + std::to_string(t) +
                               "; <num-components> is " + std::to_string(G));
      xv::AppendRows(b, u, &feats);
      xv::Append(post, &off, &idx, &w);
      while (off.size() - 1 >= (size_t)xv::kFgmmAccFrameBlock) block((size_t)xv::kFgmmAccFrameBlock);
      ++num_done;
    }
  });
  if (off.size() > 1) block(off.size() - 1);
  XLOG("Done " << num_done << " files; " << unread + num_err << " with errors.");
  if (!acc) {
    XWARN("No statistics were accumulated: nothing is written");
    return 1;
  }
  xv::FgmmAccGet(*acc, host.occ.data(), host.mean.data(), host.second.data());
  xv::WriteGmmAccsFile(pos[3], o.binary, host);
  XLOG("Written accs to " << pos[3]);
  return num_done != 0 ? 0 : 1;
}

// ------------------------------------------------------------------------------------------------- fgmm-global-init-from-accs
int InitFromAccs(bool binary, bool remove_low_count, const std::vector<std::string>& pos) {
  const int G = ParseNumComponents(pos[1]);
  xv::FgmmAccs accs;
  xv::ReadGmmAccsFile(pos[0], false, &accs);
  if (accs.num_gauss != G)
    throw xv::KioError("the statistics have " + std::to_string(accs.num_gauss) + " Gaussians, <num-components> is " + std::to_string(G));
  xv::FullGmmData gmm;
  xv::FgmmInitResult r;
  xv::FgmmInitFromAccs(accs, remove_low_count, &gmm, &r);
  for (const std::string& w : r.warnings) XWARN(w);
  XLOG("Initialised " << gmm.num_gauss << " Gaussians of dimension " << gmm.dim << "; " << r.removed.size() << " removed, " << r.bad_gconsts << " bad gconsts.");
  xv::WriteFullGmmFile(pos[2], binary, gmm);
  XLOG("Written model to " << pos[2]);
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------ nnet3-info
// The (input, output) dimension of every component node; the nodes of a network read from several configs are in no particular order.
struct NodeDims {
  const xv::RawNnet& net;
  std::map<std::string, std::pair<int, int>> memo;
  std::map<std::string, bool> open;   // the nodes on the way: a cycle is an error, not a recursion without end

  int Descriptor(const std::string& text) {
    int d = 0;
    for (const xv::DescTerm& t : xv::FlattenDescriptor(text)) d += Of(t.node).second;
    return d;
  }
  std::pair<int, int> Of(const std::string& name) {
    auto it = memo.find(name);
    if (it != memo.end()) return it->second;
    if (const xv::RawNode* in = net.FindNode(name, "input-node")) return memo[name] = {in->dim, in->dim};
    const xv::RawNode* n = net.FindNode(name, "component-node");
    if (!n) throw xv::KioError("the graph refers to the unknown node '" + name + "'");
    if (open[name]) throw xv::KioError("the graph has a cycle through the node '" + name + "'");
    open[name] = true;
    const xv::RawComponent* c = net.FindComponent(n->component);
    if (!c) throw xv::KioError("node '" + n->name + "' refers to unknown component '" + n->component + "'");
    const int from_graph = Descriptor(n->input);
    int in = from_graph, od = from_graph;
    if (c->has_linear) {
      in = c->linear.cols;
      od = c->linear.rows;
    } else if (c->type == "StatisticsExtractionComponent") {
      in = (int)c->Get("<InputDim>", from_graph);
      od = 1 + in * (c->Get("<IncludeVarinance>", 1) != 0.0 ? 2 : 1);
    } else if (c->type == "StatisticsPoolingComponent") {
      in = (int)c->Get("<InputDim>", from_graph);
      od = in - 1 + (int)c->Get("<NumLogCountFeatures>", 0);
    } else {
      in = od = (int)c->Get("<Dim>", from_graph);
    }
    if (in != from_graph)
      throw xv::KioError("component-node " + n->name + ": its input " + n->input + " has dimension " + std::to_string(from_graph) + ", its component takes " + std::to_string(in));
    open[name] = false;
    return memo[name] = {in, od};
  }
};

int Nnet3Info(const std::string& rxfilename) {
  xv::RawNnet net;
  net.ReadFrom(rxfilename);
  int64_t params = 0;
  for (const xv::RawComponent& c : net.components) params += (int64_t)c.linear.data.size() + (int64_t)c.bias.size();
  std::string out = "num-parameters: " + std::to_string(params) + "\n";
  NodeDims dims{net, {}, {}};
  std::map<std::string, std::pair<int, int>> comp_dims;        // component -> (input, output) dimension, from its nodes
  std::vector<std::string> outputs;
  for (const xv::RawNode& n : net.nodes) {
    if (n.kind == "input-node") {
      out += "input-node name=" + n.name + " dim=" + std::to_string(n.dim) + "\n";
    } else if (n.kind == "component-node") {
      const std::pair<int, int> d = dims.Of(n.name);
      comp_dims[n.component] = d;
      out += "component-node name=" + n.name + " component=" + n.component + " input=" + n.input + " input-dim=" + std::to_string(d.first) + " output-dim=" + std::to_string(d.second) + "\n";
    } else if (n.kind == "output-node") {
      out += "output-node name=" + n.name + " input=" + n.input + " dim=" + std::to_string(dims.Descriptor(n.input)) + " objective=linear\n";
      outputs.push_back(n.name);
    } else {
      throw xv::KioError("node '" + n.name + "' is a " + n.kind + ", which the reader of this library does not evaluate");
    }
  }
  for (const xv::RawComponent& c : net.components) {
    out += "component name=" + c.name + " type=" + c.type;
    auto it = comp_dims.find(c.name);
    if (it != comp_dims.end()) out += ", input-dim=" + std::to_string(it->second.first) + ", output-dim=" + std::to_string(it->second.second);
    out += "\n";
  }
  // what the extractor makes of every output it can run
  for (const std::string& name : outputs) {
    std::string d;
    try {
      d = xv::LowerToProgram(net, name).Describe();   // the text of xv_model_describe
    } catch (const xv::KioError& e) {
      out += "# " + name + ": not lowered (" + e.what() + ")\n";
      continue;
    }
    size_t a = 0;
    while (a < d.size()) {
      const size_t e = d.find('\n', a);
      out += "# " + name + ": " + d.substr(a, e == std::string::npos ? std::string::npos : e - a) + "\n";
      if (e == std::string::npos) break;
      a = e + 1;
    }
  }
  fputs(out.c_str(), stdout);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  using Pos = std::vector<std::string>;
  bool binary = true, remove_low_count = true;
  PostOptions p;
  AccOptions o;
  const char* no_mix_up = "--mix-up is not built: no script of the recipes increases the number of Gaussians here";
  const std::vector<xv::CliTool> tools = {
      {"logprob-to-post",
       "Convert a matrix of log-probabilities (e.g. from nnet-logprob) to posteriors\n"
       "Usage: logprob-to-post [options] <logprob-matrix-rspecifier> <posteriors-wspecifier>\n"
       "Options: --min-post (0.01) --random-prune (true) --device=<gpu>\n",
       {xv::Float("min-post", &p.min_post), xv::Bool("random-prune", &p.random_prune), xv::Int("device", &p.device)},
       2, 2, [&](const Pos& pos) { return LogprobToPost(p, pos); }},
      {"fgmm-global-acc-stats-post",
       "Accumulate stats for training a full-covariance GMM, given posteriors\n"
       "Usage: fgmm-global-acc-stats-post [options] <posterior-rspecifier> <number-of-components> <feature-rspecifier> <stats-out>\n"
       "Options: --binary (true) --update-flags (mvw) --device=<gpu>\n"
       "Not built (refused): --weights.\n",
       {xv::Bool("binary", &o.binary), xv::String("update-flags", &o.update_flags), xv::Int("device", &o.device),
        xv::Refused("weights", "--weights is not built: no script of the recipes passes per-frame weights")},
       4, 4, [&](const Pos& pos) { return AccStatsPost(o, pos); }},
      {"fgmm-global-init-from-accs",
       "Initialize a full-covariance GMM from the accumulated stats.\n"
       "Usage: fgmm-global-init-from-accs [options] <stats-in> <number-of-components> <model-out>\n"
       "Options: --binary (true) --remove-low-count-gaussians (true)\n"
       "Accepted and without effect here, as in fgmm-global-est's option set: --update-flags --min-gaussian-weight\n"
       "         --min-gaussian-occupancy --variance-floor --max-condition\n"
       "Not built (refused): --mix-up other than 0.\n",
       {xv::Bool("binary", &binary), xv::Bool("remove-low-count-gaussians", &remove_low_count),
        xv::Custom("update-flags", [](const std::string&, const std::string& val) { return xv::ParseGmmFlags(val), true; }),
        xv::Double("min-gaussian-weight", nullptr), xv::Double("min-gaussian-occupancy", nullptr), xv::Double("variance-floor", nullptr),
        xv::Double("max-condition", nullptr), xv::RefusedIfNonZero("mix-up", no_mix_up)},
       3, 3, [&](const Pos& pos) { return InitFromAccs(binary, remove_low_count, pos); }},
      {"nnet3-info",
       "Print some text information about 'raw' nnet3 neural network, to standard output\n"
       "Usage: nnet3-info <raw-nnet-rxfilename>\n"
       "e.g.: nnet3-info \"nnet3-am-copy --raw=true final.mdl - |\"\n",
       {}, 0, -1, [&](const Pos& pos) {
         // sid/init_full_ubm_from_nnet3.sh:91 passes $nnet_raw unquoted: the words of "nnet3-am-copy --raw=true final.mdl - |" arrive
         // one by one, and are put together again
         std::string rx = pos.empty() ? "" : pos[0];
         if (pos.size() > 1 && pos.back() == "|")
           for (size_t i = 1; i < pos.size(); ++i) rx += " " + pos[i];
         else if (pos.size() != 1) return (int)xv::kUsageError;
         return Nnet3Info(rx);
       }},
  };
  return xv::ToolsMain(argc, argv, tools, xv::NameRule::kExactOrRefuse);
}
